"""Which doc -> posting lookup structure the seal gives a term (segment.cpp: build_term_aux; plan.h: kLook*), without a GPU:
tests/mockhip/lookup_policy.py seals the corpus of tests/test_lookup_structures_gpu.py under that test's whole assignment
matrix against the stand-in HIP runtime (kernels do nothing: the decision is host code) and reads every term back through
nrtgpu_debug_term_lookup of the development library.  The expectations are tests/_lookup_cases.py's: the rule restated from the
comment above build_term_aux for every term, and (kind, shift, bytes) worked out by hand for the terms each case is about --
neither asks the library.  Boundaries the corpus cannot hold are sealed on their own and pinned here."""
import json
import os
import shutil
import subprocess
import sys

import pytest

from tests import _lookup_cases as lc
from tests._lookup_cases import BITS, CELLS, NONE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "nrtsearch_amd", "libnrtgpu.so")
DEV_LIB = os.path.join(ROOT, "nrtsearch_amd", "libnrtgpu_dev.so")


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """{case name: {"terms": [{term id: (kind, shift, bytes)} per segment], "device_bytes": [per segment]}} as the library answered."""
    if not (shutil.which("gcc") and os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h") and os.path.exists(LIB)):
        pytest.skip("gcc, the HIP headers or the built library are not here")
    from nrtsearch_amd import build
    build.build_dev()
    mock = str(tmp_path_factory.mktemp("mockhip") / "libmockhip.so")
    subprocess.run(["gcc", "-O1", "-w", "-fPIC", "-shared", "-I/opt/rocm/include", os.path.join(ROOT, "tests", "mockhip", "mockhip.c"), "-o", mock],
                   check=True)
    e = dict(os.environ, LD_PRELOAD=mock, NRTGPU_LIB_PATH=DEV_LIB)
    for name in ("NRTGPU_PACKED_POSTINGS", "NRTGPU_TEST_LOOKUP_BUDGET_PCT", "NRTGPU_LOOK_POLICY"):
        e.pop(name, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mockhip", "lookup_policy.py")], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "done" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
    out = {}
    for line in r.stdout.split("\n"):
        if line.startswith("CASE "):
            rec = json.loads(line[5:])
            rec["terms"] = [{int(t): tuple(v) for t, v in seg.items()} for seg in rec["terms"]]
            out[rec["name"]] = rec
    return out


@pytest.fixture(scope="module")
def corpus():
    return lc.build_corpus()


def test_the_restated_rule_agrees_with_the_hand_worked_pins(corpus):
    """tests/_lookup_cases.py states the expectations twice; the two must say the same (no library involved)."""
    assert sorted(lc.PINNED) == sorted(c.name for c in lc.MATRIX)
    for case in lc.MATRIX:
        exp = lc.expected_for(case, corpus)
        for si, pins in enumerate(lc.PINNED[case.name]):
            for t, want in pins.items():
                assert exp[si][t] == want, (case.name, si, lc.NAMES[t])
    small12 = lc.expected_for(lc.Case("small12_packed", lc.DEFAULT_POLICY, 12, True), corpus)[2]
    assert {t: small12[t] for t in lc.SMALL12_PACKED_200} == lc.SMALL12_PACKED_200


@pytest.mark.parametrize("case", lc.MATRIX, ids=lambda c: c.name)
def test_every_term_of_the_gpu_matrix_gets_the_intended_structure(answers, corpus, case):
    got = answers[case.name]["terms"]
    exp = lc.expected_for(case, corpus)
    for si, pins in enumerate(lc.PINNED[case.name]):
        for t, want in pins.items():
            assert got[si][t] == want, (case.name, corpus.segments[si].max_doc, lc.NAMES[t], got[si][t], want)
    for si in range(len(corpus.segments)):
        assert got[si] == exp[si], (case.name, corpus.segments[si].max_doc, {lc.NAMES[t]: (got[si][t], exp[si][t]) for t in exp[si] if got[si][t] != exp[si][t]})


def test_the_matrix_reaches_every_kind_for_sparse_and_dense_terms_in_both_layouts(corpus):
    """What the GPU test's matrix is for, from the expectations alone: the dense term (every 2nd doc) and a sparse one (64
    postings in 200 003 docs) each go through records, lookup cells -- the dense one at one doc per cell -- and the tile table,
    with two columns and packed; and one case's budget runs out in the middle of the list."""
    for packed in (False, True):
        seen = {lc.DENSE: set(), lc.P64: set()}
        for case in lc.MATRIX:
            if case.packed != packed:
                continue
            big = lc.expected_for(case, corpus)[2]
            for t in seen:
                seen[t].add(big[t][:2] if t == lc.DENSE else big[t][0])
        assert seen[lc.DENSE] == {(NONE, 0), (BITS, 0), (CELLS, 0)}, (packed, seen)
        assert seen[lc.P64] == {NONE, BITS, CELLS}, (packed, seen)
        small = lc.expected_for(next(c for c in lc.MATRIX if c.packed == packed and c.name.startswith("default_small")), corpus)[2]
        order = sorted((t for t in small if t not in (lc.P63, lc.LAST32)), key=lambda t: -len(corpus.segments[2].postings(t)[0]))
        kinds = [small[t][0] for t in order]
        assert kinds[:2] == [BITS, BITS] and NONE in kinds[2:] and kinds.index(NONE) < max(i for i, k in enumerate(kinds) if k != NONE)


def test_device_bytes_follow_the_structures(answers, corpus):
    """A segment's device bytes = those of the same segment without any structure + the structures' bytes (+ 64 of slack behind
    the group's one buffer): a budget or policy knob that silently does nothing shows here."""
    for case in lc.MATRIX:
        base = answers[f"default_none_{'packed' if case.packed else 'plain'}"]["device_bytes"]
        exp = lc.expected_for(case, corpus)
        for si in range(len(corpus.segments)):
            look = sum(b for _, _, b in exp[si].values())
            assert answers[case.name]["device_bytes"][si] - base[si] == look + (64 if look else 0), (case.name, si)


def test_the_same_percentage_pays_for_less_under_the_packed_layout(answers):
    """The budget is a share of the RESIDENT posting bytes: 8 per posting in two columns, 4 packed.  12 % of the 200 003-doc
    segment pays for two sets of records and two sets of cells in two columns, for one and one packed."""
    got = answers["small12_packed"]["terms"][2]
    assert {t: got[t] for t in lc.SMALL12_PACKED_200} == lc.SMALL12_PACKED_200
    plain = answers["default_small_plain"]["terms"][2]     # 12 % as well
    assert plain[lc.ABSENT] == (BITS, 0, 50016) and plain[lc.UNDER256] == (CELLS, 8, 3136) and plain[lc.TILE300] == (NONE, 0, 0)


def test_a_negative_budget_gives_no_term_a_structure(answers):
    for name in ("default_none_plain", "default_none_packed"):
        assert all(v == (NONE, 0, 0) for seg in answers[name]["terms"] for v in seg.values()), name
        assert len(answers[name]["terms"][2]) == 11


def test_the_boundaries_of_the_rule(answers):
    t = lambda name: answers[name]["terms"][0]   # noqa: E731
    # kLookMinPostings: 63 postings never, 64 do (the corpus, default policy and budget)
    for seg in answers["default_default_plain"]["terms"]:
        assert seg[lc.P63] == (NONE, 0, 0) and seg[lc.P64][0] != NONE
    # "a posting per 256 docs or more": 256 postings in 65 536 docs are (records: 2049 blocks + 1 -> 16400 B), 255 are not (cells: 255
    # << 8 = 65280 <= 65536: shift 8, 256 cells, 1032 -> 1040 B); nor are 256 postings in 65 537 docs (256 * 256 = max_doc - 1)
    assert t("density_equal") == {20: (BITS, 0, 16400), 21: (CELLS, 8, 1040)}
    assert answers["default_default_plain"]["terms"][1][lc.UNDER256] == (CELLS, 8, 1040)
    assert answers["default_default_plain"]["terms"][1][lc.PER256] == (BITS, 0, 16400)
    # largest first, ties by the order the terms were added in (not by id): 600 postings, 4800 B, 400 % = 19200 B pay for one set
    # of records (16400 B) -- the first term's; 2800 B are left: no second set, but the cells of a later rule (300 << 7 <= 65536:
    # shift 7, 512 cells, 2064 B) fit
    assert t("tie_bits") == {31: (BITS, 0, 16400), 30: (NONE, 0, 0)}
    assert t("tie_bits_cells") == {31: (BITS, 0, 16400), 30: (CELLS, 7, 2064)}
    # a budget per upload group: 130 % of 24000 B pays for the first group's records, 130 % of 2400 B for none -- in ONE group
    # (26400 B, 34320 B of budget) both terms would be served
    assert t("two_groups") == {40: (BITS, 0, 16400), 41: (NONE, 0, 0)}
    assert t("one_group") == {40: (BITS, 0, 16400), 41: (BITS, 0, 16400)}


def test_a_packed_contexts_lookup_cells_stay_inside_a_super_window(answers):
    """64 postings in 2^27 docs: a posting per 2^21 docs.  Two columns: cells of 2^21 docs (64 cells, 264 -> 272 B of the 768 B
    budget).  Packed, the walk's search compares doc offsets inside a 2^20-doc super-window (maxscore.hip: dd = d & kPackDocMask),
    and a cell of 2^21 docs holds the offsets of two windows, which do not ascend: the seal stops at 2^20 docs per cell (128
    cells, 520 -> 528 B).  That is more than the default budget of the 256 packed bytes (384 B), so by default the term is searched
    in its tile-table cell (capped the same way: kPackMaxCellShift); with budget it gets the capped cells."""
    assert answers["huge_plain"]["terms"][0] == {50: (CELLS, 21, 272)}
    assert answers["huge_packed"]["terms"][0] == {50: (NONE, 0, 0)}
    assert answers["huge_packed_100000"]["terms"][0] == {50: (CELLS, 20, 528)}
