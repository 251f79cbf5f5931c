"""Multi-match queries without a GPU: the struct layout, the refusals (those that need a context against the stand-in runtime of
tests/mockhip), the arithmetic the kernel compiles (nrtgpu_multi_match_value == plan.h: multi_match_group / multi_match_fold /
multi_match_value) against the NumPy reference's per-doc rule, the reference itself against the oracle where a grouping
degenerates to a flat query the oracle offers, and the condition on the GPU tests' inputs that grouping is observable."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from nrtsearch_amd import _lib, build

from tests import _multi_match_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
SHAPES = {"cross_fields": _lib.NRTGPU_GROUPS_SUM_OF_MAX, "best_fields": _lib.NRTGPU_GROUPS_MAX_OF_SUM}
INV, UNS = _lib.NRTGPU_ERR_INVALID_ARG, _lib.NRTGPU_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _groups(shape, group_of, n_groups=None, mins=None, tie_breaker=0.0, group_occur=0, null=False):
    of = (C.c_int32 * max(len(group_of), 1))(*group_of)
    g = _lib.ClauseGroups()
    g.shape = shape if isinstance(shape, int) else SHAPES[shape]
    g.n_groups = (max(group_of) + 1) if n_groups is None else n_groups
    g.group_of_term = None if null else of
    g._keep = [of]
    if mins is not None:
        mm = (C.c_int32 * len(mins))(*mins)
        g.group_min_should_match = mm
        g._keep.append(mm)
    g.tie_breaker = tie_breaker
    g.group_occur = group_occur
    return g


def _value(lib, g, scores, matched, occur=None, msm=0, n_terms=None):
    sc = np.ascontiguousarray(scores, dtype=f32)
    oc = None if occur is None else np.ascontiguousarray(occur, dtype=np.int32)
    score, hit = C.c_float(0), C.c_int32(-1)
    rc = lib.nrtgpu_multi_match_value(C.byref(g), len(sc) if n_terms is None else n_terms, None if oc is None else oc.ctypes.data, int(msm),
                                      sc.ctypes.data, int(matched), C.byref(score), C.byref(hit))
    return rc, f32(score.value), hit.value


def test_struct_sizes():
    assert C.sizeof(_lib.ClauseGroups) == 32
    assert (_lib.NRTGPU_MAX_GROUPS, _lib.NRTGPU_GROUPS_SUM_OF_MAX, _lib.NRTGPU_GROUPS_MAX_OF_SUM) == (8, 0, 1)


def test_refusals_that_need_no_device(lib):
    one = [f32(1.0)] * 4
    bad = [
        (_groups(2, [0, 0, 1, 1]), {}, INV), (_groups(-1, [0, 0, 1, 1]), {}, INV),                       # shape
        (_groups(0, [0, 0, 1, 1], n_groups=0), {}, INV), (_groups(0, [0, 0, 1, 1], n_groups=9), {}, INV),   # n_groups
        (_groups(0, [0, 0, 2, 1], n_groups=2), {}, INV), (_groups(1, [0, -1, 1, 1], n_groups=2), {}, INV),  # a group index
        (_groups(0, [0, 0, 1, 1], group_occur=2), {}, INV), (_groups(0, [0, 0, 1, 1], group_occur=-1), {}, INV),
        (_groups(0, [0, 0, 2, 2], n_groups=3), {}, INV), (_groups(1, [1, 1, 1, 1], n_groups=2), {}, INV),   # an empty group
        (_groups(0, [0, 0, 1, 1], tie_breaker=1.5), {}, INV), (_groups(1, [0, 0, 1, 1], tie_breaker=-0.1), {}, INV),
        (_groups(0, [0, 0, 1, 1], tie_breaker=float("nan")), {}, INV), (_groups(1, [0, 0, 1, 1], tie_breaker=float("inf")), {}, INV),
        (_groups(1, [0, 0, 1, 1], mins=[0, -1]), {}, INV),                                                # a negative group minimum
        (_groups(0, [0, 0, 1, 1], null=True), {}, INV),                                                   # group_of_term == NULL
        (_groups(0, [0, 0, 1, 1]), {"occur": [0, 1, 0, 0]}, INV), (_groups(0, [0, 0, 1, 1]), {"occur": [1, 1, 1, 1]}, INV),   # SUM_OF_MAX with occur
        (_groups(1, [0, 0, 1, 1]), {"occur": [0, 2, 0, 0]}, INV),
        (_groups(1, [0, 0, 1, 1]), {"msm": 1}, INV),                                                      # MAX_OF_SUM with the query's minimum
        (_groups(1, [0, 0, 1, 1], group_occur=1), {}, INV),
        (_groups(0, [0, 0, 1, 1]), {"msm": -1}, INV),
        (_groups(0, [0, 0, 1, 1]), {"n_terms": 0}, INV),
        (_groups(1, [0, 0, 1, 1]), {"occur": [1, 0, 1, 1]}, UNS),                                         # a group that mixes MUST and SHOULD
        (_groups(1, [0] * 33), {"n_terms": 33, "scores": [f32(1.0)] * 33}, UNS),
    ]
    for g, kw, code in bad:
        rc, _, _ = _value(lib, g, kw.get("scores", one), 15, kw.get("occur"), kw.get("msm", 0), kw.get("n_terms"))
        assert rc == code, (g.shape, g.n_groups, g.tie_breaker, g.group_occur, kw, rc)
        assert lib.nrtgpu_last_error().decode() != ""
    g = _groups(0, [0, 0, 1, 1])
    sc = np.ones(4, f32)
    assert lib.nrtgpu_multi_match_value(None, 4, None, 0, sc.ctypes.data, 15, C.byref(C.c_float()), C.byref(C.c_int32())) == INV
    assert lib.nrtgpu_multi_match_value(C.byref(g), 4, None, 0, None, 15, C.byref(C.c_float()), C.byref(C.c_int32())) == INV
    assert lib.nrtgpu_multi_match_value(C.byref(g), 4, None, 0, sc.ctypes.data, 15, None, C.byref(C.c_int32())) == INV
    assert lib.nrtgpu_multi_match_value(C.byref(g), 4, None, 0, sc.ctypes.data, 15, C.byref(C.c_float()), None) == INV
    # the entries that need a context refuse a NULL one before anything else
    assert lib.nrtgpu_search_multi_match_batch(None, None, None, 0, None, None, 1, None) == INV
    assert lib.nrtgpu_multi_match_supported(None, None, 0, None, None) == INV
    # the widest accepted shapes
    assert _value(lib, _groups(0, list(range(8)) * 4, tie_breaker=1.0, group_occur=1), [f32(1.0)] * 32, 2**32 - 1)[0] == 0
    assert _value(lib, _groups(1, [0] * 32, mins=[33]), [f32(1.0)] * 32, 2**32 - 1) == (0, f32(0.0), 0)


def _score_pool(rng, n):
    """float32 scores whose float64 sums fall on and next to float32 rounding boundaries: values around 1 and 2 with the last
    mantissa bits set, half-ulp and quarter-ulp sized addends, and ordinary BM25-sized values."""
    kinds = rng.integers(0, 4, n)
    out = np.empty(n, f32)
    out[kinds == 0] = rng.uniform(0.05, 6.0, int((kinds == 0).sum()))
    out[kinds == 1] = (1.0 + rng.integers(0, 8, int((kinds == 1).sum())) * 2.0 ** -23)
    out[kinds == 2] = rng.integers(1, 8, int((kinds == 2).sum())) * 2.0 ** -25       # 1/4 .. 7/4 of an ulp of 1.0 .. 2.0
    out[kinds == 3] = (2.0 - rng.integers(1, 8, int((kinds == 3).sum())) * 2.0 ** -23)
    return out.astype(f32)


def test_value_is_the_reference_rule(lib):
    """Both shapes; 1..8 groups over 1..32 clauses; SHOULD with minima 0..n+1 and MUST; tie breakers 0, 1, 0.3 and the float below 1."""
    rng = np.random.default_rng(77)
    ties = [0.0, 1.0, 0.3, float(np.nextafter(f32(1), f32(0)))]
    n_docs, checked = 16, 0
    for shape in ("cross_fields", "best_fields"):
        for n_groups in range(1, 9):
            for n_clauses in sorted({n_groups, min(32, n_groups + 1), min(32, 2 * n_groups + 3), 32, int(rng.integers(n_groups, 33))}):
                group_of = list(range(n_groups)) + rng.integers(0, n_groups, n_clauses - n_groups).tolist()
                rng.shuffle(group_of)
                sizes = [group_of.count(g) for g in range(n_groups)]
                scores = _score_pool(rng, n_clauses * n_docs).reshape(n_clauses, n_docs)
                matched = rng.random((n_clauses, n_docs)) < rng.choice([0.3, 0.7, 1.0])
                if shape == "cross_fields":
                    variants = [("must", 0)] + [("should", m) for m in range(0, n_groups + 2)]
                else:
                    variants = [("must", 0), ("should", 0)] + [("should", tuple(int(rng.integers(0, s + 2)) for s in sizes)) for _ in range(3)]
                for operator, msm in variants:
                    for tb in ties:
                        exp_score, exp_hit = ref.combine(shape, group_of, scores, matched, operator, msm, tb)
                        best = shape == "best_fields"
                        g = _groups(shape, group_of, mins=list(msm) if isinstance(msm, tuple) else ([msm] * n_groups if best else None),
                                    tie_breaker=tb, group_occur=int(operator == "must" and not best))
                        occur = [int(operator == "must" and best)] * n_clauses
                        for d in range(n_docs):
                            bits = sum(1 << c for c in range(n_clauses) if matched[c, d])
                            rc, got, hit = _value(lib, g, scores[:, d], bits, occur, 0 if best else msm)
                            assert rc == 0 and hit == int(exp_hit[d]), (shape, group_of, operator, msm, tb, d)
                            if hit:
                                assert got.view(np.uint32) == exp_score[d].view(np.uint32), (shape, group_of, operator, msm, tb, d, got, exp_score[d])
                                checked += 1
    assert checked > 20_000


def _same(a, b, what):
    assert a[0].tolist() == b[0].tolist(), what
    assert a[1].view(np.uint32).tolist() == b[1].view(np.uint32).tolist(), what
    assert tuple(a[2:]) == tuple(b[2:]), (what, a[2:], b[2:])


def test_degenerate_groupings_are_the_flat_queries_of_the_oracle(oracle):
    """One clause per group, or one group: the reference must return what oracle.search_bm25 returns for the flat query (one field,
    the oracle's index being one)."""
    fields = ref.build_index()
    terms = [2, 5, 9, 13]
    flat = [(0, t, 1.0) for t in terms]
    singles = [[c] for c in flat]
    for slicing in (oracle.DEFAULT_SLICING, (2_000, 2)):
        kw = dict(slicing=slicing)
        for k, thr in ((10, 1000), (300, 100), (1024, 2**31 - 1)):
            okw = dict(total_hits_threshold=thr, slicing=slicing)
            rkw = dict(total_hits_threshold=thr, **kw)
            # SUM_OF_MAX, one clause per group: the boolean sum, with its minimum or as a conjunction
            _same(ref.search(oracle, fields, singles, "cross_fields", k, tie_breaker=0.7, **rkw), oracle.search_bm25(fields[0], terms, k, **okw), "sum")
            _same(ref.search(oracle, fields, singles, "cross_fields", k, msm=2, **rkw), oracle.search_bm25(fields[0], terms, k, min_should_match=2, **okw), "msm 2")
            _same(ref.search(oracle, fields, singles, "cross_fields", k, "must", **rkw), oracle.search_bm25(fields[0], terms, k, must=[True] * 4, **okw), "must")
            # MAX_OF_SUM, one clause per group: the flat DisjunctionMaxQuery
            for tb in (0.0, 0.3, 1.0):
                _same(ref.search(oracle, fields, singles, "best_fields", k, tie_breaker=tb, **rkw), oracle.search_bm25(fields[0], terms, k, dismax=tb, **okw), f"dismax {tb}")
                # one group: that group's flat query
                _same(ref.search(oracle, fields, [flat], "cross_fields", k, tie_breaker=tb, **rkw), oracle.search_bm25(fields[0], terms, k, dismax=tb, **okw), f"one dismax group {tb}")
            _same(ref.search(oracle, fields, [flat], "best_fields", k, tie_breaker=0.3, **rkw), oracle.search_bm25(fields[0], terms, k, **okw), "one boolean group")
            _same(ref.search(oracle, fields, [flat], "best_fields", k, msm=3, **rkw), oracle.search_bm25(fields[0], terms, k, min_should_match=3, **okw), "one group msm 3")
            _same(ref.search(oracle, fields, [flat], "best_fields", k, "must", **rkw), oracle.search_bm25(fields[0], terms, k, must=[True] * 4, **okw), "one must group")
    exp = oracle.search_bm25(fields[0], terms, 20, total_hits_threshold=0)
    after = (int(exp[0][6]), float(exp[1][6]))
    _same(ref.search(oracle, fields, singles, "cross_fields", 20, after=after, total_hits_threshold=0),
          oracle.search_bm25(fields[0], terms, 20, after=after, total_hits_threshold=0), "after")


def test_the_index_is_what_the_gpu_tests_need():
    fields = ref.build_index()
    assert [s.max_doc for s in fields[0].segments] == [13_400, 2_085, 1_024] and len(fields) == 3
    for corpus in fields:
        assert max(int(s.freqs.max()) for s in corpus.segments) > 12 and max(int(s.freqs.max()) for s in corpus.segments) <= 20
        assert ref.TERM_NOWHERE not in corpus.doc_freq
        assert len(corpus.segments[1].postings(ref.TERM_NOT_IN_LEAF[0])[0]) == 0 and len(corpus.segments[0].postings(ref.TERM_NOT_IN_LEAF[0])[0]) > 0
        dead = sum(int((~ref._bits(s.live_bits, s.max_doc)).sum()) for s in corpus.segments)
        assert 0.03 < dead / corpus.n_docs < 0.07
        assert 0.3 < corpus.doc_freq[1] / corpus.n_docs < 0.7 and corpus.doc_freq[12] / corpus.n_docs < 1 / 250
    assert max(int(s.norms.max()) for s in fields[0].segments) >= 128                 # escape codes by the norm byte as well
    assert fields[0].sum_total_term_freq != fields[1].sum_total_term_freq != fields[2].sum_total_term_freq


def test_grouping_is_observable_on_the_test_index(oracle):
    """A condition on the GPU tests' inputs: for the queries they run, the top-k score bits differ from those of the flat query
    over the same clauses -- a kernel that ignored the groups could not pass."""
    fields = ref.build_index()
    for shape, groups in (("cross_fields", ref.cross_fields_groups((2, 4, 7))), ("best_fields", ref.best_fields_groups((2, 4, 7)))):
        singles = [[c] for g in groups for c in g]
        grouped = ref.search(oracle, fields, groups, shape, 100, tie_breaker=0.3)
        flat = ref.search(oracle, fields, singles, shape, 100, tie_breaker=0.3)     # (pinned to the oracle's flat queries above)
        assert grouped[1].view(np.uint32).tolist() != flat[1].view(np.uint32).tolist(), shape
        assert grouped[0].tolist() != flat[0].tolist(), shape
        assert grouped[2] == flat[2]   # SHOULD groups without minima: the same docs are hits


@pytest.fixture(scope="module")
def mockhip(tmp_path_factory):
    if not (shutil.which("gcc") and os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h")):
        pytest.skip("gcc or the HIP headers are not here")
    build.build()
    out = str(tmp_path_factory.mktemp("mockhip") / "libmockhip.so")
    subprocess.run(["gcc", "-O1", "-w", "-fPIC", "-shared", "-I/opt/rocm/include", os.path.join(ROOT, "tests", "mockhip", "mockhip.c"), "-o", out],
                   check=True)
    return out


def test_host_side_against_the_stand_in_runtime(mockhip):
    e = dict(os.environ, LD_PRELOAD=mockhip)
    e.pop("NRTGPU_LIB_PATH", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mockhip", "multi_match_host.py")], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "done" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    got = dict(line.split(" ", 1) for line in r.stdout.strip().split("\n") if " " in line)
    I, U = str(INV), str(UNS)
    expect = {
        "cross_supported": "0", "best_supported": "0", "best_must_supported": "0", "escape_terms_supported": "0", "msm_above_n_groups": "0",
        "term_nowhere": "0", "search_cross": "0", "search_batch_of_4": "0", "search_batch_above_max_batch": I,
        "diagnostics_items": "0 1", "stats_counted": "1", "32_clauses": "0",
        "disjunction_max_set": I, "query_tie_breaker_set": I, "k_zero": I, "null_groups": I,
        "min_competitive_score": U, "mask_not_resident": U, "must_not_mask_not_resident": U, "five_fields": U, "33_clauses": U,
        "weights_span_too_many_binades": U, "mixed_group": U,
        "flag_no_fixed_point": U, "flag_no_fixed_point_search": U, "flag_packed_postings": U, "flag_packed_postings_search": U,
    }
    assert got == expect, {k: (got.get(k), v) for k, v in expect.items() if got.get(k) != v}
