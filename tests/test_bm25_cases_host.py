"""tests/_bm25_cases.py checked without a device: (1) every generated request is one nrtgpu_search_bm25_batch takes -- the planner's
refusal rules restated (refusal / taken_by: both messages), and nrtgpu_query_supported itself on every request, against tests/mockhip (the stand-in HIP
runtime of tests/test_planner_host.py) in a subprocess; (2) floors on what the sweep's layouts and the default fuzz rounds contain,
computed from the oracle alone, so that tests/test_bm25_edges_gpu.py and tests/test_fuzz_bm25_gpu.py cannot go hollow -- conditions
on the INPUTS, not on the library; (3) the Model's glue around oracle.search_bm25 -- the accept words, the per-slice counts, the set D
of the documented cursor / slice rule -- against plain per-doc Python loops over two small layouts."""
import collections
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle

from tests import _bm25_cases as bc
from tests import _final_score_cases as fc
from tests.test_fuzz_bm25_gpu import BASE
from tests.test_planner_host import ROOT, mockhip   # noqa: F401  (the fixture: the stand-in runtime, built once)

DEFAULT_ROUNDS = 8
INT_MAX = bc.INT_MAX


# ---- 1. every generated request is one the library takes ---------------------------------------------------------------------------------
def assert_drawn_legally(m: bc.Model, r: bc.Req, flags: int, name: str):
    assert bc.taken_by(r, flags), name
    assert all(t in bc.QUERY_TERMS + (bc.TERM_NOWHERE,) and b in bc.BOOSTS for t, b in r.clauses), name
    assert r.filter in (0,) + tuple(m.masks) and r.must_not in (0,) + tuple(m.masks), name
    assert r.dismax is None or (0.0 <= r.dismax <= 1.0 and r.min_should_match == 0 and not r.must), name
    assert not r.must or (len(r.must) == len(r.clauses) and r.min_should_match == 0 and list(r.must) == sorted(r.must, reverse=True)), name   # MUST first
    if r.min_competitive_score > 0.0:   # an exact count, no cursor: the header says what is counted, not which relation a bound from outside leaves
        assert r.threshold == INT_MAX and r.after is None and not r.second_accumulator, name
    if r.after is not None:
        assert 0 <= r.after[0] < m.n_docs and r.after[1] == float(np.float32(r.after[1])), name


@pytest.mark.parametrize("layout", bc.LAYOUTS, ids=[str(l) for l in bc.LAYOUTS])
def test_every_sweep_request_is_drawn_legally(layout):
    m, reqs, _ = bc.sweep_case(layout)
    assert 30 <= len(reqs) <= 128
    for i, r in enumerate(reqs):
        assert_drawn_legally(m, r, 0, f"layout {layout}, request {i}: {bc.describe(r)}")
    scan = [r for r in reqs if bc.taken_by(r, bc.NO_PRUNE)]
    assert len(scan) >= 30 and all(not r.second_accumulator for r in scan) and any(r.second_accumulator for r in reqs)


@pytest.mark.parametrize("round_", range(DEFAULT_ROUNDS))
def test_every_fuzz_request_is_drawn_legally(round_):
    m, knobs, batches = bc.fuzz_round(BASE, round_)
    assert 1 <= len(m.sizes) <= 12 and m.n_docs <= bc.FUZZ_MAX_DOCS and set(m.sizes) <= set(bc.FUZZ_SIZES)
    assert m.slicing in bc.FUZZ_SLICINGS and m.target_items in bc.FUZZ_TARGET_ITEMS and knobs.flags in bc.FUZZ_FLAGS and knobs.budget_pct in bc.FUZZ_BUDGETS
    assert len(batches) == 3
    for bi, reqs in enumerate(batches):
        assert 8 <= len(reqs) <= 32
        for i, r in enumerate(reqs):
            assert_drawn_legally(m, r, knobs.flags, f"round {round_}, batch {bi}, index {i}: {bc.describe(r)}")


def test_the_library_takes_every_generated_request(mockhip):   # noqa: F811
    """nrtgpu_query_supported on every request of the sweep (default flags, NO_PRUNE, NO_FIXED_POINT) and of the default fuzz rounds;
    what a context refuses -- the second-accumulator shapes without the MaxScore route, the clause-counting shapes without the
    fixed-point sums -- it refuses with that message of the planner's (tests/mockhip/bm25_cases_supported.py)."""
    # (the stand-in first, so that its HIP symbols win; whatever the environment already preloads stays behind it)
    e = dict(os.environ, LD_PRELOAD=":".join(x for x in (mockhip, os.environ.get("LD_PRELOAD", "")) if x))
    e.pop("NRTGPU_LIB_PATH", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mockhip", "bm25_cases_supported.py"), str(BASE), str(DEFAULT_ROUNDS)], env=e,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "done" in r.stdout, r.stderr[-2000:]
    got = {line.split(" ", 1)[0]: line.split(" ", 1)[1] for line in r.stdout.split("\n") if " " in line}
    names = [f"layout_{layout}_{flags}" for layout in bc.LAYOUTS for flags in (0, bc.NO_PRUNE, bc.NO_FIXED_POINT)] + [f"round_{i}" for i in range(DEFAULT_ROUNDS)]
    assert all(got[n].startswith("ok ") for n in names), {n: got.get(n) for n in names if not got.get(n, "").startswith("ok ")}
    for layout in bc.LAYOUTS:   # ... and the refusals were there to be checked: by either message
        m, reqs, _ = bc.sweep_case(layout)
        assert int(got[f"layout_{layout}_{bc.NO_PRUNE}"].split()[2]) >= 5 and int(got[f"layout_{layout}_0"].split()[2]) == 0
        assert sum(1 for r in reqs if bc.refusal(r, bc.NO_FIXED_POINT) == bc.REFUSED_FIXED_POINT) >= 5
        assert sum(1 for r in reqs if bc.refusal(r, bc.NO_FIXED_POINT) == bc.REFUSED_SECOND_ACCUMULATOR) >= 5


# ---- 2. what the sweep's layouts and the default rounds contain --------------------------------------------------------------------------
def test_the_sweep_layouts():
    assert bc.LAYOUTS == fc.SINGLE_LEAF + (65_535, 65_536, 65_537) + fc.MULTI_LEAF and bc.SLICE_LAYOUTS == ("eight_slices", "nine_slices", "sixteen_slices")
    for name, n in (("eight_slices", 8), ("nine_slices", 9), ("sixteen_slices", 16)):
        spec = bc.layout_of(name)
        assert spec["target_items"] == 1 and len(bc.sweep_case(name)[0].slices) == n
    for layout in bc.LAYOUTS:
        assert tuple(bc.layout_of(layout)["leaf_docs"]) == tuple(fc.layout_of(layout)["leaf_docs"])


@pytest.mark.parametrize("layout", bc.LAYOUTS, ids=[str(l) for l in bc.LAYOUTS])
def test_a_sweep_layout_reaches_what_it_is_for(layout):
    m, reqs, marks = bc.sweep_case(layout)
    spec = bc.layout_of(layout)
    assert tuple(m.sizes) == tuple(spec["leaf_docs"])
    assert [seg.live_bits is None for seg in m.segments] == [si in spec["live_none"] for si in range(len(m.sizes))]
    edge = bc.edge_flags(m.sizes)
    # the edge docs hold the edge term and nothing else does; the copy without them deletes exactly them
    for si, seg in enumerate(m.segments):
        d = seg.postings(bc.EDGE_TERM)[0].tolist()
        assert d == ([] if (si, bc.EDGE_TERM) in spec["without"] else bc.EDGE_DOCS(seg.max_doc))
        assert all(m.masks[bc.EDGE][si][x >> 6] >> np.uint64(x & 63) & np.uint64(1) for x in bc.EDGE_DOCS(seg.max_doc))
    gone = m.edges_deleted()
    if m.n_docs < 2000:
        was = np.concatenate([[seg.live_bits is None or _bit(seg.live_bits, x) for x in range(seg.max_doc)] for seg in m.segments])
        now = np.concatenate([[_bit(seg.live_bits, x) for x in range(seg.max_doc)] for seg in gone.segments])
        assert was[edge].all() and (now == (was & ~edge)).all()
    # an edge doc heads a page, and the EDGE mask decides one
    head = m.expected(reqs[marks["edge"]])
    assert edge[int(head[0][0])], (layout, head[0][:4])
    changed = 0
    for mark in ("edge_filter", "edge_must_not"):
        r = reqs[marks[mark]]
        with_, without = m.expected(r), m.expected(dataclasses.replace(r, filter=0, must_not=0))
        changed += int(with_[0].tolist() != without[0].tolist() or with_[2] != without[2])
    assert changed >= 1 and (changed == 2 or m.n_docs == 1), (layout, changed)
    if m.n_docs > 1:
        for r in bc.edges_deleted_requests(m):   # deleting the edge docs changes every page of the copy
            assert gone.expected(r)[0].tolist() != m.expected(r)[0].tolist() and not edge[gone.expected(r)[0]].any(), (layout, bc.describe(r))
    # every k, every shape, thresholds on both sides, cursors
    seen = collections.Counter()
    hits = m.expected(bc.plain(bc.T3, k=1, threshold=INT_MAX))[2]
    for r in reqs:
        seen["k", r.k] += 1
        seen["clauses", len(r.clauses)] += 1
        seen["msm"] += int(r.min_should_match >= 2)
        seen["tie", r.dismax] += int(r.dismax is not None)
        seen["must"] += int(r.mixed_must)
        seen["conjunction"] += int(bool(r.must) and all(r.must))
        seen["filter", r.filter] += 1
        seen["must_not", r.must_not] += 1
        seen["below"] += int(r.threshold < hits)
        seen["above"] += int(hits < r.threshold < INT_MAX)
        seen["complete"] += int(r.threshold == INT_MAX)
        seen["cursor"] += int(r.after is not None)
        seen["bound"] += int(r.min_competitive_score > 0.0)
        seen["gte", m.expected(r)[3]] += 1
        seen["empty"] += int(m.expected(r)[2] == 0)
    assert all(seen["k", k] >= 2 for k in (1, 64, 1000, 1024)) and all(seen["clauses", n] >= 1 for n in (1, 3, 8, 9, 10)), dict(seen)
    assert seen["msm"] >= 3 and seen["tie", 0.0] >= 2 and seen["tie", 0.3] >= 3 and seen["must"] >= 3 and seen["conjunction"] >= 1, dict(seen)
    assert all(seen["filter", i] >= 2 for i in (bc.EDGE, bc.DENSE)) and seen["filter", bc.SPARSE] >= 1 and seen["must_not", bc.EDGE] >= 2 and seen["must_not", bc.SPARSE] >= 1
    assert seen["above"] >= 5 and seen["complete"] >= 5 and seen["empty"] >= 1 and seen["gte", False] >= 10, dict(seen)
    if m.n_docs >= 63:
        assert seen["below"] >= 10 and seen["bound"] == 1 and "run" in marks, dict(seen)
        r = reqs[marks["run"]]   # the cursor lies inside a run of equal scores: the page begins with the cursor's own score
        page = m.expected(r)
        assert len(page[0]) > 0 and float(page[1][0]) == r.after[1] and int(page[0][0]) > r.after[0], (layout, bc.describe(r))
    if m.n_docs >= 1023:
        assert seen["gte", True] >= 3 and seen["cursor"] >= 5, dict(seen)   # both relations occur
        # the threshold on the largest slice's exact count, and one below it: the relation turns there
        at, below_ = reqs[marks["at_count"]], reqs[marks["below_count"]]
        assert at.threshold == max(m.slice_counts(at)) == below_.threshold + 1 and at.threshold > at.k and at.shaped, (layout, bc.describe(at))
        assert not m.expected(at)[3] and m.expected(below_)[3], layout
    if layout in bc.SLICE_LAYOUTS:
        for mark in ("in_d", "in_d_shaped"):
            r = reqs[marks[mark]]
            assert m.in_d(r) and m.expected(r)[3] and not m.oracle(r)[3] and r.shaped == (mark == "in_d_shaped"), (layout, mark)
        r = reqs[marks["not_in_d"]]
        assert r.after is not None and not m.in_d(r) and m.expected(r)[2:] == m.oracle(r)[2:] and m.oracle(r)[3], layout
    if layout == "gaps":
        assert all(len(m.segments[si].postings(t)[0]) == 0 for si in bc.GAPS_ABSENT for t in bc.QUERY_TERMS)
        assert all(len(m.segments[si].postings(bc.FILLER_TERM)[0]) > 0 for si in bc.GAPS_ABSENT)
    if layout == "many_small":
        assert len(m.sizes) == 40


@pytest.fixture(scope="module")
def census():
    c = collections.Counter()
    for round_ in range(DEFAULT_ROUNDS):
        m, knobs, batches = bc.fuzz_round(BASE, round_)
        c["slices", m.slicing, min(len(m.slices), 9) if len(m.slices) >= 9 else min(len(m.slices), 2)] += 1
        c["flags", knobs.flags] += 1
        c["packed", knobs.packed] += 1
        c["budget", knobs.budget_pct] += 1
        c["target_items", m.target_items] += 1
        c["window", any(n > bc.MS_WIN_DOCS for n in m.sizes)] += 1
        c["pair", m.slicing, knobs.budget_pct] += 1
        maxscore_round = not knobs.flags & (bc.NO_PRUNE | bc.NO_FIXED_POINT)
        c["nine_slices_some_of_two_leaves", m.slicing] += int(len(m.slices) >= 9 and any(len(g) > 1 for g in m.slices))
        c["maxscore_round_nine_slices"] += int(maxscore_round and len(m.slices) >= 9)
        c["scan_round_nine_slices"] += int(bool(knobs.flags & bc.NO_PRUNE) and len(m.slices) >= 9)
        for reqs in batches:
            for r in reqs:
                exp = m.expected(r)
                c["requests"] += 1
                c["gte", exp[3]] += 1
                c["in_d"] += int(m.in_d(r))
                c["cursor_many_slices"] += int(r.after is not None and len(m.slices) > 1)
                c["cursor_outside_d"] += int(r.after is not None and len(m.slices) > 1 and not m.in_d(r))
                c["scan_shaped"] += int(bool(knobs.flags & bc.NO_PRUNE) and len(r.clauses) <= 8 and r.shaped)
                c["second_accumulator"] += int(r.second_accumulator)
                c["bound"] += int(r.min_competitive_score > 0.0)
                c["empty"] += int(exp[2] == 0)
                c["count_mode_many_slices"] += int(len(m.slices) > 1 and bc.on_maxscore(r, knobs.flags) and r.shaped)
                c["count_mode_nine_slices"] += int(len(m.slices) >= 9 and bc.on_maxscore(r, knobs.flags) and r.shaped)
                c["maxscore_nine_slices"] += int(len(m.slices) >= 9 and bc.on_maxscore(r, knobs.flags) and m.matches_something(r))
                c["in_d_maxscore"] += int(m.in_d(r) and bc.on_maxscore(r, knobs.flags))
                c["in_d_scan"] += int(m.in_d(r) and not bc.on_maxscore(r, knobs.flags))
    return c


def test_the_default_rounds_hold_the_floors(census):
    c = census
    assert c["requests"] >= 300 and c["gte", True] >= 30 and c["gte", False] >= 30, dict(c)
    for slicing in bc.FUZZ_SLICINGS[1:]:   # every slicing but the default cuts at least one round's leaves into two slices or more
        assert c["slices", slicing, 2] + c["slices", slicing, 9] >= 1, dict(c)
    # ... and into nine or more (the item cut), every slicing that can.  (20 000, 2) cannot: of at most 12 leaves and 150 000 docs, the
    # leaves above 20 000 docs -- a slice each, 40 000 or 65 537 docs long -- are three at most, and the nine others, two to a slice,
    # make five slices: eight together (two large leaves and ten others: seven).  The default slicing gives three at most.
    for slicing in ((2000, 2), (500, 1)):
        assert c["slices", slicing, 9] >= 1, dict(c)
    assert c["nine_slices_some_of_two_leaves", (2000, 2)] >= 1, dict(c)   # (... where a slice is more than one part of the item)
    # both routes over nine slices and more, MaxScore's count mode among them
    assert c["maxscore_round_nine_slices"] >= 1 and c["scan_round_nine_slices"] >= 1 and c["maxscore_nine_slices"] >= 20 and c["count_mode_nine_slices"] >= 10, dict(c)
    # slicing and lookup budget do not move together: the default rounds pair every slicing with two budgets
    assert all(sum(1 for b in bc.FUZZ_BUDGETS if c["pair", slicing, b]) == 2 for slicing in bc.FUZZ_SLICINGS), dict(c)
    assert all(c["flags", f] >= 1 for f in bc.FUZZ_FLAGS) and c["packed", True] >= 1 and c["packed", False] >= 1, dict(c)
    assert all(c["budget", b] >= 1 for b in bc.FUZZ_BUDGETS) and all(c["target_items", t] >= 1 for t in bc.FUZZ_TARGET_ITEMS) and c["window", True] >= 2, dict(c)
    assert c["scan_shaped"] >= 30 and c["second_accumulator"] >= 10 and c["bound"] >= 3 and c["empty"] >= 3 and c["count_mode_many_slices"] >= 10, dict(c)
    # D rests on the library's own rule: it stays the exception, and is still there, with cursors over several slices outside it
    # -- on either route
    assert 1 <= c["in_d_maxscore"] and 1 <= c["in_d_scan"] and 10 * c["in_d"] <= c["requests"] and c["cursor_outside_d"] >= 5, dict(c)


# ---- 3. the glue against plain loops -----------------------------------------------------------------------------------------------------
def _bit(words, d: int) -> bool:
    return bool((int(words[d >> 6]) >> (d & 63)) & 1)


def loop_hits(m: bc.Model, r: bc.Req):
    """[(leaf, local doc)] of the request's hits, one doc at a time: liveDocs, FILTER, MUST_NOT, the clauses' postings as sets"""
    out = []
    for si, seg in enumerate(m.segments):
        sets = [set(seg.postings(t)[0].tolist()) for t in r.terms]
        for d in range(seg.max_doc):
            if seg.live_bits is not None and not _bit(seg.live_bits, d):
                continue
            if (r.filter and not _bit(m.masks[r.filter][si], d)) or (r.must_not and _bit(m.masks[r.must_not][si], d)):
                continue
            has = [d in s for s in sets]
            if any(r.must):
                hit = all(h for h, must in zip(has, r.must) if must)
            else:
                hit = sum(has) >= max(1, r.min_should_match)            # (a clause given twice counts twice)
            if hit:
                out.append((si, d))
    return out


@pytest.mark.parametrize("sizes, slicing", [((1, 64, 65), (60, 1)), ((63, 65, 1023, 64), (100, 2))])
def test_the_model_equals_plain_loops(sizes, slicing):
    corpus = bc.build_index(sizes, 171, deletes=0.1)
    m = bc.Model(corpus, bc.sweep_masks(sizes, 172), slicing)
    assert len(m.slices) == 3
    slice_of = {si: sl for sl, g in enumerate(m.slices) for si in g}
    bases = [seg.doc_base for seg in m.segments]
    shapes = [bc.plain((2, 5)), bc.plain(bc.T3), bc.plain(bc.T8, min_should_match=2), bc.plain((1, 3), filter=bc.DENSE), bc.plain((1, 3), must_not=bc.EDGE),
              bc.plain(bc.T3, filter=bc.EDGE), bc.plain((2, 3, 2), min_should_match=3, must_not=bc.SPARSE), bc.with_must((1, 2, 3), (False, True, False)),
              bc.with_must((2, 3), (True, True), filter=bc.DENSE), bc.plain((1, 2), dismax=0.3, must_not=bc.SPARSE), bc.plain((bc.TERM_NOWHERE, 4))]
    in_d = outside = 0
    for shape in shapes:
        hits = loop_hits(m, shape)
        # the accept words, bit by bit
        acc = m.accept(shape)
        assert (acc is None) == (not shape.filter and not shape.must_not)   # (None: the leaves' own liveDocs)
        for si, seg in enumerate(m.segments if acc is not None else ()):
            assert len(acc[si]) == (seg.max_doc + 63) // 64 and not any(_bit(acc[si], d) for d in range(seg.max_doc, 64 * len(acc[si])))
            for d in range(seg.max_doc):
                want = (seg.live_bits is None or _bit(seg.live_bits, d)) and (not shape.filter or _bit(m.masks[shape.filter][si], d)) and \
                       not (shape.must_not and _bit(m.masks[shape.must_not][si], d))
                assert _bit(acc[si], d) == want, (bc.describe(shape), si, d)
        # the per-slice counts, and the exact total
        counts = [sum(1 for si, _ in hits if slice_of[si] == sl) for sl in range(len(m.slices))]
        assert m.slice_counts(shape) == counts and m.expected(dataclasses.replace(shape, threshold=INT_MAX))[2] == len(hits), (bc.describe(shape), counts)
        # D: cursors all along the ranked list (one collector over all leaves ranks it; the loop says which slice a hit is in)
        docs, scores, total, _ = oracle.search_bm25(m.corpus, shape.terms, 1024, boosts=[b for _, b in shape.clauses], total_hits_threshold=INT_MAX,
                                                    accept=acc, min_should_match=shape.min_should_match, dismax=shape.dismax,
                                                    must=list(shape.must) if shape.must else None, slicing=None)
        assert total == len(hits) < 1024 and sorted(docs.tolist()) == sorted(bases[si] + d for si, d in hits), bc.describe(shape)
        leaf_of = np.searchsorted(np.array(bases), docs, side="right") - 1
        for k, thr in ((5, 3), (20, 0), (3, 40), (10, 5), (8, 0)):
            for at in range(0, len(docs), 5):
                r = dataclasses.replace(shape, k=k, threshold=thr, after=(int(docs[at]), float(scores[at])))
                behind = [sum(1 for j in range(at + 1, len(docs)) if slice_of[int(leaf_of[j])] == sl) for sl in range(len(m.slices))]
                got = m.oracle(r)
                assert got[0].tolist() == docs[at + 1: at + 1 + k].tolist() and got[2] == len(hits), (bc.describe(r), behind)
                # the reference's rule, where it is beyond doubt: a slice whose queue overflows above the threshold is a lower bound;
                # no slice with a full queue is none
                if any(b > k and c > thr for b, c in zip(behind, counts)):
                    assert got[3], (bc.describe(r), behind, counts)
                if all(b < k for b in behind):
                    assert not got[3], (bc.describe(r), behind, counts)
                want = sum(behind) >= k and not got[3] and max(counts) > max(thr, k)
                assert m.in_d(r) == want and m.expected(r)[3] == (got[3] or want), (bc.describe(r), behind, counts)
                in_d += int(want)
                outside += int(not want)
    assert in_d >= 10 and outside >= 10, (in_d, outside)
