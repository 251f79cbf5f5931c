"""tests/_final_score_cases.py checked without a device: (1) every generated request is one the four final-score routes take -- the
limits, and the fixed-point scale of every clause from the library's own pure function; (2) floors on what the default fuzz rounds
and the sweep's layouts contain, computed from the references alone, so that tests/test_fuzz_final_score_gpu.py and
tests/test_final_score_edges_gpu.py cannot go hollow -- conditions on the INPUTS, not on the library; (3) the Model's glue around
the four references against plain per-doc Python loops over one tiny index (leaves of 1, 64 and 65 docs): a wrong doc base, mask
word or accept set in the Model must not hide the same error in a kernel."""
import collections
import ctypes as C
import dataclasses

import numpy as np
import pytest

from nrtsearch_amd import _lib, api
from oracle import oracle

from tests import _final_score_cases as fc
from tests import _multi_match_ref as mm_ref
from tests.test_fuzz_final_score_gpu import BASE
from tests.test_text_knn_host import _clauses, _query

f32 = np.float32
DEFAULT_ROUNDS = 8
TEXT_MIN_ITEM_COST, TILE_COST = 1 << 17, 48   # planner.cpp: build_plan's min_item_cost, kTileCostPostings


# ---- 1. every generated request is one the route takes --------------------------------------------------------------------------------
class Scales:
    """nrtgpu_fixed_point_scale of a model's clauses, once per (field, term, boost)"""

    def __init__(self, m: fc.Model):
        self.m, self.memo = m, {}
        self.max_norm = [max(int(np.asarray(s.norms).max()) for s in corpus.segments) for corpus in m.fields]

    def of(self, clause):
        """the clause's scale, or None: the term is in no doc (weight 0, no posting)"""
        if clause not in self.memo:
            field, term, boost = clause
            corpus = self.m.fields[field]
            self.memo[clause] = None
            if corpus.doc_freq.get(term, 0) > 0:
                weights, cache = oracle.bm25_query_stats(corpus, [term], [boost])
                e = C.c_int32(0)
                assert weights[0] > 0
                assert _lib.load().nrtgpu_fixed_point_scale(C.c_float(float(weights[0])), cache.ctypes.data, self.max_norm[field], C.byref(e)) == 1, clause
                self.memo[clause] = e.value
        return self.memo[clause]


def assert_taken(m: fc.Model, scales: Scales, r: fc.Req, name: str):
    assert r.entry in fc.ENTRIES and 1 <= r.k <= 1024 and r.threshold >= 0, name
    assert 1 <= len(r.clauses) <= 32 and 1 <= len(r.groups) <= 8 and all(len(g) >= 1 for g in r.groups), name
    assert len({c[0] for c in r.clauses}) <= 4 and all(0 <= c[0] < len(m.fields) and c[2] > 0 for c in r.clauses), name
    assert len(r.functions) <= 8 and all(w > 0 and (i == 0 or i in m.masks) for i, w in r.functions), name
    assert all(i in m.masks for i in r.filter + r.must_not) and len(r.filter) <= 1 and len(r.must_not) <= 1, name
    assert (r.score_mode, r.boost_mode) in fc.MODE_PAIRS and r.min_score >= 0 and 0.0 <= r.tie_breaker <= 1.0, name
    if r.grouped:
        assert r.shape in ("cross_fields", "best_fields") and r.operator in ("should", "must") and (r.operator == "should" or r.msm == 0), name
        assert isinstance(r.msm, int) or (r.shape == "best_fields" and len(r.msm) == len(r.groups)), name
    else:   # a SHOULD disjunction over field 0: no MUST, no minimum above 1
        assert len(r.groups) == 1 and r.operator == "should" and r.msm == 0 and all(c[0] == 0 for c in r.clauses), name
    if not r.scored:
        assert not r.functions and r.min_score == 0.0 and not r.min_excluded, name
    e = [s for s in (scales.of(c) for c in r.clauses) if s is not None]
    assert not e or max(e) - min(e) <= 15, (name, e)
    if r.entry == "text_knn":
        assert len(r.lists) <= 8, name
        for docs, scores, boost in r.lists:
            assert len(docs) == len(scores) <= 1024 and len(set(docs)) == len(docs) and boost > 0, name
            assert all(0 <= d < m.n_docs for d in docs) and all(s > 0 for s in scores), name
        q = _query((1.0,), masks=r.nested)
        assert _lib.load().nrtgpu_text_knn_exact(C.byref(q), C.byref(_clauses(list(r.lists), nested=int(r.nested))), max(e) if e else 0) == 1, name
    else:
        assert not r.lists, name
    if r.after is not None:
        assert 0 <= r.after[0] < m.n_docs and r.after[1] == float(f32(r.after[1])), name


@pytest.mark.parametrize("layout", fc.LAYOUTS, ids=[str(l) for l in fc.LAYOUTS])
def test_every_sweep_request_is_one_the_route_takes(layout):
    m, reqs, _ = fc.sweep_case(layout)
    scales = Scales(m)
    for entry in fc.ENTRIES:
        for i, r in enumerate(reqs[entry]):
            assert r.entry == entry
            assert_taken(m, scales, r, f"layout {layout}, {entry}[{i}]: {fc.describe(r)}")
    # checked here: over 15 860 docs the terms' scales span 4 and the weight lies at most 3 binades above the grain of the longest doc
    e = [s for s in (scales.of(c) for c in list(scales.memo)) if s is not None]
    assert max(e) - min(e) <= 8, e


@pytest.mark.parametrize("round_", range(DEFAULT_ROUNDS))
def test_every_fuzz_request_is_one_the_route_takes(round_):
    m, batches = fc.fuzz_round(BASE, round_)
    assert 1 <= len(m.sizes) <= 12 and m.n_docs <= fc.FUZZ_MAX_DOCS and 1 <= len(m.fields) <= 4 and set(m.sizes) <= set(fc.FUZZ_SIZES)
    assert m.slicing in fc.FUZZ_SLICINGS and m.target_items in (0, 4096)
    assert [e for e, _ in batches] == [e for e in fc.ENTRIES for _ in range(2)]
    scales = Scales(m)
    for bi, (entry, reqs) in enumerate(batches):
        assert 1 <= len(reqs) <= 16
        for i, r in enumerate(reqs):
            assert r.entry == entry
            assert_taken(m, scales, r, f"round {round_}, batch {bi}, index {i}: {fc.describe(r)}")


# ---- 2. what the default rounds and the sweep's layouts contain ----------------------------------------------------------------------------
def items_at_most(m: fc.Model, r: fc.Req) -> int:
    """an upper bound of the items a query is cut into (tests/test_column_cases_host.text_items_at_most: its cost over the least
    cost of an item, rounded; host_math.h).  A query of one item by cost and at most kSliceSlots slices is ONE item (planner.cpp:
    the only close is the last part's; a remainder of the rounding joins the item before it); otherwise one more for the
    remainder, and one for every kSliceSlots slices beyond the first eight."""
    cost = sum(m.fields[f].doc_freq.get(t, 0) for f, t, _ in r.clauses) + TILE_COST * sum((n + fc.TILE_DOCS - 1) // fc.TILE_DOCS for n in m.sizes)
    by_cost, n_slices = max(1, (cost + TEXT_MIN_ITEM_COST // 2) // TEXT_MIN_ITEM_COST), len(m.slices)
    return by_cost + int(by_cost > 1 or n_slices > fc.SLICE_SLOTS) + (n_slices - 1) // fc.SLICE_SLOTS


def in_a_run(m: fc.Model, r: fc.Req) -> bool:
    """the cursor lies inside a run of equal final scores: the page begins with the cursor's own score"""
    exp = m.expected(r)
    return r.after is not None and len(exp[0]) > 0 and int(exp[1][:1].view(np.uint32)[0]) == int(np.array([r.after[1]], f32).view(np.uint32)[0])


def kept_after_omitted(m: fc.Model, r: fc.Req) -> bool:
    kept = m.kept_leaves(r)
    return bool(kept) and len(kept) < kept[-1] + 1


def take_census(base: int) -> collections.Counter:
    c = collections.Counter()
    for round_ in range(DEFAULT_ROUNDS):
        m, batches = fc.fuzz_round(base, round_)
        for entry, reqs in batches:
            for r in reqs:
                exp = m.expected(r)
                kept = m.kept_leaves(r)
                c["requests"] += 1
                c["buffer_overflows"] += int(r.after is None and r.k >= 1000 and exp[2] > fc.CAND_CAP[entry] * items_at_most(m, r))
                c["cursor_in_a_run"] += int(in_a_run(m, r))
                c["empty_hit_set"] += int(exp[2] == 0)
                if r.min_score > 0 or r.min_excluded:
                    without = m.expected(dataclasses.replace(r, min_score=0.0, min_excluded=False, after=None))[2]
                    c["min_score_removes_some"] += int(0 < m.expected(dataclasses.replace(r, after=None))[2] < without)
                c["more_than_8_slices"] += int(len({si for si, g in enumerate(m.slices) if set(g) & set(kept)}) > fc.SLICE_SLOTS)
                c["item_of_4_leaves"] += int(len(kept) >= 4 * items_at_most(m, r))   # (the pigeonhole, whatever the cut)
                c["four_fields"] += int(len({f for f, _, _ in r.clauses}) == 4)
                c["24_clauses"] += int(len(r.clauses) >= 24)
                c["eight_functions"] += int(len(r.functions) == 8)
                c["kept_after_omitted"] += int(kept_after_omitted(m, r))
                if entry == "text_knn":
                    for kind, n in m.kinds(r).items():
                        c["knn_" + kind] += int(n > 0)
    return c


@pytest.fixture(scope="module")
def census():
    return take_census(BASE)


@pytest.mark.parametrize("what", ["buffer_overflows", "cursor_in_a_run", "empty_hit_set", "min_score_removes_some", "more_than_8_slices", "item_of_4_leaves",
                                  "four_fields", "24_clauses", "eight_functions", "kept_after_omitted", "knn_text", "knn_no_text", "knn_outside",
                                  "knn_deleted"])
def test_the_default_rounds_hold_at_least_three_of(census, what):
    assert census[what] >= 3, dict(census)


def test_the_default_rounds_hold_300_requests(census):
    assert census["requests"] >= 300, dict(census)


def test_the_sweep_layouts():
    assert fc.SINGLE_LEAF == (1, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193, 12287, 12288, 12289)
    assert fc.LAYOUTS == fc.SINGLE_LEAF + ("many_small", "tiny_first", "tiny_last", "eight_slices", "nine_slices", "sixteen_slices", "gaps", "mixed_live")
    assert fc.EDGE_DOCS(5000) == [0, 62, 63, 64, 65, 1022, 1023, 1024, 1025, 4998, 4999] and fc.EDGE_DOCS(64) == [0, 62, 63]
    for name, n in (("eight_slices", 8), ("nine_slices", 9), ("sixteen_slices", 16)):
        spec = fc.layout_of(name)
        assert set(spec["leaf_docs"]) == {1025} and spec["target_items"] == 0
        fields = fc.build_fields(spec["leaf_docs"], 1, 1)
        assert len(oracle.corpus_slices(fields[0], spec["slicing"])) == n
        # ... and the library cuts the same slices (nrtgpu_slices: what the context does with set_slicing's numbers)
        assert len(api.slices(spec["leaf_docs"], slice_max_docs=spec["slicing"][0], slice_max_segments=spec["slicing"][1])[0]) == n
    assert fc.layout_of("many_small")["leaf_docs"] == (1, 63, 64, 65, 700, 1023, 1024, 1025) * 5
    spec = fc.layout_of("mixed_live")
    assert spec["leaf_docs"] == (1025, 64, 4097, 1024) and spec["live_none"] == (0, 2)


@pytest.mark.parametrize("layout", fc.LAYOUTS, ids=[str(l) for l in fc.LAYOUTS])
def test_a_sweep_layout_reaches_what_it_is_for(layout):
    m, reqs, marks = fc.sweep_case(layout)
    spec = fc.layout_of(layout)
    assert tuple(m.sizes) == spec["leaf_docs"] and len(m.fields) == 4
    assert [seg.live_bits is None for seg in m.segments] == [si in spec["live_none"] for si in range(len(m.sizes))]
    edge_docs = {seg.doc_base + d for seg in m.segments for d in fc.EDGE_DOCS(seg.max_doc)}
    live_edge = {seg.doc_base + d for si, seg in enumerate(m.segments) for d in fc.EDGE_DOCS(seg.max_doc) if m.live(si)[d]}
    cursors = 0
    for entry in fc.ENTRIES:
        assert len(reqs[entry]) >= 8, (layout, entry)
        cursors += sum(int(r.after is not None) for r in reqs[entry])
        ks = {r.k for r in reqs[entry]}
        assert ks >= {1, 10, 1024}
        if entry != "multi_match":   # the edge function (text_knn: the edge list): an edge doc heads the page
            r = reqs[entry][marks[entry]["edge"]]
            assert r.after is None and (r.functions == ((fc.EDGE, 8.0),) or entry == "text_knn")
            exp = m.expected(r)
            assert len(live_edge) < 2 or int(exp[0][0]) in edge_docs, (layout, entry, exp[0][:4])
        if entry.startswith("function_score") and m.n_docs >= 64:
            assert in_a_run(m, reqs[entry][marks[entry]["run"]]), (layout, entry)
    assert cursors >= 8, (layout, cursors)
    seen = collections.Counter()
    for entry in fc.ENTRIES:
        for r in reqs[entry]:
            seen["modes", r.score_mode, r.boost_mode] += int(bool(r.functions))
            seen["eight"] += int(len(r.functions) == 8)
            seen["limits", r.shape] += int(len(r.clauses) == 32 and len(r.groups) == 8 and len({c[0] for c in r.clauses}) == 4)
            seen["all_limits"] += int(len(r.clauses) == 32 and len(r.functions) == 8)
            seen["mask0"] += int(r.functions == ((0, 2.0),))
            seen["lastword_function"] += int(r.functions == ((fc.LASTWORD, 3.0),))
            seen["lastword_filter"] += int(r.filter == (fc.LASTWORD,))
            seen["third_must_not"] += int(r.must_not == (fc.THIRD,))
            seen["msm_per_group"] += int(isinstance(r.msm, tuple))
            seen["twice"] += int(r.grouped and len(r.groups) == 2 and r.groups[0][0] == r.groups[1][0])
            seen["min_score", r.min_excluded] += int(r.min_score > 0)
            seen["lists", len(r.lists)] += int(entry == "text_knn")
            seen["nested", r.nested] += int(entry == "text_knn" and bool(r.lists))
            seen["shape", r.shape, r.operator, r.msm, r.tie_breaker] += int(r.grouped)
            if entry == "text_knn" and r.filter == (fc.THIRD,) and r.lists:
                seen["outside"] += int(m.kinds(r)["outside"] > 0)
    assert all(seen["modes", s, b] >= 2 for s, b in fc.MODE_PAIRS) and seen["eight"] >= 4 and seen["all_limits"] >= 2, dict(seen)
    assert all(seen["limits", s] >= 2 for s in ("cross_fields", "best_fields")) and seen["mask0"] >= 2 and seen["twice"] >= 4 and seen["msm_per_group"] >= 2, dict(seen)
    assert seen["lastword_function"] >= 2 and seen["lastword_filter"] >= 4 and seen["third_must_not"] >= 4, dict(seen)
    assert all(seen["shape", s, o, n, t] >= 1 for s in ("cross_fields", "best_fields") for o, n in (("should", 0), ("must", 0), ("should", 2)) for t in (0.0, 0.3, 1.0))
    assert all(seen["lists", n] >= 4 for n in (0, 1, 3)) and seen["nested", False] >= 4 and seen["nested", True] >= 8, dict(seen)
    if m.n_docs >= 64:
        assert seen["min_score", True] >= 2 and seen["min_score", False] >= 2 and seen["outside"] >= 1, dict(seen)
    if layout == "gaps":
        for si in fc.GAPS_ABSENT:
            assert all(len(corpus.segments[si].postings(t)[0]) == 0 for corpus in m.fields for t in fc.QUERY_TERMS)
        leaf, field, term = fc.GAPS_ONE_FIELD
        assert len(m.fields[field].segments[leaf].postings(term)[0]) == 0 and len(m.fields[0].segments[leaf].postings(term)[0]) > 0
        for entry in fc.ENTRIES:
            for r in reqs[entry]:
                assert {t for _, t, _ in r.clauses} <= set(fc.QUERY_TERMS) | {fc.TERM_NOWHERE}
                if not r.lists:
                    assert not set(m.kept_leaves(r)) & set(fc.GAPS_ABSENT) and (not m.kept_leaves(r) or kept_after_omitted(m, r))
    if layout in ("nine_slices", "sixteen_slices"):
        assert len(m.slices) > fc.SLICE_SLOTS and all(m.expected(r)[2] > 0 for r in reqs["multi_match"] if r.operator == "should" and not r.filter)
    if layout == "many_small":
        assert len(m.sizes) == 40 and all(len(m.kept_leaves(r)) == 40 for r in reqs["function_score"])


# ---- 3. the glue against plain loops --------------------------------------------------------------------------------------------------------
def _bit(words, d: int) -> bool:
    return bool((int(words[d >> 6]) >> (d & 63)) & 1)


def _r32(x: float) -> float:
    return float(f32(x))


def _add(values) -> float:
    """a float64 sum, one addition after the other"""
    acc = 0.0
    for v in values:
        acc = acc + v
    return acc


def loop_multi_match(r: fc.Req, sc):
    """(inner, is_hit) of one doc by the rules of _multi_match_ref's docstring; sc: per clause the float32 score or None"""
    tb = _r32(r.tie_breaker)

    def dismax(best, total):
        return _r32(best + (total - best) * tb)

    cross, must = r.shape == "cross_fields", r.operator == "must"
    at, o_sum, o_best, o_n, seen = 0, 0.0, 0.0, 0, []
    for g in r.groups:
        ms = [x for x in sc[at: at + len(g)] if x is not None]
        at += len(g)
        if cross:
            g_match, s_g = len(ms) > 0, dismax(max(ms, default=0.0), _add(ms))
        else:
            need = r.msm[len(seen)] if isinstance(r.msm, tuple) else r.msm
            g_match, s_g = len(ms) >= (len(g) if must else max(1, need)), _r32(_add(ms))
        seen.append(g)
        if g_match:
            o_sum, o_best, o_n = o_sum + s_g, max(o_best, s_g), o_n + 1
    if cross:
        return _r32(o_sum), (o_n == len(r.groups) if must else o_n >= max(1, r.msm))
    return dismax(o_best, o_sum), o_n > 0


def loop_function_score(m: fc.Model, r: fc.Req, si: int, d: int, inner: float):
    """(final, is_hit) by the rules of _function_score_ref's docstring"""
    final = inner
    if r.functions:
        holds = [i == 0 or _bit(m.masks[i][si], d) for i, _ in r.functions]
        if r.score_mode == "multiply":
            v = 1.0
            for h, (_, w) in zip(holds, r.functions):
                v = v * _r32(w) if h else v
        else:
            v = _add(_r32(w) for h, (_, w) in zip(holds, r.functions) if h) if any(holds) else 1.0
        final = _r32(inner * v) if r.boost_mode == "multiply" else _r32(inner + v) if r.boost_mode == "sum" else _r32(v)
    ms = _r32(r.min_score)
    hit = True
    if ms > 0 or r.min_excluded:
        hit = final > ms or (final == ms and not r.min_excluded)
    return final, hit


def loop_expected(m: fc.Model, r: fc.Req):
    """one doc at a time; then sorted() by (-score, doc), the cursor, the cut at k.  One slice, a threshold nobody reaches."""
    per = [mm_ref.clause_scores(oracle, m.fields, c) for c in r.clauses]
    hits = []
    for si, seg in enumerate(m.segments):
        scores = [dict(zip(p[si][0].tolist(), p[si][1].tolist())) for p in per]
        for d in range(seg.max_doc):
            live = seg.live_bits is None or _bit(seg.live_bits, d)
            accepted = live and all(_bit(m.masks[i][si], d) for i in r.filter) and not any(_bit(m.masks[i][si], d) for i in r.must_not)
            sc = [s.get(d) for s in scores]
            if r.grouped:
                inner, inner_hit = loop_multi_match(r, sc)
            else:
                ms = [x for x in sc if x is not None]
                text, inner_hit = _add(ms), len(ms) > 0
                inner = _r32(text)
            if r.entry == "text_knn":
                text_ok = inner_hit and accepted
                vals = [_r32(f32(s[docs.index(seg.doc_base + d)]) * f32(b)) for docs, s, b in r.lists if seg.doc_base + d in docs]
                listed = bool(vals) and live
                if not (text_ok or listed):
                    continue
                ks = _add(vals)
                final = (_r32(_r32(text) + ks) if r.nested else _r32(text + ks)) if text_ok and listed else _r32(text) if text_ok else _r32(ks)
            else:
                if not (accepted and inner_hit):
                    continue
                final, hit = loop_function_score(m, r, si, d, inner) if r.scored else (inner, True)
                if not hit:
                    continue
            hits.append((-final, seg.doc_base + d))
    page = sorted(hits)
    if r.after is not None:
        page = [(s, d) for s, d in page if -s < r.after[1] or (-s == r.after[1] and d > r.after[0])]
    page = page[: r.k]
    return [d for _, d in page], [int(f32(-s).view(np.uint32)) for s, _ in page], len(hits), False


def test_the_model_equals_plain_loops():
    sizes = (1, 64, 65)
    fields = fc.build_fields(sizes, 2, 71, deletes=0.0)
    for corpus in fields:   # one deleted doc: the last but one of the last leaf
        corpus.segments[2].live_bits = mm_ref.words_of(np.arange(65) != 63)
    m = fc.Model(fields, fc.sweep_masks(sizes, 72))
    assert len(m.slices) == 1
    reqs, _ = fc.sweep_requests(m, 73)
    paged = runs = nested = 0
    for entry in fc.ENTRIES:
        assert len(reqs[entry]) >= 30
        for r in reqs[entry]:
            r = dataclasses.replace(r, threshold=fc.INT_MAX)   # (the relation is the collector's business: the count is exact, EQUAL_TO)
            got, exp = m.expected(r), loop_expected(m, r)
            got = (got[0].tolist(), got[1].view(np.uint32).tolist(), got[2], got[3])
            assert got == exp, f"{fc.describe(r)}: the model {got}, the loop {exp}"
            paged += int(r.after is not None and len(got[0]) > 0)
            runs += int(in_a_run(m, r))
            nested += int(entry == "text_knn" and r.nested and m.kinds(r)["text"] > 0)
    assert paged >= 40 and runs >= 2 and nested >= 4
