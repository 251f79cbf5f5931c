"""The two routes of nrtgpu_search_bm25_batch -- the exhaustive scan (csrc/kernels.hip) and the MaxScore walk (csrc/maxscore.hip) --
through the C ABI on the device over the layouts the fixed test corpora cannot reach: leaves that end on and next to the 64-doc mask
word, the 1024-doc sub-tile, a full 12-wave round of 12 288 docs and the MaxScore window of 64 x 1024 docs; 40 small leaves in one
item; a one-doc part at either end; 8, 9 and 16 searcher slices (kSliceSlots = 8: the 8 | 9 item cut, slice_relation_kernel's
loop, MaxScore's "count until SOME slice passes the floor"); leaves without a query term between leaves with them (omitted parts,
tile_offset); leaves without liveDocs next to leaves with them.  Every layout under the default flags (MaxScore for the requests
of up to 8 clauses) and under NRTGPU_FLAG_NO_PRUNE (the scan for all of them), over plain and packed postings.  The cases and what
each must return come from tests/_bm25_cases.py (sweep_case: edge docs that head the page, masks that accept or reject exactly
them, a copy of the index that deletes exactly them, the shaped queries, cursors inside runs of equal scores and on both sides of
the documented cursor / slice rule); here are the upload, the calls and the comparisons.  Bit-exact: docids, ranks, float32 score
bits, the relation, and the count -- exact, or under GREATER_THAN_OR_EQUAL_TO a bound in (max(threshold, numHits), exact].
Needs a real MI355X."""
import numpy as np
import pytest

from nrtsearch_amd import _lib, api

from tests import _bm25_cases as bc
from tests.test_parity_gpu import assert_same

pytestmark = pytest.mark.gpu
MAX_BATCH = 128
FLAG_SETS = {"default": 0, "no_prune": bc.NO_PRUNE}


def open_context(m: bc.Model, flags: int = 0, packed: bool = False, budget_pct: int = 0):
    """packed: the context's own flag, whatever NRTGPU_PACKED_POSTINGS says (the environment can only add it)"""
    ctx = api.GpuContext(device_id=0, max_batch=MAX_BATCH, target_items=m.target_items, flags=flags | (_lib.NRTGPU_FLAG_PACKED_POSTINGS if packed else 0),
                         lookup_budget_pct=budget_pct)
    if m.slicing != bc.DEFAULT_SLICING:
        ctx.set_slicing(*m.slicing)
    return ctx


def upload(ctx, m: bc.Model):
    """The model's leaves and masks on the device -> (leaves, searcher)."""
    leaves = [api.GpuSegment.from_data(ctx, seg) for seg in m.segments]
    for mid, words in m.masks.items():
        for leaf, w in zip(leaves, words):
            leaf.set_mask(mid, w)
    return leaves, api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics.from_corpus(m.corpus))


def release(leaves):
    for leaf in leaves:
        leaf.release()


def run(searcher, reqs):
    return searcher.search_batch([bc.query_of(r) for r in reqs], [bc.manager_of(r) for r in reqs])


def check(name: str, m: bc.Model, r: bc.Req, got):
    """docids, score bits, the relation, and the count: exact, or for GREATER_THAN_OR_EQUAL_TO in (max(threshold, numHits), exact]"""
    exp = m.expected(r)
    assert_same(name, got, exp, r.k, r.threshold)
    assert len(got.docs) == 0 or (0 <= int(got.docs.min()) and int(got.docs.max()) < m.n_docs), f"{name}: a docid at or beyond {m.n_docs}"


def same_pages(name: str, a, b):
    """two routes' answers to one request: the same hits, score bits and relation; the same count where it is exact"""
    assert a.docs.tolist() == b.docs.tolist(), f"{name}: the routes' docids differ"
    assert a.scores.view(np.uint32).tolist() == b.scores.view(np.uint32).tolist(), f"{name}: the routes' score bits differ"
    assert a.relation_gte == b.relation_gte, f"{name}: the routes' relations differ"
    assert a.relation_gte or a.total_hits == b.total_hits, f"{name}: the routes' exact counts differ ({a.total_hits}, {b.total_hits})"


def assert_routes(name: str, flags: int, d: dict, reqs, m: bc.Model):
    if flags & (bc.NO_PRUNE | bc.NO_FIXED_POINT):
        assert d["items_maxscore"] == 0, (name, d)
        assert d["items_scan"] > 0 or not any(m.matches_something(r) for r in reqs), (name, d)
    elif any(bc.on_maxscore(r, flags) and m.matches_something(r) for r in reqs):
        assert d["items_maxscore"] > 0, (name, d)


@pytest.mark.parametrize("packed", (False, True), ids=("plain", "packed"))
@pytest.mark.parametrize("flag_set", list(FLAG_SETS))
@pytest.mark.parametrize("layout", bc.LAYOUTS, ids=[str(l) for l in bc.LAYOUTS])
def test_layout(layout, flag_set, packed):
    flags = FLAG_SETS[flag_set]
    m, reqs, _ = bc.sweep_case(layout)
    reqs = [r for r in reqs if bc.taken_by(r, flags)]     # (the second-accumulator shapes: the MaxScore route only)
    assert len(reqs) >= 30
    ctx = open_context(m, flags, packed)
    leaves, forks = [], []
    try:
        leaves, searcher = upload(ctx, m)
        names = [f"layout {layout}, {flag_set}, {'packed' if packed else 'plain'}, request {i}: {bc.describe(r)}" for i, r in enumerate(reqs)]
        got = run(searcher, reqs)
        d = api.GpuContext.last_diagnostics()
        assert_routes(names[0], flags, d, reqs, m)
        live = sum(1 for r in reqs if m.matches_something(r))
        items = d["items_maxscore"] + d["items_scan"]
        if layout == "eight_slices":                      # target_items = 1: one item per query, eight slices in its eight slots
            assert items == live, (names[0], d, live)
        if layout in ("nine_slices", "sixteen_slices"):   # no item holds more than kSliceSlots slices
            assert items >= 2 * live, (names[0], d, live)
        for name, r, g in zip(names, reqs, got):
            check(name, m, r, g)
        # the second copy: the same postings under liveDocs that delete exactly the edge docs
        gone = m.edges_deleted()
        forks = [leaf.fork(seg.live_bits) for leaf, seg in zip(leaves, gone.segments)]
        others = bc.edges_deleted_requests(m)
        got = run(api.GpuIndexSearcher(ctx, forks, api.IndexStatistics.from_corpus(gone.corpus)), others)
        assert_routes(names[0], flags, api.GpuContext.last_diagnostics(), others, gone)
        for i, (r, g) in enumerate(zip(others, got)):
            check(f"layout {layout}, {flag_set}, {'packed' if packed else 'plain'}, edge docs deleted, request {i}: {bc.describe(r)}", gone, r, g)
    finally:
        release(forks)
        release(leaves)
        ctx.close()


@pytest.mark.parametrize("layout", bc.LAYOUTS, ids=[str(l) for l in bc.LAYOUTS])
def test_the_two_routes_return_the_same_pages(layout):
    """The MaxScore walk and the exhaustive scan over one index, request by request, compared with each other directly (each is
    held to the oracle by test_layout): what both take, the requests of nine and ten clauses aside (the scan either way)."""
    m, reqs, _ = bc.sweep_case(layout)
    reqs = [r for r in reqs if bc.taken_by(r, bc.NO_PRUNE) and bc.on_maxscore(r, 0)]
    assert len(reqs) >= 20
    pages = []
    for flags in (0, bc.NO_PRUNE):
        ctx = open_context(m, flags)
        leaves = []
        try:
            leaves, searcher = upload(ctx, m)
            pages.append(run(searcher, reqs))
            assert_routes(f"layout {layout}, flags {flags}", flags, api.GpuContext.last_diagnostics(), reqs, m)
        finally:
            release(leaves)
            ctx.close()
    for i, (r, a, b) in enumerate(zip(reqs, *pages)):
        same_pages(f"layout {layout}, request {i}: {bc.describe(r)}", a, b)
