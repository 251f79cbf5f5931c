"""The four routes on csrc/finalscore.hiph's skeleton -- function score, multi-match, function score over multi-match, a text
query beside knn clauses -- through the C ABI on the device over the layouts the one fixed test index cannot reach: leaves that end
on and next to the 64-doc mask word, the 1024-doc sub-tile and a full round of 8 / 12 sub-tiles; 40 small leaves in one item; a
one-doc part at either end; 8, 9 and 16 searcher slices (kSliceSlots = 8: the 8 | 9 item cut); leaves without a query term between
leaves with them; leaves without liveDocs next to leaves with them.  The cases and what each must return come from
tests/_final_score_cases.py (sweep_case: the layouts, the masks whose edge docs decide the answers, the requests); here are the
upload, the calls and the comparisons.  Bit-exact: docids, ranks, float32 score bits, the exact total_hits and the relation.
Needs a real MI355X."""
import dataclasses

import numpy as np
import pytest

from nrtsearch_amd import api

from tests import _final_score_cases as fc
from tests.test_parity_gpu import assert_same

pytestmark = pytest.mark.gpu
MAX_BATCH = 64


@pytest.fixture(scope="module", autouse=True)
def two_column_postings():
    """The routes refuse packed postings: these contexts keep the two-column layout also where the whole suite runs with
    NRTGPU_PACKED_POSTINGS=1, which packs every api.GpuContext."""
    mp = pytest.MonkeyPatch()
    mp.delenv("NRTGPU_PACKED_POSTINGS", raising=False)
    yield
    mp.undo()


def open_context(m: fc.Model):
    ctx = api.GpuContext(device_id=0, max_batch=MAX_BATCH, target_items=m.target_items)
    if m.slicing != fc.DEFAULT_SLICING:
        ctx.set_slicing(*m.slicing)
    return ctx


def upload(ctx, m: fc.Model):
    """The model's leaves and masks on the device -> (leaves, searcher)."""
    leaves, stats = m.upload(ctx)
    for mid, words in m.masks.items():
        for leaf, w in zip(leaves, words):
            leaf.set_mask(mid, w)
    return leaves, api.GpuIndexSearcher(ctx, leaves, stats)


def supported(searcher, m: fc.Model, r: fc.Req) -> bool:
    q, mgr = fc.query_of(m, r), fc.manager_of(r)
    if r.entry == "function_score":
        return searcher.function_score_supported(q, mgr)
    if r.entry == "multi_match":
        return searcher.multi_match_supported(q, mgr)
    if r.entry == "function_score_multi_match":
        return searcher.function_score_multi_match_supported(q, mgr)
    return searcher.text_knn_supported(q, fc.knn_clauses_of(r), mgr)


def run(searcher, m: fc.Model, entry: str, reqs):
    """one call of the entry over the requests (at most the context's max_batch of them)"""
    queries, managers = [fc.query_of(m, r) for r in reqs], [fc.manager_of(r) for r in reqs]
    if entry == "function_score":
        return searcher.search_function_score_batch(queries, managers)
    if entry == "multi_match":
        return searcher.search_multi_match_batch(queries, managers)
    if entry == "function_score_multi_match":
        return searcher.search_function_score_multi_match_batch(queries, managers)
    return searcher.search_text_knn_batch(queries, [fc.knn_clauses_of(r) for r in reqs], managers)


def check(name: str, m: fc.Model, r: fc.Req, got):
    exp = m.expected(r)
    assert_same(name, got, exp, r.k, r.threshold)
    assert got.total_hits == exp[2], f"{name}: total_hits {got.total_hits}, the reference counts {exp[2]}"
    assert len(got.docs) == 0 or (0 <= int(got.docs.min()) and int(got.docs.max()) < m.n_docs), f"{name}: a docid at or beyond {m.n_docs}"


def release(leaves):
    for leaf in leaves:
        leaf.release()


@pytest.mark.parametrize("layout", fc.LAYOUTS, ids=[str(l) for l in fc.LAYOUTS])
def test_layout(layout):
    m, reqs, _ = fc.sweep_case(layout)
    ctx = open_context(m)
    leaves = []
    try:
        leaves, searcher = upload(ctx, m)
        for entry in fc.ENTRIES:
            rs = reqs[entry]
            for lo in range(0, len(rs), MAX_BATCH):
                batch = rs[lo: lo + MAX_BATCH]
                names = [f"layout {layout}, {entry}[{lo + i}]: {fc.describe(r)}" for i, r in enumerate(batch)]
                for name, r in zip(names, batch):
                    assert supported(searcher, m, r) is True, name
                got = run(searcher, m, entry, batch)
                d = api.GpuContext.last_diagnostics()
                live = sum(1 for r in batch if m.kept_leaves(r))   # the queries with a part: a posting of a clause or a listed doc in some leaf
                assert d["items_maxscore"] == 0, names[0]
                if layout in ("nine_slices", "sixteen_slices"):   # no item holds more than kSliceSlots slices
                    assert d["items_scan"] >= 2 * live, (names[0], d["items_scan"], live)
                if layout == "eight_slices":
                    assert d["items_scan"] == live, (names[0], d["items_scan"], live)
                for name, r, g in zip(names, batch, got):
                    check(name, m, r, g)
    finally:
        release(leaves)
        ctx.close()


# ---- named cases, spelled out by hand; a mismatch that the sweep or the fuzz (tests/test_fuzz_final_score_gpu.py) finds is added here -----
def slice_counts(m: fc.Model, r: fc.Req):
    """per searcher slice (hits, hits behind the request's cursor), from the reference's whole hit list"""
    docs, scores = m.expected(dataclasses.replace(r, after=None, k=1024, threshold=fc.INT_MAX))[:2]
    assert len(docs) < 1024   # the whole list
    bases = np.cumsum([0] + m.sizes)
    leaf = np.searchsorted(bases, docs, side="right") - 1
    a_doc, a_score = r.after
    past = (scores < np.float32(a_score)) | ((scores == np.float32(a_score)) & (docs > a_doc))
    return [(int(np.isin(leaf, g).sum()), int((np.isin(leaf, g) & past).sum())) for g in m.slices]


def test_a_page_that_no_single_slice_fills_is_equal_to():
    """Two leaves, each a searcher slice of its own, about 400 hits in each; numHits 300, threshold 10.  A collector with a cursor
    counts every hit but queues only those behind it, and its count becomes a lower bound only once its queue is full.  With the
    cursor 400 hits before the end, each slice has more than 300 hits but about 200 behind the cursor: no queue fills, EQUAL_TO --
    although the merged page is full.  (The fuzz found the device answering GREATER_THAN_OR_EQUAL_TO here: it asked for one slice
    above the floor and a full page.)  With the cursor 700 before the end one slice fills its queue alone."""
    fields = fc.build_fields((2085, 2085), 2, 91)
    m = fc.Model(fields, fc.sweep_masks((2085, 2085), 92), slicing=(1000, 5))
    assert len(m.slices) == 2
    ctx = open_context(m)
    leaves = []
    try:
        leaves, searcher = upload(ctx, m)
        for entry in fc.ENTRIES:
            kw = dict(groups=fc.groups_of("cross_fields", (3,), (0,)), shape="cross_fields") if entry.endswith("multi_match") else dict(groups=fc.flat((3,)))
            if entry.startswith("function_score"):
                kw.update(functions=((fc.THIRD, 1.5), (0, 0.5)), score_mode="sum")
            if entry == "text_knn":
                kw.update(lists=(fc.edge_list(m, 93),))
            whole = m.expected(fc.Req(entry, k=1024, threshold=fc.INT_MAX, **kw))
            for back, gte in ((400, False), (700, True)):
                at = whole[2] - back - 1
                r = fc.Req(entry, k=300, threshold=10, after=(int(whole[0][at]), float(whole[1][at])), **kw)
                counts = slice_counts(m, r)
                assert all(h > 300 for h, _ in counts) and sum(p for _, p in counts) == back and any(p >= 300 for _, p in counts) == gte, counts
                exp = m.expected(r)
                assert len(exp[0]) == 300 and exp[3] == gte
                name = f"{entry}, the cursor {back} before the end: per slice (hits, behind the cursor) {counts}"
                assert supported(searcher, m, r) is True, name
                check(name, m, r, run(searcher, m, entry, [r])[0])
    finally:
        release(leaves)
        ctx.close()
