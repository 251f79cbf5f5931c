"""Filter masks built on the device from 64-bit doc value columns (nrtgpu_segment_set_mask_from_values64) against
tests/_value_masks64_ref.py: every word of every mask, the counts, and the masks at work as filters of a BM25 search and of a
sorted search over the same column ("in the last 30 days, newest first").  Exact equality throughout.  Needs a real MI355X."""
import numpy as np
import pytest

from nrtsearch_amd import _lib, api

from tests import _field_sort64_ref as ref
from tests import _field_sort_ref as fs
from tests import _value_masks64_ref as mref

pytestmark = pytest.mark.gpu
LCOL, DCOL, FULL, RATING = 7, 8, 9, 10
DAY = 86_400_000
NOW = 1_700_000_000_000
SIZES = [40, 1500, 3000]
LONG_EDGES = [ref.INT64_MIN, -1, 0, 1, NOW - 30 * DAY, NOW, ref.INT64_MAX]
DOUBLE_EDGE_BITS = [0xFFF0000000000000, ref.bits_of("double", -1.5), 0x8000000000000000, 0, 1, ref.bits_of("double", 3.25), 0x7FF0000000000000,
                    0x7FF8000000000000, 0x7FF0000000000001, 0xFFF8000000000123]


@pytest.fixture(scope="module", autouse=True)
def two_column_postings():
    mp = pytest.MonkeyPatch()
    mp.delenv("NRTGPU_PACKED_POSTINGS", raising=False)
    yield
    mp.undo()


@pytest.fixture(scope="module")
def index():
    c = api.GpuContext(device_id=0, max_batch=64)
    corpus = fs.make_corpus(SIZES, {1: 0.5, 2: 0.3}, seed=15, delete_fraction=0.02)
    rng = np.random.default_rng(16)
    cols = {LCOL: [], DCOL: [], FULL: [], RATING: []}
    for seg in corpus.segments:
        n = seg.max_doc
        d = np.nonzero(rng.random(n) < 0.7)[0].astype(np.int32)
        cols[LCOL].append((d, rng.choice(np.array(LONG_EDGES, dtype=np.int64).view(np.uint64), size=len(d))))
        d = np.nonzero(rng.random(n) < 0.7)[0].astype(np.int32)
        cols[DCOL].append((d, rng.choice(np.array(DOUBLE_EDGE_BITS, dtype=np.uint64), size=len(d))))
        cols[FULL].append((None, (NOW - rng.integers(0, 365, size=n).astype(np.int64) * DAY).view(np.uint64)))   # a year of days: every doc
        cols[RATING].append((None, rng.integers(0, 6, size=n).astype(np.int32).view(np.uint32)))

    def more(g, si):
        g.add_doc_values64(DCOL, "double", cols[DCOL][si][1], cols[DCOL][si][0])
        g.add_doc_values64(FULL, "long", cols[FULL][si][1])
        g.add_doc_values(RATING, "int", cols[RATING][si][1])

    leaves = ref.upload(c, corpus, "long", cols[LCOL], column_field=LCOL, more=more)
    yield c, corpus, cols, leaves
    for l in leaves:
        l.release()
    c.close()


def built(leaf, mask_id, clauses):
    """(count the call reports, the words get_mask returns)"""
    return leaf.set_mask_from_values64(mask_id, clauses), leaf.get_mask(mask_id)


def test_range_and_exists_over_the_edge_values(index):
    ctx, corpus, cols, leaves = index
    VC = api.ValueClause64
    longs = [ref.bits_of("long", v) for v in LONG_EDGES]
    for si, (seg, leaf) in enumerate(zip(corpus.segments, leaves)):
        n = seg.max_doc
        cases = [("long", LCOL, lo, hi) for lo in longs for hi in longs] + [("double", DCOL, lo, hi) for lo in DOUBLE_EDGE_BITS for hi in DOUBLE_EDGE_BITS]
        empty = 0
        for kind, field, lo, hi in cases:
            count, words = built(leaf, 20, [VC("range", field, kind, lo, hi)])
            exp = mref.mask(n, [(cols[field][si], kind, ("range", lo, hi))])
            assert words.tolist() == exp.tolist(), (si, kind, hex(lo), hex(hi))
            assert count == int(fs._bits(exp, n).sum())
            empty += int(ref.order_int(kind, lo) > ref.order_int(kind, hi) and count == 0)
        assert empty > 20   # lower > upper: an empty range, not an error
        for kind, field in (("long", LCOL), ("double", DCOL), ("long", FULL)):
            count, words = built(leaf, 21, [VC.exists(field)])
            exp = mref.mask(n, [(cols[field][si], kind, ("exists",))])
            assert words.tolist() == exp.tolist() and count == int(fs._bits(exp, n).sum())
            if n % 64:
                assert int(words[-1]) >> (n % 64) == 0   # bits at or beyond max_doc are 0 (FULL: every doc has a value)
        assert built(leaf, 21, [VC.exists(FULL)])[0] == n


def test_the_nan_and_signed_zero_rules(index):
    ctx, corpus, cols, leaves = index
    VC = api.ValueClause64
    si, leaf, n = 2, leaves[2], SIZES[2]
    d, bits = cols[DCOL][si]
    is_nan = (bits & np.uint64(2**63 - 1)) > np.uint64(0x7FF0000000000000)
    everything = built(leaf, 22, [VC.range_(DCOL, "double", float("-inf"), float("inf"))])
    assert everything[0] == int((~is_nan).sum()) > 0                                   # [-inf, +inf] drops the NaN docs
    nans = built(leaf, 22, [VC("range", DCOL, "double", 0x7FF8000000000000, 0xFFF8000000000123)])
    assert nans[0] == int(is_nan.sum()) > 0                                            # [NaN, NaN] keeps only them, whatever the payloads
    assert sorted(np.nonzero(fs._bits(nans[1], n))[0].tolist()) == sorted(d[is_nan].tolist())
    pz = built(leaf, 22, [VC.range_(DCOL, "double", 0.0, 0.0)])
    nz = built(leaf, 22, [VC.range_(DCOL, "double", -0.0, -0.0)])
    assert pz[0] == int((bits == 0).sum()) > 0 and nz[0] == int((bits == np.uint64(2**63)).sum()) > 0   # -0.0 and +0.0 are two values
    assert built(leaf, 22, [VC.range_(DCOL, "double", 0.0, -0.0)])[0] == 0            # -0.0 < +0.0: an empty range
    assert built(leaf, 22, [VC.range_(DCOL, "double", -0.0, 0.0)])[0] == pz[0] + nz[0]


def test_several_clauses_and_the_mask_at_work(index):
    ctx, corpus, cols, leaves = index
    VC = api.ValueClause64
    cut = NOW - 30 * DAY
    last30, rated, both = [], [], []
    for si, (seg, leaf) in enumerate(zip(corpus.segments, leaves)):
        n = seg.max_doc
        count, words = built(leaf, 30, [VC.range_(FULL, "long", cut, NOW), VC.exists(LCOL)])
        exp = mref.mask(n, [(cols[FULL][si], "long", ("range", ref.bits_of("long", cut), ref.bits_of("long", NOW))), (cols[LCOL][si], "long", ("exists",))])
        assert words.tolist() == exp.tolist() and count == int(fs._bits(exp, n).sum())
        count, words = built(leaf, 31, [VC.range_(FULL, "long", cut, NOW)])             # "in the last 30 days"
        last30.append(words)
        assert 0 < count < n or n == 40
        leaf.set_mask_from_values(32, [api.ValueClause.range_(RATING, "int", 4, 5)])     # a 32-bit built mask beside it: "rating >= 4"
        rated.append(leaf.get_mask(32))
    s = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics.from_corpus(corpus))
    MF = api.MaskFilter
    # as filter_mask of a BM25 search: the hits are the filtered docs (total_hits exact under a high threshold)
    q = api.BooleanQuery((api.TermQuery(0, 1), api.TermQuery(0, 2)), 1, (MF(31),))
    td = s.search_batch([q], [api.TopScoreDocCollectorManager(10, None, 2**31 - 1)])[0]
    accept = [seg.live_bits[: len(w)] & w for seg, w in zip(corpus.segments, last30)]
    hits = ref.text_hits(corpus, (1, 2), 1, accept=accept)
    assert td.total_hits == sum(int(h.sum()) for h in hits) > 0
    # "last 30 days, newest first": the same mask as the filter of a sorted search over the same column
    for rev in (True, False):
        got = api.search_sorted64_batch(s, [q], [api.TopScoreDocCollectorManager(100)], [api.SortField64(FULL, "long", rev)])[0]
        exp = ref.search(corpus, hits, cols[FULL], "long", 100, rev)
        assert got.docs.tolist() == exp[0].tolist() and got.value_bits.tolist() == exp[1].tolist() and got.total_hits == exp[2]
        assert got.values.min() >= cut
    # "rating >= 4 AND last 30 days": two masks, filter_mask and more_filters
    q2 = api.BooleanQuery((api.TermQuery(0, 1), api.TermQuery(0, 2)), 1, (MF(32), MF(31)))
    accept2 = [a & r for a, r in zip(accept, rated)]
    hits2 = ref.text_hits(corpus, (1, 2), 1, accept=accept2)
    got = api.search_sorted64_batch(s, [q2], [api.TopScoreDocCollectorManager(100)], [api.SortField64(FULL, "long", True)])[0]
    exp = ref.search(corpus, hits2, cols[FULL], "long", 100, True)
    assert got.docs.tolist() == exp[0].tolist() and got.value_bits.tolist() == exp[1].tolist() and got.total_hits == exp[2] > 0
    got = api.search_docset_sorted64_batch(s, [api.DocSetQuery((MF(32), MF(31)))], [api.TopScoreDocCollectorManager(100)],
                                           [api.SortField64(FULL, "long", True)])[0]
    exp = ref.search(corpus, ref.docset_hits(corpus, filters=[rated, last30]), cols[FULL], "long", 100, True)
    assert got.docs.tolist() == exp[0].tolist() and got.value_bits.tolist() == exp[1].tolist() and got.total_hits == exp[2] > 0


def test_refusals_and_timing(index):
    ctx, corpus, cols, leaves = index
    VC = api.ValueClause64
    leaf = leaves[1]
    leaf.set_mask_from_values64(40, [VC.exists(FULL)])
    kept = leaf.get_mask(40)
    for clauses, says in (([VC.exists(55)], "55"), ([VC.exists(RATING)], "nrtgpu_segment_set_mask_from_values")):
        with pytest.raises(_lib.NrtGpuError) as e:
            leaf.set_mask_from_values64(40, clauses)
        assert e.value.code == _lib.NRTGPU_ERR_UNSUPPORTED and says in str(e.value)
        assert leaf.get_mask(40).tolist() == kept.tolist()   # a failed call leaves the old mask in place
    with pytest.raises(_lib.NrtGpuError) as e:
        leaf.set_mask_from_values(40, [api.ValueClause.exists(FULL)])
    assert e.value.code == _lib.NRTGPU_ERR_UNSUPPORTED and "nrtgpu_segment_set_mask_from_values64" in str(e.value)
    c2 = api.GpuContext(device_id=0, max_batch=16, collect_timing=True)
    try:
        seg = corpus.segments[2]
        g = ref.upload(c2, fs.make_corpus([3000], {1: 0.5}, seed=17), "long", [cols[FULL][2]], column_field=FULL)[0]
        assert g.set_mask_from_values64(41, [VC.range_(FULL, "long", NOW - 30 * DAY, NOW)]) > 0
        d = api.GpuContext.last_diagnostics()
        assert 0.0 < d["device_ms"] <= d["total_ms"]
        g.release()
    finally:
        c2.close()
