"""Sort by a 64-bit field (nrtgpu_search_sorted64_batch, nrtgpu_search_docset_sorted64_batch) through the C ABI on the device,
against tests/_field_sort64_ref.py.  Every comparison is exact equality: docids, ranks, the 64 value bits each hit sorted as,
total_hits, the relation.  Needs a real MI355X."""
import ctypes as C

import numpy as np
import pytest

from nrtsearch_amd import _lib, api, synth

from tests import _field_sort64_ref as ref
from tests import _field_sort_ref as fs
from tests.test_field_sort_gpu import QUERIES, T

pytestmark = pytest.mark.gpu
INT_MAX = 2**31 - 1
COL = 7
TERMS = {1: 0.5, 2: 0.3, 3: 0.2}
EPOCH = 1_700_000_000_000
# values that straddle the 32-bit boundary: a key that keeps 32 bits of them fails, and ties decide most ranks
LONG_POOL = np.array([EPOCH + d for d in (0, 1, 2, 2**20, 2**31, 2**32 - 1, 2**32, 2**32 + 1, 2**36)], dtype=np.int64).view(np.uint64)
DOUBLE_POOL = (np.uint64(ref.bits_of("double", 1.5)) + np.array([0, 1, 2, 3, 77, 2**10, 2**20, 2**29, 2**29 + 1, 2**30 - 2, 2**30 - 1, 5], dtype=np.uint64))
POOL = {"long": LONG_POOL, "double": DOUBLE_POOL}
KIND_MIN = {"long": ref.bits_of("long", ref.INT64_MIN), "double": 0xFFF0000000000000}
KIND_MAX = {"long": ref.bits_of("long", ref.INT64_MAX), "double": ref.CANONICAL_NAN}
UNS, INV = _lib.NRTGPU_ERR_UNSUPPORTED, _lib.NRTGPU_ERR_INVALID_ARG


@pytest.fixture(scope="module", autouse=True)
def two_column_postings():
    """The text route refuses packed postings: these contexts keep the two-column layout also where the whole suite runs with
    NRTGPU_PACKED_POSTINGS=1."""
    mp = pytest.MonkeyPatch()
    mp.delenv("NRTGPU_PACKED_POSTINGS", raising=False)
    yield
    mp.undo()


@pytest.fixture(scope="module")
def ctx(two_column_postings):
    c = api.GpuContext(device_id=0, max_batch=256)
    yield c
    c.close()


def release(leaves):
    for l in leaves:
        l.release()


def same(name, got, exp):
    docs, bits, total, gte = exp
    assert got.docs.tolist() == docs.tolist(), f"{name}: docs"
    assert got.value_bits.dtype == np.uint64 and got.value_bits.tolist() == bits.tolist(), f"{name}: value bits"
    assert got.total_hits == total, f"{name}: total_hits {got.total_hits}, the reference counts {total}"
    assert got.relation_gte == gte, f"{name}: relation"


def missing_values(kind):
    """the kind's minimum, its maximum, a value that also occurs"""
    return (KIND_MIN[kind], KIND_MAX[kind], int(POOL[kind][2]))


def sort_field(kind, reverse, missing_bits, field=COL):
    return api.SortField64(field, kind, reverse, ref.value_of(kind, missing_bits))


# ---- index A: leaves of 3000, 1500 and 40 docs; the column on 80 % of leaf 0, every doc of leaf 1, absent from leaf 2 ---------
class IndexA:
    def __init__(self, ctx, kind, corpus, doc_bases=None, pool=None):
        rng = np.random.default_rng(41 if kind == "long" else 42)
        d0 = np.nonzero(rng.random(3000) < 0.8)[0].astype(np.int32)
        pool = POOL[kind] if pool is None else pool
        self.kind, self.corpus, self.doc_bases = kind, corpus, doc_bases
        self.columns = [(d0, rng.choice(pool, size=len(d0))), (None, rng.choice(pool, size=1500)), None]
        self.masks = {(si, mid): synth.random_mask(seg.max_doc, dens, 40 * mid + si)
                      for si, seg in enumerate(corpus.segments) for mid, dens in ((5, 0.6), (6, 0.2))}
        self.accept = [synth.accept_words(seg, self.masks[(si, 5)], self.masks[(si, 6)]) for si, seg in enumerate(corpus.segments)]
        self.leaves = ref.upload(ctx, corpus, kind, self.columns, column_field=COL, doc_bases=doc_bases)
        for (si, mid), bits in self.masks.items():
            self.leaves[si].set_mask(mid, bits)
        self.searcher = api.GpuIndexSearcher(ctx, self.leaves, api.IndexStatistics.from_corpus(corpus))

    def expect(self, clauses, need, masked, k, reverse, missing_bits, live=None, **kw):
        hits = ref.text_hits(self.corpus, clauses, need, accept=self.accept if masked else None, live=live)
        return ref.search(self.corpus, hits, self.columns, self.kind, k, reverse, missing_bits, doc_bases=self.doc_bases, **kw)


@pytest.fixture(scope="module")
def corpus_a():
    c = fs.make_corpus([3000, 1500, 40], TERMS, seed=5, delete_fraction=0.01)
    assert all(seg.live_bits is not None for seg in c.segments)
    return c


@pytest.fixture(scope="module", params=["long", "double"])
def ix_a(request, ctx, corpus_a):
    x = IndexA(ctx, request.param, corpus_a)
    yield x
    release(x.leaves)


def test_every_query_shape_direction_missing_value_and_k(ix_a):
    kind = ix_a.kind
    cases = [(q, k, rev, mb) for q in QUERIES for k in (1, 10, 1024) for rev in (False, True) for mb in missing_values(kind)]
    mgrs = [api.TopScoreDocCollectorManager(k) for _, k, _, _ in cases]
    got = api.search_sorted64_batch(ix_a.searcher, [q[1] for q, _, _, _ in cases], mgrs, [sort_field(kind, rev, mb) for _, _, rev, mb in cases])
    d = api.GpuContext.last_diagnostics()
    assert d["items_maxscore"] == 0 and d["items_scan"] >= len(cases) * 5 // 6
    full_pages = 0
    for ((name, _, clauses, need, masked), k, rev, mb), td in zip(cases, got):
        exp = ix_a.expect(clauses, need, masked, k, rev, mb)
        same(f"{kind}_{name}_k{k}_rev{int(rev)}_missing{mb:#x}", td, exp)
        assert (exp[2] == 0) == (name == "nowhere")
        full_pages += int(k == 1024 and exp[2] > 1024)
    assert full_pages >= 10
    for q, k, rev, mb in cases[:: len(cases) // 6]:
        assert api.sorted64_supported(ix_a.searcher, q[1], api.TopScoreDocCollectorManager(k), sort_field(kind, rev, mb)) is True


@pytest.mark.parametrize("reverse", [False, True])
def test_pages_through_after_equal_one_long_page(ix_a, reverse):
    kind = ix_a.kind
    name, query, clauses, need, masked = QUERIES[1]
    mb = int(POOL[kind][2])
    sort = sort_field(kind, reverse, mb)
    full = api.search_sorted64_batch(ix_a.searcher, [query], [api.TopScoreDocCollectorManager(70)], [sort])[0]
    same(f"{kind}_page70", full, ix_a.expect(clauses, need, masked, 70, reverse, mb))
    after, docs, bits, cut_in_a_run = None, [], [], 0
    for page in range(10):
        got = api.search_sorted64_batch(ix_a.searcher, [query], [api.TopScoreDocCollectorManager(7)], [sort], [after])[0]
        exp = ix_a.expect(clauses, need, masked, 7, reverse, mb, after=None if after is None else (after.doc, ref.bits_of(kind, after.value)))
        same(f"{kind}_page7_{page}", got, exp)
        assert got.total_hits == full.total_hits
        if bits:
            cut_in_a_run += int(bits[-1] == int(got.value_bits[0]))
        docs += got.docs.tolist()
        bits += got.value_bits.tolist()
        after = api.FieldDoc(int(got.docs[-1]), ref.value_of(kind, int(got.value_bits[-1])))
    assert docs == full.docs.tolist() and bits == full.value_bits.tolist()
    assert cut_in_a_run >= 1   # a cursor inside a run of equal values: the docid decides


def test_cursors_at_the_missing_value_and_outside_the_window(ix_a):
    kind = ix_a.kind
    name, query, clauses, need, masked = QUERIES[1]
    mgr = api.TopScoreDocCollectorManager(50)
    # a cursor whose value IS the missing value (the kind's minimum, ascending: the docs without a value come first)
    mb = KIND_MIN[kind]
    sort = sort_field(kind, False, mb)
    first = api.search_sorted64_batch(ix_a.searcher, [query], [mgr], [sort])[0]
    assert int(first.value_bits[-1]) == mb   # (20 % of leaf 0 and all of leaf 2 lack a value: the page ends among them)
    after = api.FieldDoc(int(first.docs[-1]), ref.value_of(kind, mb))
    got = api.search_sorted64_batch(ix_a.searcher, [query], [mgr], [sort], [after])[0]
    same(f"{kind}_after_missing", got, ix_a.expect(clauses, need, masked, 50, False, mb, after=(after.doc, mb)))
    assert got.docs[0] > first.docs[-1] or int(got.value_bits[0]) != mb
    # the clamp trap: a cursor value outside [lo, hi] that is NOT the missing value -- every real doc lies behind it, no missing doc
    # does.  A compare of clamped keys would put the cursor ON the missing docs' sentinel and return those behind after_doc.
    trap = ref.bits_of("long", ref.INT64_MIN + 5) if kind == "long" else ref.bits_of("double", -1e300)
    after = api.FieldDoc(0, ref.value_of(kind, trap))
    got = api.search_sorted64_batch(ix_a.searcher, [query], [mgr], [sort], [after])[0]
    exp = ix_a.expect(clauses, need, masked, 50, False, mb, after=(0, trap))
    same(f"{kind}_clamp_trap", got, exp)
    assert mb not in got.value_bits.tolist() and got.total_hits == first.total_hits
    # and descending under the kind's maximum: a cursor just below the maximum, above every real value
    mb = KIND_MAX[kind]
    trap = ref.bits_of("long", ref.INT64_MAX - 5) if kind == "long" else 0x7FF0000000000000
    sort = sort_field(kind, True, mb)
    got = api.search_sorted64_batch(ix_a.searcher, [query], [mgr], [sort], [api.FieldDoc(0, ref.value_of(kind, trap))])[0]
    same(f"{kind}_clamp_trap_desc", got, ix_a.expect(clauses, need, masked, 50, True, mb, after=(0, trap)))
    assert mb not in got.value_bits.tolist()


# ---- docid bits ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first_base", [2**30, 0])
def test_doc_bases_set_the_docid_field(ctx, corpus_a, first_base):
    """Leaves based from 2^30 (31 docid bits) and from 0 (13): the same ranks, other global docids.  31 docid bits leave 33 for the
    values: the column draws from the pool without its + 2^36 member (a span of 2^32 + 1), which the whole pool's 37 bits exceed --
    the whole pool is refused there, with the bits in the reason."""
    bases = [first_base, first_base + 3000, first_base + 4500]
    x = IndexA(ctx, "long", corpus_a, doc_bases=bases, pool=LONG_POOL[:-1])
    try:
        for name, query, clauses, need, masked in (QUERIES[1], QUERIES[4]):
            for k, rev, mb in ((10, False, KIND_MIN["long"]), (1024, True, KIND_MAX["long"]), (1024, False, int(LONG_POOL[2]))):
                got = api.search_sorted64_batch(x.searcher, [query], [api.TopScoreDocCollectorManager(k)], [sort_field("long", rev, mb)])[0]
                same(f"base{first_base}_{name}_k{k}", got, x.expect(clauses, need, masked, k, rev, mb))
                assert got.docs.min() >= first_base
    finally:
        release(x.leaves)
    if first_base:
        y = IndexA(ctx, "long", corpus_a, doc_bases=bases)
        try:
            with pytest.raises(_lib.NrtGpuError) as e:
                api.search_sorted64_batch(y.searcher, [QUERIES[1][1]], [api.TopScoreDocCollectorManager(10)], [sort_field("long", False, 0)])
            assert e.value.code == UNS and "span needs 37 bits, 31-bit docids leave 33" in str(e.value), str(e.value)
        finally:
            release(y.leaves)


def test_a_single_leaf_below_one_word(ctx):
    corpus = fs.make_corpus([40], {1: 0.8}, seed=6)
    col = [(None, np.random.default_rng(7).choice(LONG_POOL, size=40))]
    leaves = ref.upload(ctx, corpus, "long", col, column_field=COL)
    try:
        s = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics.from_corpus(corpus))
        for rev in (False, True):
            got = api.search_sorted64_batch(s, [T[1]], [api.TopScoreDocCollectorManager(1024)], [sort_field("long", rev, 0)])[0]
            same(f"forty_rev{int(rev)}", got, ref.search(corpus, ref.text_hits(corpus, (1,)), col, "long", 1024, rev, 0))
    finally:
        release(leaves)


def _status(s, query, sort, docset=False):
    """(entry status, predicate status, reason) of one sorted search."""
    mgr = api.TopScoreDocCollectorManager(10)
    L = _lib.load()
    h = api._Outputs64([mgr])
    if docset:
        ds, keep = api._marshal_docsets([query], [mgr])
        fsr = api._field_sorts64([sort], None, 1)
        rc = L.nrtgpu_search_docset_sorted64_batch(s.ctx._h, s._segs, s._bases, len(s.leaves), ds, fsr, 1, h.outs)
        text = L.nrtgpu_last_error().decode()
        return rc, L.nrtgpu_docset_sorted64_supported(s.ctx._h, s._segs, len(s.leaves), ds, fsr), text
    m, fsr = api._marshal_sorted64(s, [query], [mgr], [sort], None)
    rc = L.nrtgpu_search_sorted64_batch(s.ctx._h, s._segs, s._bases, len(s.leaves), m.queries, fsr, 1, h.outs)
    text = L.nrtgpu_last_error().decode()
    return rc, L.nrtgpu_sorted64_supported(s.ctx._h, s._segs, len(s.leaves), m.queries, fsr), text


def test_the_fit_boundary_and_a_double_column_of_both_signs(ctx):
    """3000 docs from base 0: 12 docid bits leave 52 -- a column whose codes span exactly 2^52 - 4 is sorted, 2^52 - 3 refused, the
    predicate and the search agreeing; {-1.0, 1.0} never fits."""
    corpus = fs.make_corpus([3000], {1: 1.0}, seed=12)
    cols = {}
    for field, span in ((20, 2**52 - 4), (21, 2**52 - 3)):
        col = np.full(3000, -17, dtype=np.int64)
        col[2999] = -17 + span
        cols[field] = col
    signs = np.where(np.arange(3000) % 2 == 0, -1.0, 1.0)

    def more(g, si):
        for field, col in cols.items():
            g.add_doc_values64(field, "long", col)
        g.add_doc_values64(22, "double", signs)

    leaves = ref.upload(ctx, corpus, "long", [None], more=more)
    try:
        s = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics.from_corpus(corpus))
        for docset, query in ((False, T[1]), (True, api.DocSetQuery())):
            assert _status(s, query, api.SortField64(20, "long"), docset)[:2] == (0, 0)
            rc, rc2, text = _status(s, query, api.SortField64(21, "long"), docset)
            assert (rc, rc2) == (UNS, UNS) and "span needs 53 bits, 12-bit docids leave 52" in text and "field 21" in text and "query 0" in text, text
            rc, rc2, text = _status(s, query, api.SortField64(22, "double"), docset)
            assert (rc, rc2) == (UNS, UNS) and "span needs" in text, text
        got = api.search_sorted64_batch(s, [T[1]], [api.TopScoreDocCollectorManager(3)], [api.SortField64(20, "long", True)])[0]
        assert got.docs.tolist() == [2999, 0, 1] and got.values.tolist() == [-17 + 2**52 - 4, -17, -17] and got.total_hits == 3000
    finally:
        release(leaves)


# ---- index B: 13 000 docs, a term in 60 % of them: the first round's hits overflow the candidate buffer ----------------------
def test_wave_by_wave_compaction_and_the_selects_radix_fallback(ctx):
    corpus = fs.make_corpus([13_000], {1: 0.6}, seed=8)
    seg = corpus.segments[0]
    assert int((seg.postings(1)[0] < 12 * 1024).sum()) > 3072   # kScanWaves sub-tiles hold more hits than kFsCandCap
    perm = (EPOCH + np.random.default_rng(9).permutation(13_000).astype(np.int64) * 86_400_000)   # a day apart: no ties
    const = np.full(13_000, EPOCH, dtype=np.int64)   # all ties: more than 64 keys share a high word
    columns = {7: [(None, perm.view(np.uint64))], 8: [(None, const.view(np.uint64))]}

    def more(g, si):
        g.add_doc_values64(8, "long", const)

    leaves = ref.upload(ctx, corpus, "long", columns[7], column_field=7, more=more)
    try:
        searcher = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics.from_corpus(corpus))
        cases = [(f, k, rev) for f in (7, 8) for k in (10, 1024) for rev in (False, True)]
        got = api.search_sorted64_batch(searcher, [T[1]] * len(cases), [api.TopScoreDocCollectorManager(k, None, INT_MAX) for _, k, _ in cases],
                                        [api.SortField64(f, "long", rev, 0) for f, _, rev in cases])
        hits = ref.text_hits(corpus, (1,))
        for (f, k, rev), td in zip(cases, got):
            exp = ref.search(corpus, hits, columns[f], "long", k, rev, 0, total_hits_threshold=INT_MAX)
            assert exp[2] > 7000 and len(exp[0]) == k
            same(f"compaction_field{f}_k{k}_rev{int(rev)}", td, exp)
            if f == 8:
                assert td.docs.tolist() == sorted(td.docs.tolist())   # all ties: the first k docs, in both directions
    finally:
        release(leaves)


# ---- index C: one query cut into several items; the last item holds every winner ------------------------------------------
def test_several_items_share_theta(ctx):
    n = 300_000
    corpus = fs.make_corpus([n], {1: 1.0}, seed=10)
    values = EPOCH + (n - np.arange(n, dtype=np.int64)) * 1000   # ascending sort ("oldest first"): the winners are the LAST docs
    columns = [(None, values.view(np.uint64))]
    leaves = ref.upload(ctx, corpus, "long", columns, column_field=COL)
    try:
        searcher = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics.from_corpus(corpus))
        hits = ref.text_hits(corpus, (1,))
        for k, rev in ((10, False), (1024, False), (10, True)):
            got = api.search_sorted64_batch(searcher, [T[1]], [api.TopScoreDocCollectorManager(k)], [api.SortField64(COL, "long", rev, 0)])[0]
            assert api.GpuContext.last_diagnostics()["items_scan"] >= 2
            same(f"items_k{k}_rev{int(rev)}", got, ref.search(corpus, hits, columns, "long", k, rev, 0))
            if not rev:
                assert got.docs.tolist() == list(range(n - 1, n - 1 - k, -1)) and got.total_hits == n
    finally:
        release(leaves)


# ---- counts, relation, forks, bytes ---------------------------------------------------------------------------------------------------
def test_counts_and_relation_equal_the_32_bit_route(ctx, corpus_a):
    """A column that fits 32 bits, uploaded as INT64 under one field and as INT32 under another: total_hits and the relation of the
    two routes are equal, and so are the docs and the values."""
    rng = np.random.default_rng(51)
    small = [rng.integers(-50, 50, size=seg.max_doc).astype(np.int32) for seg in corpus_a.segments]
    cols64 = [(None, v.astype(np.int64).view(np.uint64)) for v in small]

    def more(g, si):
        g.add_doc_values(8, "int", small[si])

    leaves = ref.upload(ctx, corpus_a, "long", cols64, column_field=COL, more=more)
    try:
        s = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics.from_corpus(corpus_a))
        for name, query, clauses, need, masked in QUERIES[:2]:
            for k, thr in ((1, 1000), (10, 1000), (1024, 1000), (10, 5000), (10, 0)):
                mgr = api.TopScoreDocCollectorManager(k, None, thr)
                got = api.search_sorted64_batch(s, [query], [mgr], [api.SortField64(COL, "long", False, 7)])[0]
                old = api.search_sorted_batch(s, [query], [mgr], [api.SortField(8, "int", False, 7)])[0]
                assert (got.total_hits, got.relation_gte) == (old.total_hits, old.relation_gte), (name, k, thr)
                assert got.docs.tolist() == old.docs.tolist() and got.values.tolist() == old.values.tolist()
                same(f"{name}_thr{thr}", got, ref.search(corpus_a, ref.text_hits(corpus_a, clauses, need), cols64, "long", k, False, 7, total_hits_threshold=thr))
    finally:
        release(leaves)


def test_relation_per_slice(corpus_a):
    c = api.GpuContext(device_id=0, max_batch=16)
    x = None
    try:
        c.set_slicing(1000, 5, 1)
        slicing = (1000, 5, 1)
        x = IndexA(c, "long", corpus_a)
        name, query, clauses, need, masked = QUERIES[0]
        info = {}
        x.expect(clauses, need, masked, 10, False, 0, total_hits_threshold=50, slicing=slicing, info=info)
        per_slice = info["slice_hits"]
        assert len(per_slice) == 3 and max(per_slice) > 50 and min(per_slice) <= 50
        for thr, gte in ((50, True), (max(per_slice), False)):
            got = api.search_sorted64_batch(x.searcher, [query], [api.TopScoreDocCollectorManager(10, None, thr)], [sort_field("long", False, 0)])[0]
            same(f"slices_thr{thr}", got, x.expect(clauses, need, masked, 10, False, 0, total_hits_threshold=thr, slicing=slicing))
            assert got.relation_gte == gte and got.total_hits > thr
    finally:
        if x is not None:
            release(x.leaves)
        c.close()


def test_a_fork_with_more_deletes_reads_the_shared_column(ix_a):
    kind, corpus = ix_a.kind, ix_a.corpus
    lives, forks = [], []
    try:
        for si, (seg, leaf) in enumerate(zip(corpus.segments, ix_a.leaves)):
            n = (seg.max_doc + 63) // 64
            live = seg.live_bits[:n] & ~synth.random_mask(seg.max_doc, 0.3, 900 + si)[:n]
            lives.append(live)
            forks.append(leaf.fork(live))
        searcher = api.GpuIndexSearcher(ix_a.searcher.ctx, forks, api.IndexStatistics.from_corpus(corpus))
        name, query, clauses, need, _ = QUERIES[2]
        for rev in (False, True):
            mb = KIND_MIN[kind]
            got = api.search_sorted64_batch(searcher, [query], [api.TopScoreDocCollectorManager(100)], [sort_field(kind, rev, mb)])[0]
            same(f"fork_{kind}_rev{int(rev)}", got, ix_a.expect(clauses, need, False, 100, rev, mb, live=lives))
            parent = api.search_sorted64_batch(ix_a.searcher, [query], [api.TopScoreDocCollectorManager(100)], [sort_field(kind, rev, mb)])[0]
            same(f"fork_parent_{kind}_rev{int(rev)}", parent, ix_a.expect(clauses, need, False, 100, rev, mb))
            assert parent.total_hits > got.total_hits
    finally:
        release(forks)


def test_device_bytes_and_store_refusals(ctx):
    g = api.GpuSegment(ctx, 2500, 0)
    try:
        before = g.device_bytes
        g.add_doc_values64(7, "long", np.arange(100, dtype=np.int64), np.arange(0, 200, 2, dtype=np.int32))
        assert g.device_bytes - before >= 8 * 2500 + 2500 // 8   # the codes and the `has` words
        before = g.device_bytes
        g.add_doc_values64(8, "double", np.zeros(2500))
        assert 8 * 2500 <= g.device_bytes - before < 8 * 2500 + 8 * 1024   # every doc has a value: no `has` words
        for fn in (lambda: g.add_doc_values64(7, "double", np.zeros(2500)), lambda: g.add_doc_values(7, "int", np.zeros(2500, dtype=np.int32)),
                   lambda: g.add_doc_values64(9, "long", np.zeros(10, dtype=np.int64))):
            with pytest.raises(_lib.NrtGpuError) as e:
                fn()
            assert e.value.code == INV
        g.seal()
        with pytest.raises(_lib.NrtGpuError) as e:
            g.add_doc_values64(10, "long", np.zeros(2500, dtype=np.int64))
        assert e.value.code == _lib.NRTGPU_ERR_STATE
    finally:
        g.release()


# ---- the two widths meet (the 32-bit entries over a 64-bit column and the other way round), the refusals of the new entries ----------
def test_refusals_on_the_device(ctx, corpus_a):
    rng = np.random.default_rng(61)
    n = [seg.max_doc for seg in corpus_a.segments]

    def more(g, si):
        g.add_doc_values(8, "int", np.arange(n[si], dtype=np.int32))
        g.add_doc_values_multi(9, "int", np.arange(n[si], dtype=np.int32), np.arange(n[si], dtype=np.int32))
        g.add_doc_values64(11, "long" if si != 1 else "double", np.zeros(n[si], dtype=np.uint64))
        wide = np.zeros(n[si], dtype=np.int64)
        wide[0], wide[1] = ref.INT64_MIN, ref.INT64_MAX
        g.add_doc_values64(12, "long", wide)

    cols = [(None, rng.choice(LONG_POOL, size=m)) for m in n]
    leaves = ref.upload(ctx, corpus_a, "long", cols, column_field=COL, more=more)
    try:
        s = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics.from_corpus(corpus_a))
        or3, ALL = QUERIES[1][1], api.DocSetQuery()
        for docset, query, entry32 in ((False, or3, "nrtgpu_search_sorted_batch"), (True, ALL, "nrtgpu_search_docset_sorted_batch")):
            for name, code, sort, says in (("no column", UNS, api.SortField64(55, "long"), "55"), ("a 32-bit column", UNS, api.SortField64(8, "long"), entry32),
                                           ("a multi-valued column", UNS, api.SortField64(9, "long"), entry32),
                                           ("kinds differ", INV, api.SortField64(11, "long"), "kinds"),
                                           ("does not fit", UNS, api.SortField64(12, "long"), "span needs 65 bits, 13-bit docids leave 51")):
                rc, rc2, text = _status(s, query, sort, docset)
                assert (rc, rc2) == (code, code) and says in text and "query 0" in text, (name, docset, rc, rc2, text)
        rc, rc2, text = _status(s, api.DocSetQuery((api.MaskFilter(77),)), api.SortField64(COL, "long"), True)
        assert (rc, rc2) == (UNS, UNS) and "77" in text
        # the 32-bit entries over the 64-bit column
        top = api.TopScoreDocCollectorManager(10)
        for fn, says in ((lambda: api.search_sorted_batch(s, [or3], [top], [api.SortField(COL, "int")]), "nrtgpu_search_sorted64_batch"),
                         (lambda: api.count_terms_batch(s, [or3], [api.TermsCollector(COL, 10)], 16), "64-bit buckets are not built"),
                         (lambda: api.search_docset_sorted_batch(s, [ALL], [top], [api.SortField(COL, "int")]), "nrtgpu_search_docset_sorted64_batch"),
                         (lambda: api.count_docset_terms_batch(s, [ALL], [api.TermsCollector(COL, 10)], 16), "64-bit buckets are not built"),
                         (lambda: api.search_docset_sorted_batch(s, [api.DocSetQuery(ranges=(api.RangeClause(COL, "int", 0, 5),))], [top], [api.SortField(8, "int")]),
                          "nrtgpu_segment_set_mask_from_values64"),
                         (lambda: leaves[0].set_mask_from_values(30, [api.ValueClause.exists(COL)]), "nrtgpu_segment_set_mask_from_values64"),
                         (lambda: leaves[0].set_mask_from_values64(30, [api.ValueClause64.exists(8)]), "nrtgpu_segment_set_mask_from_values")):
            with pytest.raises(_lib.NrtGpuError) as e:
                fn()
            assert e.value.code == UNS and says in str(e.value), str(e.value)
        assert api.sorted_supported(s, or3, top, api.SortField(COL, "int")) is False
        assert api.docset_sorted_supported(s, ALL, top, api.SortField(COL, "int")) is False
        # and the routes still answer
        got = api.search_sorted64_batch(s, [or3], [top], [api.SortField64(COL, "long")])[0]
        same("after_refusals", got, ref.search(corpus_a, ref.text_hits(corpus_a, (1, 2, 3)), cols, "long", 10))
        old = api.search_sorted_batch(s, [or3], [top], [api.SortField(8, "int")])[0]
        assert old.total_hits == got.total_hits
    finally:
        release(leaves)


@pytest.mark.parametrize("flag", [_lib.NRTGPU_FLAG_PACKED_POSTINGS, _lib.NRTGPU_FLAG_NO_FIXED_POINT])
def test_contexts_the_text_route_refuses_and_the_doc_set_route_runs_under(flag):
    corpus = fs.make_corpus([200], {1: 0.5}, seed=13)
    c = api.GpuContext(device_id=0, max_batch=16, flags=flag)
    leaves = []
    try:
        col = [(None, (EPOCH + np.arange(200, dtype=np.int64) % 7).view(np.uint64))]
        leaves = ref.upload(c, corpus, "long", col, column_field=COL)
        s = api.GpuIndexSearcher(c, leaves, api.IndexStatistics.from_corpus(corpus))
        rc, rc2, text = _status(s, T[1], api.SortField64(COL, "long"))
        assert (rc, rc2) == (UNS, UNS) and len(text) > 20
        for rev in (False, True):
            got = api.search_docset_sorted64_batch(s, [api.DocSetQuery()], [api.TopScoreDocCollectorManager(30)], [api.SortField64(COL, "long", rev)])[0]
            same(f"docset_flag{flag}_rev{int(rev)}", got, ref.search(corpus, ref.docset_hits(corpus), col, "long", 30, rev))
    finally:
        release(leaves)
        c.close()


# ---- the doc-set route ---------------------------------------------------------------------------------------------------------------
class DocsetIndex:
    """Leaves of 3000 / 1500 / 40 docs with deletes: the 64-bit sort column as in IndexA, a 32-bit column for the doc set's own range
    clauses, a filter mask whose word 3 of leaf 0 is empty, a must-not mask."""

    def __init__(self, ctx, kind, corpus):
        rng = np.random.default_rng(71 if kind == "long" else 72)
        d0 = np.nonzero(rng.random(3000) < 0.8)[0].astype(np.int32)
        self.kind, self.corpus = kind, corpus
        self.columns = [(d0, rng.choice(POOL[kind], size=len(d0))), (None, rng.choice(POOL[kind], size=1500)), None]
        self.rating = [(None, rng.integers(0, 6, size=seg.max_doc).astype(np.int32).view(np.uint32)) for seg in corpus.segments]
        self.filter = [synth.random_mask(seg.max_doc, 0.6, 300 + si) for si, seg in enumerate(corpus.segments)]
        self.filter[0] = self.filter[0].copy()
        self.filter[0][3] = 0   # a 64-doc word without an accepted doc
        self.must_not = [synth.random_mask(seg.max_doc, 0.2, 400 + si) for si, seg in enumerate(corpus.segments)]

        def more(g, si):
            g.add_doc_values(8, "int", self.rating[si][1])

        self.leaves = ref.upload(ctx, corpus, kind, self.columns, column_field=COL, more=more)
        for si, leaf in enumerate(self.leaves):
            leaf.set_mask(5, self.filter[si])
            leaf.set_mask(6, self.must_not[si])
        self.searcher = api.GpuIndexSearcher(ctx, self.leaves, api.IndexStatistics.from_corpus(corpus))


@pytest.fixture(scope="module", params=["long", "double"])
def ix_d(request, ctx, corpus_a):
    x = DocsetIndex(ctx, request.param, corpus_a)
    yield x
    release(x.leaves)


def test_doc_sets_sorted_by_a_64_bit_column(ix_d):
    kind, corpus = ix_d.kind, ix_d.corpus
    MF, R = api.MaskFilter, api.RangeClause
    shapes = [
        ("all", api.DocSetQuery(), dict()),
        ("filter", api.DocSetQuery((MF(5),)), dict(filters=[ix_d.filter])),
        ("filter_must_not", api.DocSetQuery((MF(5),), (MF(6),)), dict(filters=[ix_d.filter], must_nots=[ix_d.must_not])),
        ("range32", api.DocSetQuery(ranges=(R(8, "int", 4, 5),)), dict(ranges32=[(ix_d.rating, "int", 4, 5)])),
        ("filter_range32", api.DocSetQuery((MF(5),), (), (R(8, "int", 0, 2),)), dict(filters=[ix_d.filter], ranges32=[(ix_d.rating, "int", 0, 2)])),
    ]
    cases = [(sh, k, rev, mb) for sh in shapes for k in (1, 10, 1024) for rev in (False, True) for mb in missing_values(kind)]
    got = api.search_docset_sorted64_batch(ix_d.searcher, [sh[1] for sh, _, _, _ in cases], [api.TopScoreDocCollectorManager(k) for _, k, _, _ in cases],
                                           [sort_field(kind, rev, mb) for _, _, rev, mb in cases])
    for ((name, _, kw), k, rev, mb), td in zip(cases, got):
        same(f"docset_{kind}_{name}_k{k}_rev{int(rev)}_missing{mb:#x}", td, ref.search(corpus, ref.docset_hits(corpus, **kw), ix_d.columns, kind, k, rev, mb))
    assert api.docset_sorted64_supported(ix_d.searcher, shapes[4][1], api.TopScoreDocCollectorManager(10), sort_field(kind, True, KIND_MAX[kind])) is True


@pytest.mark.parametrize("reverse", [False, True])
def test_doc_set_pages(ix_d, reverse):
    kind, corpus = ix_d.kind, ix_d.corpus
    query, hits = api.DocSetQuery((api.MaskFilter(5),)), ref.docset_hits(corpus, filters=[ix_d.filter])
    mb = int(POOL[kind][2])
    sort = sort_field(kind, reverse, mb)
    full = api.search_docset_sorted64_batch(ix_d.searcher, [query], [api.TopScoreDocCollectorManager(70)], [sort])[0]
    same(f"docset_{kind}_page70", full, ref.search(corpus, hits, ix_d.columns, kind, 70, reverse, mb))
    after, docs, bits = None, [], []
    for page in range(10):
        got = api.search_docset_sorted64_batch(ix_d.searcher, [query], [api.TopScoreDocCollectorManager(7)], [sort], [after])[0]
        exp = ref.search(corpus, hits, ix_d.columns, kind, 7, reverse, mb, after=None if after is None else (after.doc, ref.bits_of(kind, after.value)))
        same(f"docset_{kind}_page7_{page}", got, exp)
        docs += got.docs.tolist()
        bits += got.value_bits.tolist()
        after = api.FieldDoc(int(got.docs[-1]), ref.value_of(kind, int(got.value_bits[-1])))
    assert docs == full.docs.tolist() and bits == full.value_bits.tolist()
    # the clamp trap on this route
    mb = KIND_MIN[kind]
    trap = ref.bits_of("long", ref.INT64_MIN + 5) if kind == "long" else ref.bits_of("double", -1e300)
    got = api.search_docset_sorted64_batch(ix_d.searcher, [query], [api.TopScoreDocCollectorManager(50)], [sort_field(kind, False, mb)],
                                           [api.FieldDoc(0, ref.value_of(kind, trap))])[0]
    same(f"docset_{kind}_clamp_trap", got, ref.search(corpus, hits, ix_d.columns, kind, 50, False, mb, after=(0, trap)))
    assert mb not in got.value_bits.tolist()
