"""Sort by field (nrtgpu_search_sorted_batch) through the C ABI on the device, against tests/_field_sort_ref.py.  Every
comparison is bit equality over every case: docids, ranks, the value bits each hit sorted as, total_hits, the relation.
Needs a real MI355X."""
import ctypes as C

import numpy as np
import pytest

from nrtsearch_amd import _lib, api, synth

from tests import _field_sort_ref as ref

pytestmark = pytest.mark.gpu
INT_MAX = 2**31 - 1
COL = 7   # the field id the columns live under (postings and norms: field 0)
TERMS = {1: 0.5, 2: 0.3, 3: 0.2}
T = {t: api.TermQuery(0, t) for t in (1, 2, 3, 99)}
# (name, query, clauses, clauses a hit matches at least, reads the masks)
QUERIES = [
    ("term", T[1], (1,), 1, False),
    ("or3", api.BooleanQuery((T[1], T[2], T[3])), (1, 2, 3), 1, False),
    ("msm2of3", api.BooleanQuery((T[1], T[2], T[3]), 2), (1, 2, 3), 2, False),
    ("must2", api.BooleanQuery((), 0, (), (), (T[1], T[2])), (1, 2), 2, False),
    ("masks", api.BooleanQuery((T[1], T[2], T[3]), 1, (api.MaskFilter(5),), (api.MaskFilter(6),)), (1, 2, 3), 1, True),
    ("nowhere", T[99], (99,), 1, False),
    # duplicate clauses count each: a doc with term 2 alone has 2 of these 3 clauses; terms 1 and 2 together are all 3 MUSTs
    ("msm2_dup", api.BooleanQuery((T[2], T[2], T[3]), 2), (2, 2, 3), 2, False),
    ("must3_dup", api.BooleanQuery((), 0, (), (), (T[1], T[1], T[2])), (1, 1, 2), 3, False),
]


@pytest.fixture(scope="module", autouse=True)
def two_column_postings():
    """The route refuses packed postings (tested below): these contexts keep the two-column layout also where the whole suite
    runs with NRTGPU_PACKED_POSTINGS=1, which packs every api.GpuContext."""
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
    assert got.value_bits.tolist() == bits.tolist(), f"{name}: value bits"
    assert got.total_hits == total, f"{name}: total_hits {got.total_hits}, the reference counts {total}"
    assert got.relation_gte == gte, f"{name}: relation"


def missing_values(kind):
    """the kind's minimum, its maximum, a value that also occurs"""
    return (ref.KIND_MIN[kind], ref.KIND_MAX[kind], int(ref.VALUES[kind][2]))


def sort_field(kind, reverse, missing_bits, field=COL):
    return api.SortField(field, kind, reverse, ref.value_of(kind, missing_bits))


# ---- index A: leaves of 3000, 1500 and 40 docs; the column on 80 % of leaf 0, every doc of leaf 1, absent from leaf 2 ---------
class IndexA:
    def __init__(self, ctx, kind, corpus):
        rng = np.random.default_rng(21 if kind == "int" else 22)
        d0 = np.nonzero(rng.random(3000) < 0.8)[0].astype(np.int32)
        self.kind, self.corpus = kind, corpus
        self.columns = [(d0, rng.choice(ref.VALUES[kind], size=len(d0))), (None, rng.choice(ref.VALUES[kind], size=1500)), None]
        self.masks = {(si, mid): synth.random_mask(seg.max_doc, dens, 40 * mid + si)
                      for si, seg in enumerate(corpus.segments) for mid, dens in ((5, 0.6), (6, 0.2))}
        self.accept = [synth.accept_words(seg, self.masks[(si, 5)], self.masks[(si, 6)]) for si, seg in enumerate(corpus.segments)]
        self.leaves = ref.upload(ctx, corpus, kind, self.columns, column_field=COL)
        for (si, mid), bits in self.masks.items():
            self.leaves[si].set_mask(mid, bits)
        self.searcher = api.GpuIndexSearcher(ctx, self.leaves, api.IndexStatistics.from_corpus(corpus))

    def expect(self, clauses, need, masked, k, reverse, missing_bits, **kw):
        return ref.search(self.corpus, self.columns, self.kind, clauses, k, reverse, missing_bits, need,
                          accept=self.accept if masked else None, **kw)


@pytest.fixture(scope="module")
def corpus_a():
    c = ref.make_corpus([3000, 1500, 40], TERMS, seed=5, delete_fraction=0.01)
    assert all(seg.live_bits is not None for seg in c.segments)
    return c


@pytest.fixture(scope="module", params=["int", "float"])
def ix_a(request, ctx, corpus_a):
    x = IndexA(ctx, request.param, corpus_a)
    yield x
    release(x.leaves)


def test_every_query_shape_direction_missing_value_and_k(ix_a):
    kind = ix_a.kind
    cases = [(q, k, rev, mb) for q in QUERIES for k in (1, 10, 1024) for rev in (False, True) for mb in missing_values(kind)]
    mgrs = [api.TopScoreDocCollectorManager(k) for _, k, _, _ in cases]
    got = api.search_sorted_batch(ix_a.searcher, [q[1] for q, _, _, _ in cases], mgrs, [sort_field(kind, rev, mb) for _, _, rev, mb in cases])
    d = api.GpuContext.last_diagnostics()
    assert d["items_maxscore"] == 0 and d["items_scan"] >= len(cases) * 5 // 6
    full_pages = 0
    for ((name, _, clauses, need, masked), k, rev, mb), td in zip(cases, got):
        exp = ix_a.expect(clauses, need, masked, k, rev, mb)
        same(f"{kind}_{name}_k{k}_rev{int(rev)}_missing{mb:#x}", td, exp)
        assert (exp[2] == 0) == (name == "nowhere")
        full_pages += int(k == 1024 and exp[2] > 1024)
    assert full_pages >= 10   # (k = 1024 pages that are full: the hits ranked, not just listed)
    for q, k, rev, mb in cases[:: len(cases) // 6]:
        assert api.sorted_supported(ix_a.searcher, q[1], api.TopScoreDocCollectorManager(k), sort_field(kind, rev, mb)) is True


@pytest.mark.parametrize("reverse", [False, True])
def test_pages_through_after_equal_one_long_page(ix_a, reverse):
    kind = ix_a.kind
    name, query, clauses, need, masked = QUERIES[1]
    mb = int(ref.VALUES[kind][2])
    sort = sort_field(kind, reverse, mb)
    full = api.search_sorted_batch(ix_a.searcher, [query], [api.TopScoreDocCollectorManager(70)], [sort])[0]
    same(f"{kind}_page70", full, ix_a.expect(clauses, need, masked, 70, reverse, mb))
    after, docs, bits, cut_in_a_run = None, [], [], 0
    for page in range(10):
        got = api.search_sorted_batch(ix_a.searcher, [query], [api.TopScoreDocCollectorManager(7)], [sort], [after])[0]
        exp = ix_a.expect(clauses, need, masked, 7, reverse, mb,
                          after=None if after is None else (after.doc, ref.bits_of(kind, after.value)))
        same(f"{kind}_page7_{page}", got, exp)
        assert got.total_hits == full.total_hits
        if bits:
            cut_in_a_run += int(bits[-1] == int(got.value_bits[0]))
        docs += got.docs.tolist()
        bits += got.value_bits.tolist()
        after = api.FieldDoc(int(got.docs[-1]), ref.value_of(kind, int(got.value_bits[-1])))
    assert docs == full.docs.tolist() and bits == full.value_bits.tolist()
    assert cut_in_a_run >= 1   # a cursor inside a run of equal values: the docid decides


def test_counts_and_relation_equal_the_function_score_route(ix_a):
    """Pure disjunctions: total_hits and the relation are what nrtgpu_search_function_score_batch with no function reports."""
    kind = ix_a.kind
    for name, query, clauses, need, masked in QUERIES[:2]:
        for k, thr in ((1, 1000), (10, 1000), (1024, 1000), (10, 5000), (10, 0)):
            mgr = api.TopScoreDocCollectorManager(k, None, thr)
            got = api.search_sorted_batch(ix_a.searcher, [query], [mgr], [sort_field(kind, False, ref.KIND_MAX[kind])])[0]
            fs = ix_a.searcher.search_function_score_batch([api.FunctionScoreQuery(query)], [mgr])[0]
            assert (got.total_hits, got.relation_gte) == (fs.total_hits, fs.relation_gte), (name, k, thr)
            same(f"{kind}_{name}_thr{thr}", got, ix_a.expect(clauses, need, masked, k, False, ref.KIND_MAX[kind], total_hits_threshold=thr))


def test_relation_per_slice(corpus_a):
    c = api.GpuContext(device_id=0, max_batch=16)
    x = None
    try:
        c.set_slicing(1000, 5, 1)
        slicing = (1000, 5, 1)
        x = IndexA(c, "int", corpus_a)
        name, query, clauses, need, masked = QUERIES[0]
        info = {}
        x.expect(clauses, need, masked, 10, False, 0, total_hits_threshold=50, slicing=slicing, info=info)
        per_slice = info["slice_hits"]
        assert len(per_slice) == 3 and max(per_slice) > 50 and min(per_slice) <= 50
        # 50: some slice passes it; the largest slice's count: total_hits exceeds it, no slice does -- EQUAL_TO
        for thr, gte in ((50, True), (max(per_slice), False)):
            got = api.search_sorted_batch(x.searcher, [query], [api.TopScoreDocCollectorManager(10, None, thr)], [sort_field("int", False, 0)])[0]
            same(f"slices_thr{thr}", got, x.expect(clauses, need, masked, 10, False, 0, total_hits_threshold=thr, slicing=slicing))
            assert got.relation_gte == gte and got.total_hits > thr
    finally:
        if x is not None:
            release(x.leaves)
        c.close()


# ---- index B: 13 000 docs, a term in 60 % of them: the first round's hits overflow the candidate buffer ----------------------
def test_wave_by_wave_compaction(ctx):
    corpus = ref.make_corpus([13_000], {1: 0.6}, seed=8)
    seg = corpus.segments[0]
    assert int((seg.postings(1)[0] < 12 * 1024).sum()) > 3072   # kScanWaves sub-tiles hold more hits than kFsCandCap
    perm = np.random.default_rng(9).permutation(13_000).astype(np.int32)
    g = api.GpuSegment(ctx, seg.max_doc, 0)
    try:
        g.add_field_norms(0, seg.norms)
        g.add_terms(0, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
        g.add_doc_values(7, "int", perm)                                       # no ties
        g.add_doc_values(8, "int", np.full(13_000, 42, dtype=np.int32))        # all ties
        g.seal()
        searcher = api.GpuIndexSearcher(ctx, [g], api.IndexStatistics.from_corpus(corpus))
        columns = {7: [(None, perm.view(np.uint32))], 8: [(None, np.full(13_000, 42, dtype=np.uint32))]}
        cases = [(f, k, rev) for f in (7, 8) for k in (10, 1024) for rev in (False, True)]
        got = api.search_sorted_batch(searcher, [T[1]] * len(cases), [api.TopScoreDocCollectorManager(k, None, INT_MAX) for _, k, _ in cases],
                                      [api.SortField(f, "int", rev, 0) for f, _, rev in cases])
        for (f, k, rev), td in zip(cases, got):
            exp = ref.search(corpus, columns[f], "int", (1,), k, rev, 0, total_hits_threshold=INT_MAX)
            assert exp[2] > 7000 and len(exp[0]) == k
            same(f"compaction_field{f}_k{k}_rev{int(rev)}", td, exp)
            if f == 8:
                assert td.docs.tolist() == sorted(td.docs.tolist())   # all ties: the first k docs, in both directions
    finally:
        g.release()


# ---- index C: one query cut into several items; the last item holds every winner ------------------------------------------
def test_several_items_share_theta(ctx):
    n = 300_000
    corpus = ref.make_corpus([n], {1: 1.0}, seed=10)
    seg = corpus.segments[0]
    values = (n - np.arange(n)).astype(np.int32)   # ascending sort: the winners are the LAST docs
    g = api.GpuSegment(ctx, n, 0)
    try:
        g.add_field_norms(0, seg.norms)
        g.add_terms(0, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
        g.add_doc_values(COL, "int", values)
        g.seal()
        searcher = api.GpuIndexSearcher(ctx, [g], api.IndexStatistics.from_corpus(corpus))
        columns = [(None, values.view(np.uint32))]
        for k, rev in ((10, False), (1024, False), (10, True)):
            got = api.search_sorted_batch(searcher, [T[1]], [api.TopScoreDocCollectorManager(k)], [api.SortField(COL, "int", rev, 0)])[0]
            assert api.GpuContext.last_diagnostics()["items_scan"] >= 2
            same(f"items_k{k}_rev{int(rev)}", got, ref.search(corpus, columns, "int", (1,), k, rev, 0))
            if not rev:
                assert got.docs.tolist() == list(range(n - 1, n - 1 - k, -1)) and got.total_hits == n
    finally:
        g.release()


# ---- refusals and lifecycle ----------------------------------------------------------------------------------------------------
def _raw(searcher, query, mgr, sort, after=None, **fields):
    """nrtgpu_search_sorted_batch's status for one query with fields of its nrtgpu_field_sort overwritten."""
    m, fs = api._marshal_sorted(searcher, [query], [mgr], [sort], [after])
    for name, v in fields.items():
        setattr(fs[0], name, v)
    h = api._text_outputs(1, [mgr])
    rc = _lib.load().nrtgpu_search_sorted_batch(searcher.ctx._h, searcher._segs, searcher._bases, len(searcher.leaves), m.queries, fs, 1,
                                               C.cast(h.outs, C.POINTER(_lib.FieldDocs)))
    rc2 = _lib.load().nrtgpu_sorted_supported(searcher.ctx._h, searcher._segs, len(searcher.leaves), m.queries, fs)
    assert rc2 == rc, "the predicate and the search disagree"
    return rc, _lib.load().nrtgpu_last_error().decode()


def test_search_refusals(ix_a):
    kind, s = ix_a.kind, ix_a.searcher
    sort = sort_field(kind, False, 0)
    mgr = api.TopScoreDocCollectorManager(10)
    inv, uns = _lib.NRTGPU_ERR_INVALID_ARG, _lib.NRTGPU_ERR_UNSUPPORTED
    or3 = QUERIES[1][1]
    refusals = [
        ("reverse 2", inv, or3, mgr, sort, dict(reverse=2)),
        ("reverse -1", inv, or3, mgr, sort, dict(reverse=-1)),
        ("has_after 2", inv, or3, mgr, sort, dict(has_after=2)),
        ("after_doc < 0", inv, or3, mgr, sort, dict(has_after=1, after_doc=-1)),
        ("the query's has_after", inv, or3, api.TopScoreDocCollectorManager(10, api.ScoreDoc(3, 1.0)), sort, {}),
        ("numHits 0", inv, or3, api.TopScoreDocCollectorManager(0), sort, {}),
        ("no column on any leaf", uns, or3, mgr, sort_field(kind, False, 0, field=55), {}),
        ("dismax", uns, api.DisjunctionMaxQuery((T[1], T[2])), mgr, sort, {}),
        ("dismax with a tie breaker", uns, api.DisjunctionMaxQuery((T[1], T[2]), 0.3), mgr, sort, {}),
        ("MUST next to SHOULD", uns, api.BooleanQuery((T[2],), 0, (), (), (T[1],)), mgr, sort, {}),
        ("min_competitive_score", uns, or3, api.TopScoreDocCollectorManager(10, None, 1000, 0.5), sort, {}),
        ("numHits 2000", uns, or3, api.TopScoreDocCollectorManager(2000), sort, {}),
        ("a mask that is not resident", uns, api.BooleanQuery((T[1],), 1, (api.MaskFilter(77),)), mgr, sort, {}),
        ("a must_not mask that is not resident", uns, api.BooleanQuery((T[1],), 1, (), (api.MaskFilter(78),)), mgr, sort, {}),
    ]
    for name, code, query, m, so, fields in refusals:
        rc, text = _raw(s, query, m, so, **fields)
        assert rc == code, f"{name}: status {rc}: {text}"
        assert "query 0" in text, f"{name}: {text}"
    # the fixed-point analysis of the final-score routes (final_score_plan), kept as it is: clauses weighted 1 and 2^-20 span more
    # binades than the common scale takes.  The search and the predicate agree (_raw); the reason speaks of the batch, not of a
    # query: a batch in which ONE query fails the analysis is refused whole, wherever that query stands.
    wide = api.BooleanQuery((T[1], api.BoostQuery(T[2], 2.0 ** -20)))
    rc, text = _raw(s, wide, mgr, sort)
    assert rc == uns and "fixed-point" in text and "binades" in text, f"status {rc}: {text}"
    assert api.sorted_supported(s, wide, mgr, sort) is False
    for batch in ([or3, T[1], wide], [wide, or3], [or3, wide, T[1]]):
        assert all(api.sorted_supported(s, q, mgr, sort) is (q is not wide) for q in batch)
        with pytest.raises(_lib.NrtGpuError) as e:
            api.search_sorted_batch(s, batch, [mgr] * len(batch), [sort] * len(batch))
        assert e.value.code == uns and "fixed-point" in str(e.value), str(e.value)
    # the binding raises, and says unsupported where it is
    with pytest.raises(_lib.NrtGpuError) as e:
        api.search_sorted_batch(s, [or3], [mgr], [sort_field(kind, False, 0, field=55)])
    assert e.value.code == uns and "55" in str(e.value)
    assert api.sorted_supported(s, or3, mgr, sort_field(kind, False, 0, field=55)) is False
    with pytest.raises(_lib.NrtGpuError):
        api.sorted_supported(s, or3, api.TopScoreDocCollectorManager(0), sort)
    # NULL arguments with a context
    q, f, o = _lib.Bm25Query(), _lib.FieldSort(), _lib.FieldDocs()
    L = _lib.load()
    assert L.nrtgpu_search_sorted_batch(s.ctx._h, s._segs, s._bases, 3, None, C.byref(f), 1, C.byref(o)) == inv
    assert L.nrtgpu_search_sorted_batch(s.ctx._h, s._segs, s._bases, 3, C.byref(q), None, 1, C.byref(o)) == inv
    assert L.nrtgpu_search_sorted_batch(s.ctx._h, s._segs, s._bases, 3, C.byref(q), C.byref(f), 1, None) == inv
    assert L.nrtgpu_sorted_supported(s.ctx._h, s._segs, 3, None, C.byref(f)) == inv
    # and the route still answers
    got = api.search_sorted_batch(s, [or3], [mgr], [sort])[0]
    same("after_refusals", got, ix_a.expect((1, 2, 3), 1, False, 10, False, 0))


def test_leaves_that_disagree_on_the_kind(ctx, corpus_a):
    rng = np.random.default_rng(31)
    leaves = []
    try:
        for seg, kind in zip(corpus_a.segments, ("int", "float", "int")):
            g = api.GpuSegment(ctx, seg.max_doc, seg.doc_base)
            leaves.append(g)
            g.add_field_norms(0, seg.norms)
            g.add_terms(0, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
            g.add_doc_values(COL, kind, rng.choice(ref.VALUES[kind], size=seg.max_doc))
            g.seal()
        s = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics.from_corpus(corpus_a))
        rc, text = _raw(s, T[1], api.TopScoreDocCollectorManager(10), api.SortField(COL, "int"))
        assert rc == _lib.NRTGPU_ERR_INVALID_ARG and "kinds" in text and "query 0" in text
    finally:
        release(leaves)


@pytest.mark.parametrize("flag", [_lib.NRTGPU_FLAG_PACKED_POSTINGS, _lib.NRTGPU_FLAG_NO_FIXED_POINT])
def test_contexts_the_route_refuses(flag):
    corpus = ref.make_corpus([200], {1: 0.5}, seed=13)
    c = api.GpuContext(device_id=0, max_batch=16, flags=flag)
    leaves = []
    try:
        leaves = ref.upload(c, corpus, "int", [(None, np.arange(200, dtype=np.uint32))], column_field=COL)
        s = api.GpuIndexSearcher(c, leaves, api.IndexStatistics.from_corpus(corpus))
        rc, text = _raw(s, T[1], api.TopScoreDocCollectorManager(10), api.SortField(COL, "int"))
        assert rc == _lib.NRTGPU_ERR_UNSUPPORTED and len(text) > 20
        assert api.sorted_supported(s, T[1], api.TopScoreDocCollectorManager(10), api.SortField(COL, "int")) is False
        assert s.search_batch([T[1]], [api.TopScoreDocCollectorManager(10)])[0].total_hits == len(corpus.segments[0].postings(1)[0])
    finally:
        release(leaves)
        c.close()


def test_segment_store_refusals_and_device_bytes(ctx):
    L = _lib.load()
    inv, state = _lib.NRTGPU_ERR_INVALID_ARG, _lib.NRTGPU_ERR_STATE
    max_doc = 2500
    g = api.GpuSegment(ctx, max_doc, 0)
    try:
        v = np.arange(max_doc, dtype=np.int32)
        docs = np.arange(0, 2 * 100, 2, dtype=np.int32)

        def add(field, kind, n, d, vals):
            return L.nrtgpu_segment_add_doc_values(g._h, field, kind, n, None if d is None else d.ctypes.data, None if vals is None else vals.ctypes.data)

        assert add(7, 2, max_doc, None, v) == inv and add(7, -1, max_doc, None, v) == inv
        assert add(7, 0, -1, None, v) == inv
        assert add(7, 0, max_doc + 1, None, np.arange(max_doc + 1, dtype=np.int32)) == inv
        assert add(7, 0, 100, None, v) == inv                                   # docs == NULL with n != max_doc
        assert add(7, 0, 100, docs, None) == inv                                # values == NULL with n > 0
        for bad in (docs[::-1].copy(), np.where(docs == 20, 18, docs).astype(np.int32), np.where(docs == 198, max_doc, docs).astype(np.int32),
                    np.where(docs == 0, -1, docs).astype(np.int32)):
            assert add(7, 0, 100, bad, v) == inv, bad[:12]
        before = g.device_bytes
        assert add(7, 0, 100, docs, v) == _lib.NRTGPU_OK
        assert g.device_bytes - before >= 4 * max_doc
        assert add(7, 1, max_doc, None, v) == inv and b"already" in L.nrtgpu_last_error()   # a second column on the field
        before = g.device_bytes
        g.add_doc_values(8, "float", np.zeros(max_doc, dtype=np.float32))        # another field id: its own column
        assert g.device_bytes - before >= 4 * max_doc
        assert add(9, 0, 0, None, None) == inv and add(9, 0, 0, docs, None) == _lib.NRTGPU_OK   # no doc has a value: every doc sorts as missing
        g.seal()
        assert add(10, 0, max_doc, None, v) == state
    finally:
        g.release()


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
            mb = ref.KIND_MIN[kind]
            got = api.search_sorted_batch(searcher, [query], [api.TopScoreDocCollectorManager(100)], [sort_field(kind, rev, mb)])[0]
            exp = ref.search(corpus, ix_a.columns, kind, clauses, 100, rev, mb, need, live=lives)
            same(f"fork_{kind}_rev{int(rev)}", got, exp)
            parent = api.search_sorted_batch(ix_a.searcher, [query], [api.TopScoreDocCollectorManager(100)], [sort_field(kind, rev, mb)])[0]
            same(f"fork_parent_{kind}_rev{int(rev)}", parent, ix_a.expect(clauses, need, False, 100, rev, mb))
            assert parent.total_hits > got.total_hits
    finally:
        release(forks)
