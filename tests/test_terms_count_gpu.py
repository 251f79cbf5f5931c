"""The terms aggregation (nrtgpu_count_terms_batch) through the C ABI on the device, against tests/_terms_count_ref.py.  Every
comparison is exact equality of (value_bits, counts, n_buckets, total_hits, hits_with_value, overflowed).  Needs a real MI355X."""
import ctypes as C

import numpy as np
import pytest

from nrtsearch_amd import _lib, api, synth

from tests import _field_sort_ref as fs
from tests import _terms_count_ref as ref

pytestmark = pytest.mark.gpu
TERMS = {1: 0.5, 2: 0.3, 3: 0.2}
T = {t: api.TermQuery(0, t) for t in (1, 2, 3, 99)}
# the sort tests' eight shapes: (name, query, clauses, clauses a hit matches at least, reads the masks)
QUERIES = [
    ("term", T[1], (1,), 1, False),
    ("or3", api.BooleanQuery((T[1], T[2], T[3])), (1, 2, 3), 1, False),
    ("msm2of3", api.BooleanQuery((T[1], T[2], T[3]), 2), (1, 2, 3), 2, False),
    ("must2", api.BooleanQuery((), 0, (), (), (T[1], T[2])), (1, 2), 2, False),
    ("masks", api.BooleanQuery((T[1], T[2], T[3]), 1, (api.MaskFilter(5),), (api.MaskFilter(6),)), (1, 2, 3), 1, True),
    ("nowhere", T[99], (99,), 1, False),
    ("msm2_dup", api.BooleanQuery((T[2], T[2], T[3]), 2), (2, 2, 3), 2, False),
    ("must3_dup", api.BooleanQuery((), 0, (), (), (T[1], T[1], T[2])), (1, 1, 2), 3, False),
]
NAN_PAYLOADS = np.array([0x7FC00000, 0x7FC00001, 0xFFC12345], dtype=np.uint32)


def _f(values) -> np.ndarray:
    return np.asarray(values, dtype=np.float32).view(np.uint32)


def _i(values) -> np.ndarray:
    return np.asarray(values, dtype=np.int64).astype(np.int32).view(np.uint32)


# (kind, name) -> the pool of value bits a column draws from
POOLS = {
    ("int", "const"): _i([42]),
    ("int", "two"): _i([-7, 9]),
    ("int", "five"): _i([3, 1, 4, 15, 9]),
    ("int", "many"): _i(np.arange(700) * 37 - 9000),
    ("int", "edge"): _i([fs.INT32_MIN, -1, 0, 1, fs.INT32_MAX]),
    # codes that agree in their low 8, 16 and 20 bits
    ("int", "strided"): _i(np.concatenate([np.arange(-20, 20) << 8, np.arange(-20, 20) << 16, np.arange(-20, 20) << 20])),
    ("float", "const"): _f([2.5]),
    ("float", "two"): _f([-1.0, 1.0]),
    ("float", "five"): _f([0.5, 1.0, 2.0, 4.5, -3.0]),
    ("float", "many"): _f(np.arange(700) * 0.25 - 60.0),
    ("float", "edge"): np.concatenate([_f([-np.inf, -0.0, 0.0, 1e-45, np.inf]), NAN_PAYLOADS]),
    ("float", "strided"): np.concatenate([np.arange(1, 41, dtype=np.uint32) << 8, np.arange(1, 41, dtype=np.uint32) << 16,
                                          np.arange(1, 41, dtype=np.uint32) << 20]).astype(np.uint32),
}
FIELD = {key: 10 + i for i, key in enumerate(POOLS)}


@pytest.fixture(scope="module", autouse=True)
def two_column_postings():
    """The route refuses packed postings (tested below): these contexts keep the two-column layout also where the whole suite
    runs with NRTGPU_PACKED_POSTINGS=1."""
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
    bits, counts, n, total, valued, over = exp
    assert got.total_hits == total, f"{name}: total_hits {got.total_hits}, the reference counts {total}"
    assert int(got.overflowed) == over, f"{name}: overflowed {got.overflowed}"
    assert len(got.counts) == n and len(got.values) == n, f"{name}: {len(got.counts)} buckets, the reference has {n}"
    assert got.value_bits.tolist() == bits.tolist(), f"{name}: value bits"
    assert got.counts.tolist() == counts.tolist(), f"{name}: counts"
    assert got.hits_with_value == valued, f"{name}: hits_with_value {got.hits_with_value}, the reference has {valued}"


# ---- index A: the sort tests' leaves of 3000, 1500 and 40 docs, 1 % deletes; every column on 80 % of leaf 0, all of leaf 1, absent
# ---- from leaf 2; one upload holds all twelve columns under their own field ids
class IndexA:
    def __init__(self, ctx, corpus):
        rng = np.random.default_rng(41)
        self.corpus = corpus
        self.columns = {}
        for key, pool in POOLS.items():
            d0 = np.nonzero(rng.random(3000) < 0.8)[0].astype(np.int32)
            self.columns[key] = [(d0, rng.choice(pool, size=len(d0))), (None, rng.choice(pool, size=1500)), None]
        self.masks = {(si, mid): synth.random_mask(seg.max_doc, dens, 40 * mid + si)
                      for si, seg in enumerate(corpus.segments) for mid, dens in ((5, 0.6), (6, 0.2))}
        self.accept = [synth.accept_words(seg, self.masks[(si, 5)], self.masks[(si, 6)]) for si, seg in enumerate(corpus.segments)]
        self.leaves = []
        for si, seg in enumerate(corpus.segments):
            g = api.GpuSegment(ctx, seg.max_doc, seg.doc_base)
            g.add_field_norms(0, seg.norms)
            g.add_terms(0, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
            for key, cols in self.columns.items():
                if cols[si] is not None:
                    g.add_doc_values(FIELD[key], key[0], np.asarray(cols[si][1], dtype=np.uint32), cols[si][0])
            g.seal()
            g.set_live_docs(seg.live_bits)
            self.leaves.append(g)
        for (si, mid), bits in self.masks.items():
            self.leaves[si].set_mask(mid, bits)
        self.searcher = api.GpuIndexSearcher(ctx, self.leaves, api.IndexStatistics.from_corpus(corpus))

    def expect(self, key, clauses, need, masked, max_buckets, **kw):
        return ref.count(self.corpus, self.columns[key], key[0], clauses, need, max_buckets, accept=self.accept if masked else None, **kw)

    def collector(self, key):
        return api.TermsCollector(FIELD[key], 10, True, key[0])


@pytest.fixture(scope="module")
def ix(ctx):
    corpus = fs.make_corpus([3000, 1500, 40], TERMS, seed=5, delete_fraction=0.01)
    assert all(seg.live_bits is not None for seg in corpus.segments)
    x = IndexA(ctx, corpus)
    yield x
    release(x.leaves)


@pytest.mark.parametrize("kind", ["int", "float"])
def test_every_query_shape_over_every_column(ix, kind):
    keys = [k for k in POOLS if k[0] == kind]
    cases = [(key, q) for key in keys for q in QUERIES]
    before = ix.searcher.ctx.stats()
    got = api.count_terms_batch(ix.searcher, [q[1] for _, q in cases], [ix.collector(key) for key, _ in cases], 1024)
    d = api.GpuContext.last_diagnostics()
    after = ix.searcher.ctx.stats()
    assert d["items_maxscore"] == 0 and d["items_scan"] >= len(cases) * 5 // 8
    assert after["scan_launches"] == before["scan_launches"] + 1 and after["fixed_point_launches"] == before["fixed_point_launches"] + 1
    assert after["maxscore_launches"] == before["maxscore_launches"] and after["scan_items"] == before["scan_items"] + d["items_scan"]
    seen = set()
    for (key, (name, _, clauses, need, masked)), tc in zip(cases, got):
        exp = ix.expect(key, clauses, need, masked, 1024)
        same(f"{key}_{name}", tc, exp)
        assert exp[5] == 0 and (exp[3] == 0) == (name == "nowhere")
        assert exp[4] < exp[3] or name == "nowhere"   # some hit lacks a value (leaf 2, 20 % of leaf 0)
        seen.add((key[1], exp[2]))
    assert ("const", 1) in seen and ("two", 2) in seen and ("five", 5) in seen and max(n for name, n in seen if name == "many") > 600
    if kind == "float":   # three NaN payloads: one bucket, reported canonical and last; the zeros: two buckets
        bits = got[keys.index(("float", "edge")) * len(QUERIES) + 1].value_bits.tolist()
        assert bits == _f([-np.inf, -0.0, 0.0, 1e-45, np.inf]).tolist() + [0x7FC00000]
    else:
        assert got[keys.index(("int", "edge")) * len(QUERIES) + 1].values.tolist() == [fs.INT32_MIN, -1, 0, 1, fs.INT32_MAX]
    assert api.count_terms_supported(ix.searcher, QUERIES[2][1], ix.collector(keys[0]), 1024) is True


def test_the_overflow_boundary(ix):
    cases = []
    for kind in ("int", "float"):
        for name in ("const", "two", "many"):
            key = (kind, name)
            for qname, query, clauses, need, masked in (QUERIES[1], QUERIES[4]):
                distinct = ix.expect(key, clauses, need, masked, 65536)[2]
                assert distinct == {"const": 1, "two": 2}.get(name, distinct) and (name != "many" or distinct > 600)
                cases += [(key, query, clauses, need, masked, b) for b in (distinct, distinct - 1, distinct + 1) if b >= 1]
    got = api.count_terms_batch(ix.searcher, [c[1] for c in cases], [ix.collector(c[0]) for c in cases], [c[5] for c in cases])
    overflowed = 0
    for (key, _, clauses, need, masked, b), tc in zip(cases, got):
        exp = ix.expect(key, clauses, need, masked, b)
        same(f"{key}_max_buckets_{b}", tc, exp)
        overflowed += exp[5]
    assert overflowed == 8 and len(cases) == 32   # max_buckets one below the distinct count, wherever that is >= 1, overflows


# ---- index B: 13 000 docs, a term in 60 % of them, over a permutation column: ~7800 distinct values in ONE item, more than the
# ---- workgroup's table takes within its probe bound -- values go straight to the global table
@pytest.fixture(scope="module")
def ix_b(ctx):
    corpus = fs.make_corpus([13_000], {1: 0.6, 2: 0.01}, seed=8)
    seg = corpus.segments[0]
    perm = np.random.default_rng(9).permutation(13_000).astype(np.int32)
    g = api.GpuSegment(ctx, seg.max_doc, 0)
    g.add_field_norms(0, seg.norms)
    g.add_terms(0, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
    g.add_doc_values(7, "int", perm)
    g.add_doc_values(8, "int", np.full(13_000, 42, dtype=np.int32))
    g.seal()
    searcher = api.GpuIndexSearcher(ctx, [g], api.IndexStatistics.from_corpus(corpus))
    columns = {7: [(None, perm.view(np.uint32))], 8: [(None, np.full(13_000, 42, dtype=np.uint32))]}
    yield corpus, searcher, columns
    g.release()


def test_more_distinct_values_than_the_workgroup_table_takes(ix_b):
    corpus, searcher, columns = ix_b
    exp = ref.count(corpus, columns[7], "int", (1,), 1, 8192)
    assert 7500 < exp[2] <= 8192 and exp[5] == 0 and exp[1].max() == 1
    got = api.count_terms_batch(searcher, [T[1]], [api.TermsCollector(7, 10)], 8192)[0]
    assert api.GpuContext.last_diagnostics()["items_scan"] == 1
    same("permutation_8192", got, exp)


def test_the_global_probe_bound(ix_b):
    """max_buckets 4: a table of 8 slots under ~7800 distinct values -- the probe runs its whole bound and the flag is raised;
    alone, and as one query of a batch whose other queries stay exact."""
    corpus, searcher, columns = ix_b
    got = api.count_terms_batch(searcher, [T[1]], [api.TermsCollector(7, 10)], 4)[0]
    same("permutation_4", got, ref.count(corpus, columns[7], "int", (1,), 1, 4))
    assert got.overflowed and got.hits_with_value == -1 and got.total_hits > 7500
    cases = [(7, 1, 8192), (7, 1, 4), (8, 1, 4), (7, 2, 256), (7, 1, 1), (8, 1, 1), (7, 1, 8192), (7, 2, 64)]
    got = api.count_terms_batch(searcher, [T[t] for _, t, _ in cases], [api.TermsCollector(f, 10) for f, _, _ in cases], [b for _, _, b in cases])
    for (f, t, b), tc in zip(cases, got):
        same(f"batch_field{f}_term{t}_max_buckets_{b}", tc, ref.count(corpus, columns[f], "int", (t,), 1, b))
    assert [int(tc.overflowed) for tc in got] == [0, 1, 0, 0, 1, 0, 0, 1]


# ---- index C: one query cut into several items: the counts of one value arrive from more than one workgroup ---------------------
def test_several_items_share_the_query_table(ctx):
    n = 300_000
    corpus = fs.make_corpus([n], {1: 1.0}, seed=10)
    seg = corpus.segments[0]
    mod5 = (np.arange(n) % 5).astype(np.int32)
    every = np.arange(n, dtype=np.int32)
    g = api.GpuSegment(ctx, n, 0)
    try:
        g.add_field_norms(0, seg.norms)
        g.add_terms(0, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
        g.add_doc_values(7, "int", mod5)
        g.add_doc_values(8, "int", every)
        g.seal()
        searcher = api.GpuIndexSearcher(ctx, [g], api.IndexStatistics.from_corpus(corpus))
        got = api.count_terms_batch(searcher, [T[1], T[1]], [api.TermsCollector(7, 10), api.TermsCollector(8, 10)], [16, 65536])
        assert api.GpuContext.last_diagnostics()["items_scan"] >= 4
        same("mod5", got[0], ref.count(corpus, [(None, mod5.view(np.uint32))], "int", (1,), 1, 16))
        assert got[0].counts.tolist() == [n // 5] * 5 and got[0].total_hits == n
        # 300 000 distinct values under the largest bound: overflowed, the count still exact
        same("every_doc_its_own_value", got[1], ref.count(corpus, [(None, every.view(np.uint32))], "int", (1,), 1, 65536))
        assert got[1].overflowed and got[1].total_hits == n
    finally:
        g.release()


def test_a_batch_of_64_mixes_fields_kinds_and_bounds(ix):
    rng = np.random.default_rng(77)
    keys = list(POOLS)
    cases = []
    for i in range(64):
        key = keys[int(rng.integers(len(keys)))]
        q = QUERIES[int(rng.integers(len(QUERIES)))]
        cases.append((key, q, int(rng.choice([1, 2, 5, 100, 699, 1024, 65536]))))
    assert {c[0][0] for c in cases} == {"int", "float"}
    got = api.count_terms_batch(ix.searcher, [q[1] for _, q, _ in cases], [ix.collector(key) for key, _, _ in cases], [b for _, _, b in cases])
    overflowed = 0
    for (key, (name, _, clauses, need, masked), b), tc in zip(cases, got):
        exp = ix.expect(key, clauses, need, masked, b)
        same(f"mixed_{key}_{name}_{b}", tc, exp)
        overflowed += exp[5]
    assert 5 <= overflowed <= 50


def test_total_hits_equal_the_sorted_route(ix):
    key = ("int", "five")
    mgrs = [api.TopScoreDocCollectorManager(10)] * len(QUERIES)
    counted = api.count_terms_batch(ix.searcher, [q[1] for q in QUERIES], [ix.collector(key)] * len(QUERIES), 16)
    ranked = api.search_sorted_batch(ix.searcher, [q[1] for q in QUERIES], mgrs, [api.SortField(FIELD[key], "int")] * len(QUERIES))
    assert [c.total_hits for c in counted] == [r.total_hits for r in ranked]
    assert sum(c.total_hits for c in counted) > 5000


def test_a_fork_with_more_deletes_reads_the_shared_column(ix):
    corpus = ix.corpus
    lives, forks = [], []
    try:
        for si, (seg, leaf) in enumerate(zip(corpus.segments, ix.leaves)):
            n = (seg.max_doc + 63) // 64
            live = seg.live_bits[:n] & ~synth.random_mask(seg.max_doc, 0.3, 900 + si)[:n]
            lives.append(live)
            forks.append(leaf.fork(live))
        searcher = api.GpuIndexSearcher(ix.searcher.ctx, forks, api.IndexStatistics.from_corpus(corpus))
        name, query, clauses, need, _ = QUERIES[2]
        for key in (("int", "many"), ("float", "edge")):
            got = api.count_terms_batch(searcher, [query], [ix.collector(key)], 1024)[0]
            same(f"fork_{key}", got, ref.count(corpus, ix.columns[key], key[0], clauses, need, 1024, live=lives))
            parent = api.count_terms_batch(ix.searcher, [query], [ix.collector(key)], 1024)[0]
            same(f"fork_parent_{key}", parent, ix.expect(key, clauses, need, False, 1024))
            assert parent.total_hits > got.total_hits and parent.hits_with_value > got.hits_with_value
    finally:
        release(forks)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def _raw(searcher, query, collector, max_buckets, mgr=None, capacity=None, null_arrays=False):
    """nrtgpu_count_terms_batch's status for one query; the predicate must agree (it has no output to judge: not for `capacity`)."""
    m, tc, _ = api._marshal_terms(searcher, [query], [collector], max_buckets, None if mgr is None else [mgr])
    cap = max(max_buckets, 1) if capacity is None else capacity
    bits, counts = np.zeros(max(cap, 1), np.uint32), np.zeros(max(cap, 1), np.int32)
    out = _lib.TermCounts()
    out.capacity = cap
    if not null_arrays:
        out.value_bits = C.cast(bits.ctypes.data, C.POINTER(C.c_uint32))
        out.counts = C.cast(counts.ctypes.data, C.POINTER(C.c_int32))
    L = _lib.load()
    rc = L.nrtgpu_count_terms_batch(searcher.ctx._h, searcher._segs, searcher._bases, len(searcher.leaves), m.queries, tc, 1, C.byref(out))
    text = L.nrtgpu_last_error().decode()
    if capacity is None and not null_arrays:
        rc2 = L.nrtgpu_count_terms_supported(searcher.ctx._h, searcher._segs, len(searcher.leaves), m.queries, tc)
        assert rc2 == rc, "the predicate and the call disagree"
    return rc, text


def test_refusals(ix):
    s = ix.searcher
    col = ix.collector(("int", "five"))
    inv, uns = _lib.NRTGPU_ERR_INVALID_ARG, _lib.NRTGPU_ERR_UNSUPPORTED
    or3 = QUERIES[1][1]
    refusals = [
        ("max_buckets 0", inv, or3, col, 0, {}),
        ("max_buckets -1", inv, or3, col, -1, {}),
        ("max_buckets 65537", inv, or3, col, 65537, {}),
        ("capacity below max_buckets", inv, or3, col, 16, dict(capacity=15)),
        ("NULL output arrays", inv, or3, col, 16, dict(null_arrays=True)),
        ("numHits 0", inv, or3, col, 16, dict(mgr=api.TopScoreDocCollectorManager(0))),
        ("max_buckets 0 over no column", inv, or3, api.TermsCollector(55, 10), 0, {}),
        ("no column on any leaf", uns, or3, api.TermsCollector(55, 10), 16, {}),
        ("dismax", uns, api.DisjunctionMaxQuery((T[1], T[2])), col, 16, {}),
        ("dismax with a tie breaker", uns, api.DisjunctionMaxQuery((T[1], T[2]), 0.3), col, 16, {}),
        ("MUST next to SHOULD", uns, api.BooleanQuery((T[2],), 0, (), (), (T[1],)), col, 16, {}),
        ("min_competitive_score", uns, or3, col, 16, dict(mgr=api.TopScoreDocCollectorManager(10, None, 1000, 0.5))),
        ("numHits 2000", uns, or3, col, 16, dict(mgr=api.TopScoreDocCollectorManager(2000))),
        ("a mask that is not resident", uns, api.BooleanQuery((T[1],), 1, (api.MaskFilter(77),)), col, 16, {}),
        ("a must_not mask that is not resident", uns, api.BooleanQuery((T[1],), 1, (), (api.MaskFilter(78),)), col, 16, {}),
    ]
    for name, code, query, c, b, kw in refusals:
        rc, text = _raw(s, query, c, b, **kw)
        assert rc == code, f"{name}: status {rc}: {text}"
        assert "query 0" in text, f"{name}: {text}"
    # the fixed-point analysis of the final-score routes, the known limit it is on the sorted route
    wide = api.BooleanQuery((T[1], api.BoostQuery(T[2], 2.0 ** -20)))
    rc, text = _raw(s, wide, col, 16)
    assert rc == uns and "fixed-point" in text and "binades" in text, f"status {rc}: {text}"
    assert api.count_terms_supported(s, wide, col, 16) is False
    with pytest.raises(_lib.NrtGpuError) as e:
        api.count_terms_batch(s, [or3, wide], [col, col], 16)
    assert e.value.code == uns and "fixed-point" in str(e.value)
    # a query's has_after and totalHitsThreshold are valid and not read
    rc, text = _raw(s, or3, col, 16, mgr=api.TopScoreDocCollectorManager(10, api.ScoreDoc(3, 1.0), 0))
    assert rc == 0, text
    # the binding raises, and says unsupported where it is
    with pytest.raises(_lib.NrtGpuError) as e:
        api.count_terms_batch(s, [or3], [api.TermsCollector(55, 10)], 16)
    assert e.value.code == uns and "55" in str(e.value)
    assert api.count_terms_supported(s, or3, api.TermsCollector(55, 10), 16) is False
    with pytest.raises(_lib.NrtGpuError):
        api.count_terms_supported(s, or3, col, 0)
    # NULL arguments with a context
    q, t, o = _lib.Bm25Query(), _lib.TermsCount(), _lib.TermCounts()
    L = _lib.load()
    assert L.nrtgpu_count_terms_batch(s.ctx._h, s._segs, s._bases, 3, None, C.byref(t), 1, C.byref(o)) == inv
    assert L.nrtgpu_count_terms_batch(s.ctx._h, s._segs, s._bases, 3, C.byref(q), None, 1, C.byref(o)) == inv
    assert L.nrtgpu_count_terms_batch(s.ctx._h, s._segs, s._bases, 3, C.byref(q), C.byref(t), 1, None) == inv
    assert L.nrtgpu_count_terms_supported(s.ctx._h, s._segs, 3, None, C.byref(t)) == inv
    # and the route still answers
    same("after_refusals", api.count_terms_batch(s, [or3], [col], 16)[0], ix.expect(("int", "five"), (1, 2, 3), 1, False, 16))


def test_the_workspace_bound(ix):
    """257 tables of 2^17 slots exceed 2^25; 256 fit and run."""
    c = api.GpuContext(device_id=0, max_batch=512)
    leaves = []
    try:
        corpus = fs.make_corpus([200], {1: 0.5}, seed=13)
        values = (np.arange(200) % 3).astype(np.uint32)
        leaves = fs.upload(c, corpus, "int", [(None, values)], column_field=7)
        s = api.GpuIndexSearcher(c, leaves, api.IndexStatistics.from_corpus(corpus))
        col = api.TermsCollector(7, 10)
        with pytest.raises(_lib.NrtGpuError) as e:
            api.count_terms_batch(s, [T[1]] * 257, [col] * 257, 65536)
        assert e.value.code == _lib.NRTGPU_ERR_INVALID_ARG and "33554432" in str(e.value) and "query 256" in str(e.value)
        assert api.count_terms_supported(s, T[1], col, 65536) is True   # (the bound is the call's, not the query's)
        got = api.count_terms_batch(s, [T[1]] * 256, [col] * 256, 65536)
        exp = ref.count(corpus, [(None, values)], "int", (1,), 1, 65536)
        for tc in got[:: 51]:
            same("256_tables_of_2^17", tc, exp)
    finally:
        release(leaves)
        c.close()


def test_leaves_that_disagree_on_the_kind(ctx, ix):
    rng = np.random.default_rng(31)
    leaves = []
    try:
        for seg, kind in zip(ix.corpus.segments, ("int", "float", "int")):
            g = api.GpuSegment(ctx, seg.max_doc, seg.doc_base)
            leaves.append(g)
            g.add_field_norms(0, seg.norms)
            g.add_terms(0, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
            g.add_doc_values(7, kind, rng.choice(fs.VALUES[kind], size=seg.max_doc))
            g.seal()
        s = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics.from_corpus(ix.corpus))
        rc, text = _raw(s, T[1], api.TermsCollector(7, 10), 16)
        assert rc == _lib.NRTGPU_ERR_INVALID_ARG and "kinds" in text and "query 0" in text
    finally:
        release(leaves)


@pytest.mark.parametrize("flag", [_lib.NRTGPU_FLAG_PACKED_POSTINGS, _lib.NRTGPU_FLAG_NO_FIXED_POINT])
def test_contexts_the_route_refuses(flag):
    corpus = fs.make_corpus([200], {1: 0.5}, seed=13)
    c = api.GpuContext(device_id=0, max_batch=16, flags=flag)
    leaves = []
    try:
        leaves = fs.upload(c, corpus, "int", [(None, np.arange(200, dtype=np.uint32))], column_field=7)
        s = api.GpuIndexSearcher(c, leaves, api.IndexStatistics.from_corpus(corpus))
        rc, text = _raw(s, T[1], api.TermsCollector(7, 10), 16)
        assert rc == _lib.NRTGPU_ERR_UNSUPPORTED and len(text) > 20
        assert api.count_terms_supported(s, T[1], api.TermsCollector(7, 10), 16) is False
        assert s.search_batch([T[1]], [api.TopScoreDocCollectorManager(10)])[0].total_hits == len(corpus.segments[0].postings(1)[0])
    finally:
        release(leaves)
        c.close()
