"""Doc-set requests (nrtgpu_search_docset_sorted_batch, nrtgpu_count_docset_terms_batch) through the C ABI on the device, against
tests/_docset_ref.py.  Every comparison is exact equality of every output field.  Needs a real MI355X."""
import numpy as np
import pytest

from nrtsearch_amd import _lib, api, synth

from tests import _docset_ref as ref
from tests import _field_sort_ref as fs

pytestmark = pytest.mark.gpu
ALL = ref.ALL
T_ALL = api.TermQuery(0, ALL)
INT_MAX = 2**31 - 1
NAN_PAYLOADS = np.array([0x7FC00000, 0x7FC00001, 0xFFC12345], dtype=np.uint32)


def _f(values) -> np.ndarray:
    return np.asarray(values, dtype=np.float32).view(np.uint32)


def _i(values) -> np.ndarray:
    return np.asarray(values, dtype=np.int64).astype(np.int32).view(np.uint32)


# the twelve columns of the terms aggregation's tests: (kind, name) -> the pool of value bits a column draws from.  The two "edge"
# columns are the sort tests' edge sets (ties decide almost every rank).
POOLS = {
    ("int", "const"): _i([42]),
    ("int", "two"): _i([-7, 9]),
    ("int", "five"): _i([3, 1, 4, 15, 9]),
    ("int", "many"): _i(np.arange(700) * 37 - 9000),
    ("int", "edge"): _i([fs.INT32_MIN, -1, 0, 1, fs.INT32_MAX]),
    ("int", "strided"): _i(np.concatenate([np.arange(-20, 20) << 8, np.arange(-20, 20) << 16, np.arange(-20, 20) << 20])),
    ("float", "const"): _f([2.5]),
    ("float", "two"): _f([-1.0, 1.0]),
    ("float", "five"): _f([0.5, 1.0, 2.0, 4.5, -3.0]),
    ("float", "many"): _f(np.arange(700) * 0.25 - 60.0),
    ("float", "edge"): np.concatenate([_f([-np.inf, -1.5, -0.0, 0.0, 1e-45, 3.25, np.inf]), NAN_PAYLOADS]),
    ("float", "strided"): np.concatenate([np.arange(1, 41, dtype=np.uint32) << 8, np.arange(1, 41, dtype=np.uint32) << 16,
                                          np.arange(1, 41, dtype=np.uint32) << 20]).astype(np.uint32),
}
FIELD = {key: 10 + i for i, key in enumerate(POOLS)}
EDGE = {"int": ("int", "edge"), "float": ("float", "edge")}
# doc sets: name -> (filter mask ids, must_not mask ids); mask 9 holds no doc
DOCSETS = {"all": ((), ()), "filter": ((5,), ()), "masks": ((5, 8), (6,)), "empty": ((9,), ())}
MASK_DENSITY = {5: 0.6, 6: 0.2, 8: 0.7, 9: 0.0}
NAN, PINF, NINF, NZERO, PZERO = 0x7FC00000, 0x7F800000, 0xFF800000, 0x80000000, 0x00000000
I5, F5, IE, FE = ("int", "five"), ("float", "five"), ("int", "edge"), ("float", "edge")


def range_sets(key):
    """name -> [(column key, lower bits, upper bits)]; key: the sort / count column."""
    order = np.argsort(fs.order_key(key[0], POOLS[key]), kind="stable")
    lo, hi = int(POOLS[key][order[min(1, len(order) - 1)]]), int(POOLS[key][order[max(len(order) - 2, 0)]])
    return {
        "none": [],
        "on_the_column": [(key, lo, hi)],
        "on_another": [(I5, int(_i([3])[0]), int(_i([9])[0]))],
        "four_over_three": [(I5, int(_i([1])[0]), int(_i([15])[0])), (F5, int(_f([-3.0])[0]), int(_f([2.0])[0])),
                            (IE, int(_i([-1])[0]), int(_i([INT_MAX])[0])), (I5, int(_i([3])[0]), int(_i([15])[0]))],
        "empty_range": [(I5, int(_i([9])[0]), int(_i([3])[0]))],
        "full_float": [(FE, NINF, NAN)],            # still drops the docs without a value
        "full_int": [(IE, int(_i([fs.INT32_MIN])[0]), int(_i([INT_MAX])[0]))],
        "nan_only": [(FE, NAN, 0xFFC00001)],        # any NaN is the canonical bound
        "up_to_inf": [(FE, NINF, PINF)],            # drops the NaNs
        "neg_zero_only": [(FE, NZERO, NZERO)],
        "from_pos_zero": [(FE, PZERO, PINF)],
        "zeros_reversed": [(FE, PZERO, NZERO)],     # +0.0 > -0.0: empty
        "int_min_only": [(IE, int(_i([fs.INT32_MIN])[0]), int(_i([fs.INT32_MIN])[0]))],
        "int_max_only": [(IE, int(_i([INT_MAX])[0]), int(_i([INT_MAX])[0]))],
    }


@pytest.fixture(scope="module", autouse=True)
def two_column_postings():
    """The text routes these tests cross-check against refuse packed postings: the contexts here keep the two-column layout also
    where the whole suite runs with NRTGPU_PACKED_POSTINGS=1 (the doc-set route under that flag has a test of its own below)."""
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


def same_docs(name, got, exp):
    docs, bits, total, gte = exp
    assert got.docs.tolist() == docs.tolist(), f"{name}: docs"
    assert got.value_bits.tolist() == bits.tolist(), f"{name}: value bits"
    assert got.total_hits == total, f"{name}: total_hits {got.total_hits}, the reference counts {total}"
    assert got.relation_gte == gte, f"{name}: relation"


def same_counts(name, got, exp):
    bits, counts, n, total, valued, over = exp
    assert got.total_hits == total, f"{name}: total_hits {got.total_hits}, the reference counts {total}"
    assert int(got.overflowed) == over, f"{name}: overflowed {got.overflowed}"
    assert len(got.counts) == n and len(got.values) == n, f"{name}: {len(got.counts)} buckets, the reference has {n}"
    assert got.value_bits.tolist() == bits.tolist(), f"{name}: value bits"
    assert got.counts.tolist() == counts.tolist(), f"{name}: counts"
    assert got.hits_with_value == valued, f"{name}: hits_with_value {got.hits_with_value}, the reference has {valued}"


def chunks(seq, n=256):
    return [seq[i: i + n] for i in range(0, len(seq), n)]


def sorted_batch(searcher, docsets, managers, sorts, afters=None):
    out = []
    for lo in range(0, len(docsets), 256):
        out += api.search_docset_sorted_batch(searcher, docsets[lo: lo + 256], managers[lo: lo + 256], sorts[lo: lo + 256],
                                              None if afters is None else afters[lo: lo + 256])
    return out


def counted_batch(searcher, docsets, collectors, bounds):
    out = []
    for lo in range(0, len(docsets), 256):
        out += api.count_docset_terms_batch(searcher, docsets[lo: lo + 256], collectors[lo: lo + 256], bounds[lo: lo + 256])
    return out


# ---- index A: the sort tests' leaves of 3000, 1500 and 40 docs, 1 % deletes; every column on 80 % of leaf 0, all of leaf 1, absent
# ---- from leaf 2; term ALL in every doc (the parent's routes answer the same question through it)
class IndexA:
    def __init__(self, ctx, corpus):
        rng = np.random.default_rng(41)
        self.corpus = corpus
        self.columns = {}
        for key, pool in POOLS.items():
            d0 = np.nonzero(rng.random(3000) < 0.8)[0].astype(np.int32)
            self.columns[key] = [(d0, rng.choice(pool, size=len(d0))), (None, rng.choice(pool, size=1500)), None]
        self.masks = {mid: [synth.random_mask(seg.max_doc, dens, 40 * mid + si) for si, seg in enumerate(corpus.segments)]
                      for mid, dens in MASK_DENSITY.items()}
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
            for mid, words in self.masks.items():
                g.set_mask(mid, words[si])
            self.leaves.append(g)
        self.searcher = api.GpuIndexSearcher(ctx, self.leaves, api.IndexStatistics.from_corpus(corpus))
        self._hits = {}

    def hits(self, ds_name, rs, live=None):
        """the hit set's words per leaf (computed once per doc set and range set, shared, never written)"""
        memo = (ds_name, tuple(rs), None if live is None else id(live))
        if memo not in self._hits:
            f, mn = DOCSETS[ds_name]
            self._hits[memo] = ref.hit_set(self.corpus, [self.masks[m] for m in f], [self.masks[m] for m in mn],
                                           [(key[0], self.columns[key], lo, hi) for key, lo, hi in rs], live)
        return self._hits[memo]

    @staticmethod
    def query(ds_name, rs):
        f, mn = DOCSETS[ds_name]
        return api.DocSetQuery(tuple(api.MaskFilter(m) for m in f), tuple(api.MaskFilter(m) for m in mn),
                               tuple(api.RangeClause(FIELD[key], key[0], fs.value_of(key[0], lo), fs.value_of(key[0], hi)) for key, lo, hi in rs))

    @staticmethod
    def sort(key, reverse, missing_bits):
        return api.SortField(FIELD[key], key[0], reverse, fs.value_of(key[0], missing_bits))

    @staticmethod
    def collector(key):
        return api.TermsCollector(FIELD[key], 10, True, key[0])


@pytest.fixture(scope="module")
def corpus_a():
    c = fs.make_corpus([3000, 1500, 40], {ALL: 1.0, 2: 0.3}, seed=5, delete_fraction=0.01)
    assert all(seg.live_bits is not None for seg in c.segments)
    return c


@pytest.fixture(scope="module")
def ix(ctx, corpus_a):
    x = IndexA(ctx, corpus_a)
    yield x
    release(x.leaves)


def missing_values(kind):
    return (fs.KIND_MIN[kind], fs.KIND_MAX[kind], int(fs.VALUES[kind][2]))


# ---- sorted ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["int", "float"])
def test_sorted_over_every_doc_set_and_range_set(ix, kind):
    key = EDGE[kind]
    sets = range_sets(key)
    cases = [(ds, rn, 10, rev, fs.KIND_MAX[kind]) for ds in DOCSETS for rn in sets for rev in (False, True)]
    cases += [(ds, rn, k, rev, mb) for ds, rn in (("all", "none"), ("masks", "on_the_column"), ("filter", "four_over_three"), ("all", "full_float"))
              for k in (1, 10, 1024) for rev in (False, True) for mb in missing_values(kind)]
    before = ix.searcher.ctx.stats()
    got = sorted_batch(ix.searcher, [ix.query(ds, sets[rn]) for ds, rn, _, _, _ in cases], [api.TopScoreDocCollectorManager(k) for _, _, k, _, _ in cases],
                       [ix.sort(key, rev, mb) for _, _, _, rev, mb in cases])
    d = api.GpuContext.last_diagnostics()
    after = ix.searcher.ctx.stats()
    assert d["items_maxscore"] == 0 and d["items_scan"] >= 1 and d["postings"] == 0
    assert after["scan_launches"] == before["scan_launches"] + len(chunks(cases)) and after["maxscore_launches"] == before["maxscore_launches"]
    totals, full_pages = {}, 0
    for (ds, rn, k, rev, mb), td in zip(cases, got):
        exp = ref.search(ix.corpus, ix.hits(ds, sets[rn]), ix.columns[key], kind, k, rev, mb)
        same_docs(f"{kind}_{ds}_{rn}_k{k}_rev{int(rev)}_missing{mb:#x}", td, exp)
        totals[(ds, rn)] = exp[2]
        full_pages += int(k == 1024 and exp[2] > 1024)
    live = sum(fs.live_count(s) for s in ix.corpus.segments)
    assert totals[("all", "none")] == live and all(totals[("empty", rn)] == 0 for rn in sets)
    assert all(totals[(ds, rn)] == 0 for ds in DOCSETS for rn in ("empty_range", "zeros_reversed"))
    assert 0 < totals[("all", "full_int")] < live and 0 < totals[("all", "up_to_inf")] < totals[("all", "full_float")] < live
    assert totals[("all", "nan_only")] == totals[("all", "full_float")] - totals[("all", "up_to_inf")] > 0
    assert all(totals[("all", rn)] > 0 for rn in ("neg_zero_only", "from_pos_zero", "int_min_only", "int_max_only", "four_over_three"))
    assert totals[("masks", "four_over_three")] > 0 and full_pages >= 6
    assert api.docset_sorted_supported(ix.searcher, ix.query("masks", sets["four_over_three"]), api.TopScoreDocCollectorManager(10), ix.sort(key, False, 0)) is True


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("reverse", [False, True])
def test_pages_of_7_equal_one_page_of_70(ix, kind, reverse):
    key = EDGE[kind]
    rs = range_sets(key)["on_another"]
    q, hits, mb = ix.query("filter", rs), ix.hits("filter", rs), int(fs.VALUES[kind][2])
    sort = ix.sort(key, reverse, mb)
    full = api.search_docset_sorted_batch(ix.searcher, [q], [api.TopScoreDocCollectorManager(70)], [sort])[0]
    same_docs(f"{kind}_page70", full, ref.search(ix.corpus, hits, ix.columns[key], kind, 70, reverse, mb))
    after, docs, bits, cut_in_a_run = None, [], [], 0
    for page in range(10):
        got = api.search_docset_sorted_batch(ix.searcher, [q], [api.TopScoreDocCollectorManager(7)], [sort], [after])[0]
        exp = ref.search(ix.corpus, hits, ix.columns[key], kind, 7, reverse, mb,
                         after=None if after is None else (after.doc, fs.bits_of(kind, after.value)))
        same_docs(f"{kind}_page7_{page}", got, exp)
        assert got.total_hits == full.total_hits   # hits of earlier pages still count
        if bits:
            cut_in_a_run += int(bits[-1] == int(got.value_bits[0]))
        docs += got.docs.tolist()
        bits += got.value_bits.tolist()
        after = api.FieldDoc(int(got.docs[-1]), fs.value_of(kind, int(got.value_bits[-1])))
    assert docs == full.docs.tolist() and bits == full.value_bits.tolist() and cut_in_a_run >= 5


def test_relation_per_slice(corpus_a):
    c = api.GpuContext(device_id=0, max_batch=16)
    x = None
    try:
        c.set_slicing(1000, 5, 1)
        slicing = (1000, 5, 1)
        x = IndexA(c, corpus_a)
        key = EDGE["int"]
        rs = range_sets(key)["on_another"]
        hits, info = x.hits("filter", rs), {}
        ref.search(x.corpus, hits, x.columns[key], "int", 10, False, 0, total_hits_threshold=50, slicing=slicing, info=info)
        per_slice = info["slice_hits"]
        assert len(per_slice) == 3 and max(per_slice) > 50 and min(per_slice) <= 50
        for thr, gte in ((50, True), (max(per_slice), False), (INT_MAX, False)):
            got = api.search_docset_sorted_batch(x.searcher, [x.query("filter", rs)], [api.TopScoreDocCollectorManager(10, None, thr)], [x.sort(key, False, 0)])[0]
            same_docs(f"slices_thr{thr}", got, ref.search(x.corpus, hits, x.columns[key], "int", 10, False, 0, total_hits_threshold=thr, slicing=slicing))
            assert got.relation_gte == gte and (got.total_hits > thr or thr == INT_MAX)
    finally:
        if x is not None:
            release(x.leaves)
        c.close()


# ---- the parent's routes answer a range-free doc set through a clause every doc matches ----------------------------------------------
def test_range_free_doc_sets_equal_the_text_routes_over_a_term_in_every_doc(ix):
    docsets, texts = [], []
    for ds, (f, mn) in DOCSETS.items():
        docsets.append(ix.query(ds, []))
        texts.append(api.BooleanQuery((T_ALL,), 1, tuple(api.MaskFilter(m) for m in f), tuple(api.MaskFilter(m) for m in mn)) if f or mn else T_ALL)
    n = len(docsets)
    for kind in ("int", "float"):
        key = EDGE[kind]
        for k, rev, thr in ((10, False, 1000), (1024, True, 1000), (7, True, 100)):
            mgrs = [api.TopScoreDocCollectorManager(k, None, thr)] * n
            sorts = [ix.sort(key, rev, fs.KIND_MIN[kind])] * n
            a = api.search_docset_sorted_batch(ix.searcher, docsets, mgrs, sorts)
            b = api.search_sorted_batch(ix.searcher, texts, mgrs, sorts)
            for ds, x, y in zip(DOCSETS, a, b):
                same_docs(f"{kind}_{ds}_k{k}", x, (y.docs, y.value_bits, y.total_hits, y.relation_gte))
    for key in POOLS:
        a = api.count_docset_terms_batch(ix.searcher, docsets, [ix.collector(key)] * n, 1024)
        b = api.count_terms_batch(ix.searcher, texts, [ix.collector(key)] * n, 1024)
        for ds, x, y in zip(DOCSETS, a, b):
            same_counts(f"{key}_{ds}", x, (y.value_bits, y.counts, len(y.counts), y.total_hits, y.hits_with_value, int(y.overflowed)))
            assert (x.total_hits == 0) == (ds == "empty")


# ---- terms ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["int", "float"])
def test_counts_over_the_twelve_columns_every_doc_set_and_range_set(ix, kind):
    keys = [k for k in POOLS if k[0] == kind]
    cases = [(key, ds, rn) for key in keys for ds in DOCSETS for rn in range_sets(key)]
    got = counted_batch(ix.searcher, [ix.query(ds, range_sets(key)[rn]) for key, ds, rn in cases], [ix.collector(key) for key, _, _ in cases], [1024] * len(cases))
    d = api.GpuContext.last_diagnostics()
    assert d["items_maxscore"] == 0 and d["items_scan"] >= 1
    seen = set()
    for (key, ds, rn), tc in zip(cases, got):
        exp = ref.count(ix.corpus, ix.hits(ds, range_sets(key)[rn]), ix.columns[key], kind, 1024)
        same_counts(f"{key}_{ds}_{rn}", tc, exp)
        assert exp[5] == 0 and (ds != "empty" or exp[3] == 0)
        if (ds, rn) == ("all", "none"):
            assert exp[4] < exp[3]   # some hit lacks a value (leaf 2, 20 % of leaf 0)
            seen.add((key[1], exp[2]))
    assert ("const", 1) in seen and ("two", 2) in seen and ("five", 5) in seen and max(n for name, n in seen if name == "many") > 600
    at = [c for c in cases].index((EDGE[kind], "all", "none"))
    if kind == "float":   # three NaN payloads: one bucket, reported canonical and last; the zeros: two buckets
        assert got[at].value_bits.tolist() == _f([-np.inf, -1.5, -0.0, 0.0, 1e-45, 3.25, np.inf]).tolist() + [NAN]
    else:
        assert got[at].values.tolist() == [fs.INT32_MIN, -1, 0, 1, fs.INT32_MAX]
    assert api.count_docset_terms_supported(ix.searcher, ix.query("masks", range_sets(keys[0])["four_over_three"]), ix.collector(keys[0]), 1024) is True


def test_the_overflow_boundary(ix):
    cases = []
    for kind in ("int", "float"):
        for name in ("const", "two", "many"):
            key = (kind, name)
            for ds, rn in (("all", "none"), ("masks", "on_another")):
                rs = range_sets(key)[rn]
                distinct = ref.count(ix.corpus, ix.hits(ds, rs), ix.columns[key], kind)[2]
                assert distinct == {"const": 1, "two": 2}.get(name, distinct) and (name != "many" or distinct > 100)
                cases += [(key, ds, rs, b) for b in (distinct, distinct - 1, distinct + 1) if b >= 1]
    got = counted_batch(ix.searcher, [ix.query(ds, rs) for _, ds, rs, _ in cases], [ix.collector(c[0]) for c in cases], [c[3] for c in cases])
    overflowed = 0
    for (key, ds, rs, b), tc in zip(cases, got):
        exp = ref.count(ix.corpus, ix.hits(ds, rs), ix.columns[key], key[0], b)
        same_counts(f"{key}_{ds}_max_buckets_{b}", tc, exp)
        overflowed += exp[5]
    assert overflowed == 8 and len(cases) == 32   # max_buckets one below the distinct count, wherever that is >= 1, overflows


def test_a_mixed_batch_of_64_sorted_and_counted(ix):
    rng = np.random.default_rng(77)
    keys, ds_names = list(POOLS), list(DOCSETS)
    cases = []
    for i in range(64):
        key = keys[int(rng.integers(len(keys)))]
        sets = range_sets(key)
        rn = list(sets)[int(rng.integers(len(sets)))]
        cases.append((key, ds_names[int(rng.integers(len(ds_names)))], sets[rn], int(rng.choice([1, 5, 100, 1024])), bool(rng.integers(2)), int(rng.choice([1, 4, 64, 4096]))))
    docsets = [ix.query(ds, rs) for _, ds, rs, _, _, _ in cases]
    got = api.search_docset_sorted_batch(ix.searcher, docsets, [api.TopScoreDocCollectorManager(k) for _, _, _, k, _, _ in cases],
                                         [ix.sort(key, rev, fs.KIND_MIN[key[0]]) for key, _, _, _, rev, _ in cases])
    cnt = api.count_docset_terms_batch(ix.searcher, docsets, [ix.collector(c[0]) for c in cases], [c[5] for c in cases])
    overflowed = 0
    for i, ((key, ds, rs, k, rev, b), td, tc) in enumerate(zip(cases, got, cnt)):
        same_docs(f"mixed_{i}", td, ref.search(ix.corpus, ix.hits(ds, rs), ix.columns[key], key[0], k, rev, fs.KIND_MIN[key[0]]))
        exp = ref.count(ix.corpus, ix.hits(ds, rs), ix.columns[key], key[0], b)
        same_counts(f"mixed_{i}", tc, exp)
        overflowed += exp[5]
    assert 0 < overflowed < 64   # overflowed queries beside exact ones in one batch


# ---- index B: ONE leaf of 13 000 docs (not a multiple of 64), no deletes: word skipping, the tail, the candidate buffer ----------
@pytest.fixture(scope="module")
def ix_b(ctx):
    n = 13_000
    corpus = fs.make_corpus([n], {ALL: 1.0}, seed=8)
    seg = corpus.segments[0]
    assert seg.live_bits is None and n % 64 != 0
    perm = np.random.default_rng(9).permutation(n).astype(np.int32)
    values = {7: perm, 8: np.full(n, 42, dtype=np.int32), 9: (np.arange(n, dtype=np.int32) % 2)}
    g = api.GpuSegment(ctx, n, 0)
    g.add_field_norms(0, seg.norms)
    g.add_terms(0, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
    for f, v in values.items():
        g.add_doc_values(f, "int", v)
    g.seal()
    masks = {}
    for mid, docs in ((5, (70, 6_400, 12_930)), (6, (0, n - 1))):
        ok = np.zeros(n, dtype=bool)
        ok[list(docs)] = True
        masks[mid] = [ref.pack(ok)]
        g.set_mask(mid, masks[mid][0])
    searcher = api.GpuIndexSearcher(ctx, [g], api.IndexStatistics.from_corpus(corpus))
    columns = {f: [(None, v.view(np.uint32))] for f, v in values.items()}
    yield corpus, searcher, columns, masks
    g.release()


def test_word_skipping_and_the_tail(ix_b):
    corpus, searcher, columns, masks = ix_b
    n = corpus.segments[0].max_doc
    docsets = [api.DocSetQuery((api.MaskFilter(5),)), api.DocSetQuery((api.MaskFilter(6),)), api.DocSetQuery(),
               api.DocSetQuery((), (api.MaskFilter(5), api.MaskFilter(6))), api.DocSetQuery((), (), (api.RangeClause(9, "int", 1, 1),))]
    hit_sets = [ref.hit_set(corpus, [masks[5]]), ref.hit_set(corpus, [masks[6]]), ref.hit_set(corpus),
                ref.hit_set(corpus, [], [masks[5], masks[6]]), ref.hit_set(corpus, ranges=[("int", columns[9], 1, 1)])]
    totals = (3, 2, n, n - 5, n // 2)
    for col, rev, k in ((7, False, 10), (7, True, 1024), (8, False, 1024), (8, True, 3)):
        # ascending over the permutation: a doc at or beyond max_doc would read a padded code of 0 = the int minimum and rank first
        got = api.search_docset_sorted_batch(searcher, docsets, [api.TopScoreDocCollectorManager(k)] * 5, [api.SortField(col, "int", rev, 0)] * 5)
        for i, (td, hits, total) in enumerate(zip(got, hit_sets, totals)):
            exp = ref.search(corpus, hits, columns[col], "int", k, rev, 0)
            same_docs(f"col{col}_rev{int(rev)}_set{i}", td, exp)
            assert exp[2] == total and (len(td.docs) == 0 or int(td.docs.max()) < n)
    cnt = api.count_docset_terms_batch(searcher, docsets, [api.TermsCollector(9, 10)] * 5, 16)
    for i, (tc, hits, total) in enumerate(zip(cnt, hit_sets, totals)):
        same_counts(f"count_set{i}", tc, ref.count(corpus, hits, columns[9], "int", 16))
        assert tc.total_hits == total == tc.hits_with_value


@pytest.mark.parametrize("column", [7, 8])
def test_the_candidate_buffer_overflows(ix_b, column):
    """13 000 accepted docs in one item: the first round's candidates do not fit.  Column 7: a permutation, no ties; column 8: a
    constant -- every key ties on the high word."""
    corpus, searcher, columns, _ = ix_b
    hits = ref.hit_set(corpus)
    cases = [(k, rev) for k in (1, 1000, 1024) for rev in (False, True)]
    got = api.search_docset_sorted_batch(searcher, [api.DocSetQuery()] * len(cases), [api.TopScoreDocCollectorManager(k) for k, _ in cases],
                                         [api.SortField(column, "int", rev, 0) for _, rev in cases])
    assert api.GpuContext.last_diagnostics()["items_scan"] == len(cases)
    for (k, rev), td in zip(cases, got):
        same_docs(f"col{column}_k{k}_rev{int(rev)}", td, ref.search(corpus, hits, columns[column], "int", k, rev, 0))
        assert td.total_hits == 13_000 and len(td.docs) == k


def test_more_distinct_values_than_the_workgroup_table_takes(ix_b):
    corpus, searcher, columns, masks = ix_b
    hits = ref.hit_set(corpus)
    for bound, over in ((8192, 1), (4, 1), (13_000, 0), (16_384, 0)):
        exp = ref.count(corpus, hits, columns[7], "int", bound)
        assert exp[5] == over
        same_counts(f"alone_{bound}", api.count_docset_terms_batch(searcher, [api.DocSetQuery()], [api.TermsCollector(7, 10)], bound)[0], exp)
    # in a batch whose other queries stay exact
    docsets = [api.DocSetQuery(), api.DocSetQuery(), api.DocSetQuery((api.MaskFilter(5),)), api.DocSetQuery(), api.DocSetQuery()]
    cols, bounds = [7, 9, 7, 7, 8], [8192, 16, 4, 4, 1]
    hs = [hits, hits, ref.hit_set(corpus, [masks[5]]), hits, hits]
    got = api.count_docset_terms_batch(searcher, docsets, [api.TermsCollector(c, 10) for c in cols], bounds)
    exps = [ref.count(corpus, h, columns[c], "int", b) for h, c, b in zip(hs, cols, bounds)]
    assert [e[5] for e in exps] == [1, 0, 0, 1, 0]
    for i, (tc, exp) in enumerate(zip(got, exps)):
        same_counts(f"batch_{i}", tc, exp)


# ---- index C: 300 000 docs in one leaf, cut into several items --------------------------------------------------------------------
def test_several_items_every_winner_in_the_last_one_and_one_count_table(ctx):
    n = 300_000
    corpus = fs.make_corpus([n], {ALL: 1.0}, seed=3)
    seg = corpus.segments[0]
    rising = np.arange(n, dtype=np.int32)          # descending sort: every winner in the last item
    buckets = (np.arange(n, dtype=np.int32) * 7) % 1000
    g = api.GpuSegment(ctx, n, 0)
    try:
        g.add_field_norms(0, seg.norms)
        g.add_terms(0, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
        g.add_doc_values(7, "int", rising)
        g.add_doc_values(8, "int", buckets)
        g.seal()
        searcher = api.GpuIndexSearcher(ctx, [g], api.IndexStatistics.from_corpus(corpus))
        cols = {7: [(None, rising.view(np.uint32))], 8: [(None, buckets.view(np.uint32))]}
        half = api.DocSetQuery((), (), (api.RangeClause(8, "int", 0, 499),))
        hit_sets = [ref.hit_set(corpus), ref.hit_set(corpus, ranges=[("int", cols[8], 0, 499)])]
        for k, rev in ((1024, True), (10, False), (1024, False)):
            got = api.search_docset_sorted_batch(searcher, [api.DocSetQuery(), half], [api.TopScoreDocCollectorManager(k)] * 2, [api.SortField(7, "int", rev, 0)] * 2)
            assert api.GpuContext.last_diagnostics()["items_scan"] >= 4   # (293 sub-tiles, items of at least 64)
            for td, hits in zip(got, hit_sets):
                same_docs(f"k{k}_rev{int(rev)}", td, ref.search(corpus, hits, cols[7], "int", k, rev, 0))
            assert got[0].total_hits == n and got[0].relation_gte and (int(got[0].docs[0]) == n - 1) == rev
        cnt = api.count_docset_terms_batch(searcher, [api.DocSetQuery(), half, api.DocSetQuery()], [api.TermsCollector(8, 10)] * 3, [1024, 1024, 999])
        assert api.GpuContext.last_diagnostics()["items_scan"] >= 6
        for tc, hits, b in zip(cnt, hit_sets + hit_sets[:1], (1024, 1024, 999)):
            same_counts(f"items_{b}", tc, ref.count(corpus, hits, cols[8], "int", b))
        assert len(cnt[0].counts) == 1000 and len(cnt[1].counts) == 500 and cnt[2].overflowed and cnt[2].total_hits == n
    finally:
        g.release()


# ---- also ----------------------------------------------------------------------------------------------------------------------------
def test_a_fork_with_more_deletes_reads_the_shared_columns(ix):
    corpus = ix.corpus
    lives, forks = [], []
    try:
        for si, (seg, leaf) in enumerate(zip(corpus.segments, ix.leaves)):
            n = (seg.max_doc + 63) // 64
            live = seg.live_bits[:n] & ~synth.random_mask(seg.max_doc, 0.3, 900 + si)[:n]
            lives.append(live)
            f = leaf.fork(live)
            for mid, words in ix.masks.items():
                f.set_mask(mid, words[si])
            forks.append(f)
        searcher = api.GpuIndexSearcher(ix.searcher.ctx, forks, api.IndexStatistics.from_corpus(corpus))
        key = EDGE["float"]
        for ds, rn in (("all", "none"), ("masks", "four_over_three")):
            rs = range_sets(key)[rn]
            f, mn = DOCSETS[ds]
            hits = ref.hit_set(corpus, [ix.masks[m] for m in f], [ix.masks[m] for m in mn], [(k[0], ix.columns[k], lo, hi) for k, lo, hi in rs], live=lives)
            got = api.search_docset_sorted_batch(searcher, [ix.query(ds, rs)], [api.TopScoreDocCollectorManager(100)], [ix.sort(key, True, fs.KIND_MIN["float"])])[0]
            same_docs(f"fork_{ds}", got, ref.search(corpus, hits, ix.columns[key], "float", 100, True, fs.KIND_MIN["float"]))
            cnt = api.count_docset_terms_batch(searcher, [ix.query(ds, rs)], [ix.collector(key)], 64)[0]
            same_counts(f"fork_{ds}", cnt, ref.count(corpus, hits, ix.columns[key], "float", 64))
            parent = api.search_docset_sorted_batch(ix.searcher, [ix.query(ds, rs)], [api.TopScoreDocCollectorManager(100)], [ix.sort(key, True, fs.KIND_MIN["float"])])[0]
            same_docs(f"fork_parent_{ds}", parent, ref.search(corpus, ix.hits(ds, rs), ix.columns[key], "float", 100, True, fs.KIND_MIN["float"]))
            assert parent.total_hits > got.total_hits > 0
    finally:
        release(forks)


def test_device_bytes_are_unchanged_by_a_search(ix):
    key = EDGE["int"]
    q, sort = ix.query("masks", range_sets(key)["four_over_three"]), ix.sort(key, False, 0)
    api.search_docset_sorted_batch(ix.searcher, [q], [api.TopScoreDocCollectorManager(10)], [sort])   # (the combined accept set is built on first use)
    before = [l.device_bytes for l in ix.leaves]
    api.search_docset_sorted_batch(ix.searcher, [q, ix.query("all", [])], [api.TopScoreDocCollectorManager(10)] * 2, [sort] * 2)
    api.count_docset_terms_batch(ix.searcher, [q, ix.query("all", [])], [ix.collector(key)] * 2, 64)
    assert [l.device_bytes for l in ix.leaves] == before


def test_refusals(ix):
    s, inv, uns = ix.searcher, _lib.NRTGPU_ERR_INVALID_ARG, _lib.NRTGPU_ERR_UNSUPPORTED
    key = EDGE["int"]
    top, sort, coll = api.TopScoreDocCollectorManager(10), ix.sort(key, False, 0), ix.collector(key)
    R, MF = api.RangeClause, api.MaskFilter
    five = tuple(R(FIELD[I5], "int", 0, 1) for _ in range(5))
    refusals = [
        ("numHits 0", inv, api.DocSetQuery(), api.TopScoreDocCollectorManager(0), sort, coll, 16),
        ("numHits 1025", inv, api.DocSetQuery(), api.TopScoreDocCollectorManager(1025), sort, coll, 16),
        ("threshold -1", inv, api.DocSetQuery(), api.TopScoreDocCollectorManager(10, None, -1), sort, coll, 16),
        ("five ranges", inv, api.DocSetQuery((), (), five), top, sort, coll, 16),
        ("nine masks", inv, api.DocSetQuery(tuple(MF(5) for _ in range(9))), top, sort, coll, 16),
        ("a mask id 0 among more_filters", inv, api.DocSetQuery((MF(5), MF(0))), top, sort, coll, 16),
        ("no column on any leaf", uns, api.DocSetQuery(), top, api.SortField(55, "int"), api.TermsCollector(55, 10), 16),
        ("a range column on no leaf", uns, api.DocSetQuery((), (), (R(55, "int", 0, 1),)), top, sort, coll, 16),
        ("a mask that is not resident", uns, api.DocSetQuery((MF(77),)), top, sort, coll, 16),
        ("a must_not mask that is not resident", uns, api.DocSetQuery((), (MF(78),)), top, sort, coll, 16),
    ]
    for name, code, d, mgr, so, co, b in refusals:
        with pytest.raises(_lib.NrtGpuError) as e:
            api.search_docset_sorted_batch(s, [d], [mgr], [so])
        assert e.value.code == code and "query 0" in str(e.value), f"{name}: {e.value}"
        with pytest.raises(_lib.NrtGpuError) as e:
            api.count_docset_terms_batch(s, [d], [co], b, [mgr])
        assert e.value.code == code and "query 0" in str(e.value), f"{name}: {e.value}"
        if code == uns:
            assert api.docset_sorted_supported(s, d, mgr, so) is False and api.count_docset_terms_supported(s, d, co, b, mgr) is False
    for b in (0, 65537):
        with pytest.raises(_lib.NrtGpuError) as e:
            api.count_docset_terms_batch(s, [api.DocSetQuery()], [coll], b)
        assert e.value.code == inv
    # an invalid argument in query 1 comes before an unsupported query 0
    with pytest.raises(_lib.NrtGpuError) as e:
        api.search_docset_sorted_batch(s, [api.DocSetQuery((MF(77),)), api.DocSetQuery()], [top, api.TopScoreDocCollectorManager(0)], [sort, sort])
    assert e.value.code == inv and "query 1" in str(e.value)
    # and the route still answers
    got = api.search_docset_sorted_batch(s, [api.DocSetQuery()], [top], [sort])[0]
    same_docs("after_refusals", got, ref.search(ix.corpus, ix.hits("all", []), ix.columns[key], "int", 10, False, 0))


@pytest.mark.parametrize("flag", [_lib.NRTGPU_FLAG_PACKED_POSTINGS, _lib.NRTGPU_FLAG_NO_FIXED_POINT])
def test_the_route_runs_under_the_flags_the_text_routes_over_a_column_refuse(flag, corpus_a):
    c = api.GpuContext(device_id=0, max_batch=16, flags=flag)
    x = None
    try:
        x = IndexA(c, corpus_a)
        key = EDGE["float"]
        for ds, rn in (("all", "none"), ("masks", "four_over_three")):
            rs = range_sets(key)[rn]
            q = x.query(ds, rs)
            assert api.docset_sorted_supported(x.searcher, q, api.TopScoreDocCollectorManager(50), x.sort(key, True, 0)) is True
            got = api.search_docset_sorted_batch(x.searcher, [q], [api.TopScoreDocCollectorManager(50)], [x.sort(key, True, 0)])[0]
            same_docs(f"flag{flag}_{ds}", got, ref.search(x.corpus, x.hits(ds, rs), x.columns[key], "float", 50, True, 0))
            cnt = api.count_docset_terms_batch(x.searcher, [q], [x.collector(key)], 64)[0]
            same_counts(f"flag{flag}_{ds}", cnt, ref.count(x.corpus, x.hits(ds, rs), x.columns[key], "float", 64))
        assert api.sorted_supported(x.searcher, T_ALL, api.TopScoreDocCollectorManager(50), x.sort(key, True, 0)) is False   # (the text route's known limit)
    finally:
        if x is not None:
            release(x.leaves)
        c.close()
