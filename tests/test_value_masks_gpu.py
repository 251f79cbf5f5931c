"""Filter masks built on the device from doc value columns (nrtgpu_segment_set_mask_from_values) through the C ABI, against
tests/_value_masks_ref.py: the words and the count of every clause kind over every column arity at the word and sub-tile edges,
the routes under a built mask against the same routes under the reference's words uploaded through nrtgpu_segment_set_mask, the
mask's life cycle, and a seeded fuzz.  Every comparison is exact equality: words, counts, docids, score bits.  Needs a real MI355X."""
import numpy as np
import pytest

from nrtsearch_amd import _lib, api

from tests import _docset_ref as dsr
from tests import _field_sort_ref as fs
from tests import _value_masks_ref as ref

pytestmark = pytest.mark.gpu
VC = api.ValueClause
MF = api.MaskFilter
NAN, PINF, NINF, NZERO, PZERO = 0x7FC00000, 0x7F800000, 0xFF800000, 0x80000000, 0x00000000
# the values the columns draw from: both int ends; +-inf, +-0.0, the smallest subnormal and NaNs with three payloads
POOL = {"int": fs.VALUES["int"], "float": np.concatenate([fs.VALUES["float"][:-1], np.array([NAN, 0x7F800001, 0xFFC12345], np.uint32)])}
DENSE, SPARSE, MULTI, NONE = 10, 11, 12, 13   # the sweep's columns: one field id per arity; NONE: a multi-valued column with n_values == 0
ARITIES = {"dense": DENSE, "sparse": SPARSE, "multi": MULTI, "no_values": NONE}
MAX_DOCS = [1, 63, 64, 65, 1023, 1024, 1025, 2065]


@pytest.fixture(scope="module", autouse=True)
def two_column_postings():
    """The text routes over a column refuse packed postings: the contexts here keep the two-column layout whatever the suite runs under."""
    mp = pytest.MonkeyPatch()
    mp.delenv("NRTGPU_PACKED_POSTINGS", raising=False)
    yield
    mp.undo()


@pytest.fixture(scope="module")
def ctx(two_column_postings):
    c = api.GpuContext(device_id=0, max_batch=64)
    yield c
    c.close()


def make_columns(rng, n: int, kind: str, pool=None):
    """name -> a column of n docs in the reference's form.  sparse: about 70 % of the docs, never all; multi: docs with 0, 1 and 5
    values, one of them holding the same value five times."""
    pool = POOL[kind] if pool is None else pool
    has = rng.random(n) < 0.7
    has[rng.integers(n)] = False
    sparse_docs = np.nonzero(has)[0].astype(np.int32)
    per_doc = rng.choice([0, 1, 5], size=n)
    if n >= 3:
        per_doc[[0, n // 2, n - 1]] = [5, 0, 1]
    multi_docs = np.repeat(np.arange(n, dtype=np.int32), per_doc)
    multi_bits = rng.choice(pool, size=len(multi_docs))
    if per_doc[0] == 5:
        multi_bits[:5] = multi_bits[0]   # duplicates inside a doc
    return {"dense": ("single", None, rng.choice(pool, size=n)), "sparse": ("single", sparse_docs, rng.choice(pool, size=len(sparse_docs))),
            "multi": ("multi", multi_docs, multi_bits), "no_values": ("multi", np.zeros(0, np.int32), np.zeros(0, np.uint32))}


def add_column(g, field: int, kind: str, column):
    arity, docs, bits = column
    if arity == "multi":
        g.add_doc_values_multi(field, kind, np.asarray(bits, np.uint32), np.asarray(docs, np.int32))
    else:
        g.add_doc_values(field, kind, np.asarray(bits, np.uint32), docs)


def upload_columns(ctx, n: int, kind: str, columns, live=None):
    g = api.GpuSegment(ctx, n, 0)
    for name, field in ARITIES.items():
        add_column(g, field, kind, columns[name])
    g.seal()
    if live is not None:
        g.set_live_docs(live)
    return g


def api_clause(field: int, clause):
    if clause[0] == "exists":
        return VC.exists(field)
    if clause[0] == "range":
        return VC("range", field, clause[1], int(clause[2]), int(clause[3]))
    return VC.in_set(field, clause[1], np.asarray(clause[2], dtype=np.uint32))


def set_of_4096(kind: str, pool) -> np.ndarray:
    """exactly NRTGPU_MAX_SET_VALUES values, all distinct in the kind's order, that hold every second value of the pool, shuffled"""
    if kind == "int":
        more = np.arange(-3000, 3000, dtype=np.int64).astype(np.int32).view(np.uint32)
    else:
        more = np.arange(1, 6001, dtype=np.uint32) << np.uint32(12)   # positive floats
    some = np.asarray(pool, dtype=np.uint32)[::2]
    some = some[np.unique(fs.order_key(kind, some), return_index=True)[1]]
    more = more[~np.isin(fs.order_key(kind, more), fs.order_key(kind, pool))][: _lib.NRTGPU_MAX_SET_VALUES - len(some)]
    out = np.random.default_rng(4096).permutation(np.concatenate([more, some]))
    assert len(out) == _lib.NRTGPU_MAX_SET_VALUES == len(np.unique(fs.order_key(kind, out)))
    return out


def sweep_clauses(kind: str):
    pool = POOL[kind]
    order = np.argsort(fs.order_key(kind, pool), kind="stable")
    lo, hi = int(pool[order[1]]), int(pool[order[-2]])
    absent = 12345 if kind == "int" else 0x42F6E979   # 123.456: in no column
    out = {
        "exists": ("exists",),
        "range_full_span": ("range", kind, fs.KIND_MIN[kind], fs.KIND_MAX[kind]),
        "range_inner": ("range", kind, lo, hi),
        "range_single_value": ("range", kind, lo, lo),
        "range_lower_above_upper": ("range", kind, hi, lo),
        "set_one_value": ("in_set", kind, np.array([hi], np.uint32)),
        "set_absent_value": ("in_set", kind, np.array([absent], np.uint32)),
        "set_with_duplicates": ("in_set", kind, np.array([hi, lo, hi, absent, lo, lo], np.uint32)),
        "set_of_4096": ("in_set", kind, set_of_4096(kind, pool)),
        "set_whole_pool": ("in_set", kind, pool),
    }
    if kind == "float":
        out.update({
            "range_inf_to_inf": ("range", kind, NINF, PINF),            # drops the NaNs
            "range_nan_to_nan": ("range", kind, NAN, 0xFFC00001),       # any NaN is the canonical bound: exactly the NaN docs
            "range_zero_to_zero": ("range", kind, NZERO, PZERO),
            "set_negative_zero": ("in_set", kind, np.array([NZERO], np.uint32)),
            "set_positive_zero": ("in_set", kind, np.array([PZERO], np.uint32)),
            "set_nan_with_payload": ("in_set", kind, np.array([0x7FC00055], np.uint32)),   # a NaN no column holds: matches every NaN
        })
    return out


def check(name, g, n, mask_id, pairs):
    """build the mask of [(field, column, clause)] on the device; its words and count against the reference"""
    exp_words, exp_count = ref.mask_words(n, [(col, cl) for _, col, cl in pairs])
    count = g.set_mask_from_values(mask_id, [api_clause(field, cl) for field, _, cl in pairs])
    words = g.get_mask(mask_id)
    assert words.tolist() == exp_words.tolist(), f"{name}: the words"
    assert count == exp_count, f"{name}: out_count {count}, the reference counts {exp_count}"
    return exp_count


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("max_doc", MAX_DOCS)
def test_edge_sweep(ctx, max_doc, kind):
    """Word and sub-tile edges x both kinds x the three arities (and a column without a value) x every clause kind.  Under an
    all-accepting clause over the dense column the last partial word's padding must stay 0 (the count is max_doc)."""
    rng = np.random.default_rng(1000 * max_doc + (kind == "float"))
    columns = make_columns(rng, max_doc, kind)
    g = upload_columns(ctx, max_doc, kind, columns)
    try:
        before = g.device_bytes
        for cname, clause in sweep_clauses(kind).items():
            for aname, field in ARITIES.items():
                n_set = check(f"max_doc {max_doc}, {kind}, {aname}, {cname}", g, max_doc, 40, [(field, columns[aname], clause)])
                if aname == "dense" and cname in ("exists", "range_full_span", "set_whole_pool"):
                    assert n_set == max_doc
                    assert int(g.get_mask(40)[-1]) == ((1 << (((max_doc - 1) & 63) + 1)) - 1), "the padding of the last word"
                if aname == "no_values" or cname in ("range_lower_above_upper", "set_absent_value"):
                    assert n_set == 0
        if kind == "float" and max_doc >= 1023:   # the identities did decide something at these sizes
            nz, pz = (ref.mask_words(max_doc, [(columns["dense"], ("in_set", kind, np.array([b], np.uint32)))])[1] for b in (NZERO, PZERO))
            nans = ref.mask_words(max_doc, [(columns["dense"], ("range", kind, NAN, NAN))])[1]
            assert nz > 0 and pz > 0 and nans > 0
        assert g.device_bytes == before, "nothing stays resident behind a call"
    finally:
        g.release()


def test_four_clauses_over_columns_of_mixed_arity(ctx):
    n, kind = 2065, "int"
    rng = np.random.default_rng(77)
    pool = np.arange(-4, 5, dtype=np.int32).view(np.uint32)
    columns = make_columns(rng, n, kind, pool)
    g = upload_columns(ctx, n, kind, columns)
    bits = lambda *v: np.array(v, dtype=np.int32).view(np.uint32)   # noqa: E731
    try:
        four = [(DENSE, columns["dense"], ("range", kind, int(bits(-3)[0]), int(bits(3)[0]))), (MULTI, columns["multi"], ("in_set", kind, bits(0, 1, 2, -4, 2))),
                (SPARSE, columns["sparse"], ("exists",)), (MULTI, columns["multi"], ("range", kind, int(bits(-1)[0]), int(bits(4)[0])))]
        n_set = check("four clauses", g, n, 41, four)
        assert 0 < n_set < min(ref.mask_words(n, [(c, cl)])[1] for _, c, cl in four), "every clause narrowed the mask"
        for drop in range(4):   # and every order of three of them
            check(f"without clause {drop}", g, n, 41, four[drop + 1:] + four[:drop])
        assert check("one empty clause empties the mask", g, n, 41, four[:3] + [(NONE, columns["no_values"], ("exists",))]) == 0
        big = ("in_set", kind, set_of_4096(kind, pool))   # four sets of NRTGPU_MAX_SET_VALUES: all the LDS a call can ask for
        assert check("four full sets", g, n, 41, [(ARITIES[a], columns[a], big) for a in ("dense", "multi", "sparse", "dense")]) > 0
    finally:
        g.release()


def test_the_mask_ignores_live_docs(ctx):
    n, kind = 1500, "float"
    rng = np.random.default_rng(78)
    columns = make_columns(rng, n, kind)
    alive = rng.random(n) >= 0.3
    g = upload_columns(ctx, n, kind, columns, live=dsr.pack(alive))
    try:
        for aname in ("dense", "sparse", "multi"):
            n_set = check(f"deletes, {aname}", g, n, 42, [(ARITIES[aname], columns[aname], ("exists",))])
            kept = fs._bits(g.get_mask(42), n)
            assert (kept & ~alive).sum() > 0 and n_set > int((kept & alive).sum()), "deleted docs stay in the mask"
    finally:
        g.release()


def test_refusals_on_the_device(ctx):
    g = api.GpuSegment(ctx, 100, 0)
    g.add_doc_values(DENSE, "int", np.arange(100, dtype=np.int32))
    with pytest.raises(_lib.NrtGpuError) as e:
        g.set_mask_from_values(5, [VC.exists(DENSE)])
    assert e.value.code == _lib.NRTGPU_ERR_STATE
    g.seal()
    try:
        g.set_mask(5, np.array([5, 6], dtype=np.uint64))
        with pytest.raises(_lib.NrtGpuError) as e:
            g.set_mask_from_values(5, [VC.exists(DENSE), VC.exists(99)])
        assert e.value.code == _lib.NRTGPU_ERR_UNSUPPORTED and "99" in str(e.value)
        assert g.get_mask(5).tolist() == [5, 6], "a failed call leaves the previous mask untouched"
        with pytest.raises(_lib.NrtGpuError) as e:
            g.get_mask(6)
        assert e.value.code == _lib.NRTGPU_ERR_UNSUPPORTED
        assert g.set_mask_from_values(5, [VC.range_(DENSE, "int", 10, 19)]) == 10 and g.get_mask(5).tolist() == [0xFFC00, 0]
    finally:
        g.release()


# ---- the routes under a built mask ----------------------------------------------------------------------------------------------
RATING, TAGS, VEC, T_ALL, T_A, T_B = 7, 8, 3, 1, 2, 3
A, B, OTHER = 30, 31, 5


class Index:
    """Three leaves (1500, 700 and 40 docs, 5 % deletes) with postings, float vectors, a sparse int column `rating` in 0..9 and a
    multi-valued int column `tags`.  Mask A is built on the device from a clause, mask B holds the reference's words for it."""

    def __init__(self, ctx):
        rng = np.random.default_rng(31)
        self.corpus = fs.make_corpus([1500, 700, 40], {T_ALL: 1.0, T_A: 0.4, T_B: 0.25}, seed=9, delete_fraction=0.05)
        self.rating, self.tags, self.other, self.leaves = [], [], [], []
        for seg in self.corpus.segments:
            n = seg.max_doc
            docs = np.nonzero(rng.random(n) < 0.9)[0].astype(np.int32)
            self.rating.append(("single", docs, rng.integers(0, 10, size=len(docs)).astype(np.int32).view(np.uint32)))
            td = np.repeat(np.arange(n, dtype=np.int32), rng.choice([0, 1, 2, 4], size=n))
            self.tags.append(("multi", td, rng.integers(0, 30, size=len(td)).astype(np.int32).view(np.uint32)))
            self.other.append(dsr.pack(rng.random(n) < 0.7))
            g = api.GpuSegment(ctx, n, seg.doc_base)
            g.add_field_norms(0, seg.norms)
            g.add_terms(0, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
            g.add_vectors(VEC, rng.standard_normal((n, 16)).astype(np.float32))
            add_column(g, RATING, "int", self.rating[-1])
            add_column(g, TAGS, "int", self.tags[-1])
            g.seal()
            g.set_live_docs(seg.live_bits)
            g.set_mask(OTHER, self.other[-1])
            self.leaves.append(g)
        self.searcher = api.GpuIndexSearcher(ctx, self.leaves, api.IndexStatistics.from_corpus(self.corpus))
        self.queries = rng.standard_normal((4, 16)).astype(np.float32)

    def build(self, clauses, leaves=None):
        """clauses: [(field, columns per leaf, reference clause)] -> mask A on the device, mask B from the reference; the words agree"""
        total, self.masked = 0, set()   # masked: the mask's global docids
        for si, g in enumerate(leaves or self.leaves):
            words, count = ref.mask_words(g.max_doc, [(cols[si], cl) for _, cols, cl in clauses])
            self.masked |= set((np.nonzero(fs._bits(words, g.max_doc))[0] + g.doc_base).tolist())
            assert g.set_mask_from_values(A, [api_clause(field, cl) for field, _, cl in clauses]) == count
            assert g.get_mask(A).tolist() == words.tolist(), f"leaf {si}"
            g.set_mask(B, words)
            total += count
        return total

    def release(self):
        for g in self.leaves:
            g.release()


@pytest.fixture(scope="module")
def index(ctx):
    ix = Index(ctx)
    yield ix
    ix.release()


def i32(v) -> int:
    return int(np.array([v], np.int32).view(np.uint32)[0])


def same_topdocs(name, a, b):
    assert len(a) == len(b)
    for qi, (x, y) in enumerate(zip(a, b)):
        assert x.docs.tolist() == y.docs.tolist(), f"{name}[{qi}]: docs"
        assert x.scores.view(np.uint32).tolist() == y.scores.view(np.uint32).tolist(), f"{name}[{qi}]: score bits"
        assert (x.total_hits, x.relation_gte) == (y.total_hits, y.relation_gte), f"{name}[{qi}]: total hits"


def text_queries(mask, must_not=False):
    should = [(api.TermQuery(0, T_A),), (api.TermQuery(0, T_A), api.BoostQuery(api.TermQuery(0, T_B), 2.0)), (api.TermQuery(0, T_ALL), api.TermQuery(0, T_B))]
    if must_not:
        return [api.BooleanQuery(s, 1, (), (MF(mask),)) for s in should]
    return [api.BooleanQuery(s, 1, (MF(mask),)) for s in should]


def test_routes_under_a_built_mask_equal_the_routes_under_the_uploaded_words(index):
    sr = index.searcher
    rating_4_up = ("range", "int", i32(4), i32(9))
    n_mask = index.build([(RATING, index.rating, rating_4_up)])
    assert 0 < n_mask < index.corpus.n_docs
    top = [api.TopScoreDocCollectorManager(20)] * 3
    # the default route, the mask as FILTER and as MUST_NOT
    fa, fb = sr.search_batch(text_queries(A), top), sr.search_batch(text_queries(B), top)
    same_topdocs("filter", fa, fb)
    na, nb = sr.search_batch(text_queries(A, True), top), sr.search_batch(text_queries(B, True), top)
    same_topdocs("must_not", na, nb)
    for x, m in zip(fa, na):   # the mask decided the hits
        assert len(x.docs) == 20 and set(x.docs.tolist()) <= index.masked and len(m.docs) == 20 and not set(m.docs.tolist()) & index.masked
    # a float knn search with the pre-filter
    ka, kb = sr.knn_search(VEC, "dot_product", index.queries, 25, filter=MF(A)), sr.knn_search(VEC, "dot_product", index.queries, 25, filter=MF(B))
    same_topdocs("knn", ka, kb)
    assert all(len(x.docs) == 25 and set(x.docs.tolist()) <= index.masked and x.total_hits <= n_mask for x in ka)
    # a text sorted search
    sort = [api.SortField(RATING, "int", True, -1)] * 3
    sa, sb = api.search_sorted_batch(sr, text_queries(A), top, sort), api.search_sorted_batch(sr, text_queries(B), top, sort)
    for qi, (x, y) in enumerate(zip(sa, sb)):
        assert (x.docs.tolist(), x.value_bits.tolist(), x.total_hits, x.relation_gte) == (y.docs.tolist(), y.value_bits.tolist(), y.total_hits, y.relation_gte), qi
        assert len(x.docs) == 20 and int(x.values.min()) >= 4
    # a doc-set sorted search: the range INLINE against the same query with the built mask and no range
    one = [api.TopScoreDocCollectorManager(50)]
    for reverse in (False, True):
        s = [api.SortField(RATING, "int", reverse, 0)]
        inline = api.search_docset_sorted_batch(sr, [api.DocSetQuery((MF(OTHER),), (), (api.RangeClause(RATING, "int", 4, 9),))], one, s)[0]
        masked = api.search_docset_sorted_batch(sr, [api.DocSetQuery((MF(OTHER), MF(A)))], one, s)[0]
        assert (inline.docs.tolist(), inline.value_bits.tolist(), inline.total_hits, inline.relation_gte) == \
            (masked.docs.tolist(), masked.value_bits.tolist(), masked.total_hits, masked.relation_gte)
        assert 0 < masked.total_hits < n_mask
    # a doc-set terms count with the mask among more_filters
    coll = [api.TermsCollector(TAGS, 10)]
    ca = api.count_docset_terms_batch(sr, [api.DocSetQuery((MF(OTHER), MF(A)))], coll, 64)[0]
    cb = api.count_docset_terms_batch(sr, [api.DocSetQuery((MF(OTHER), MF(B)))], coll, 64)[0]
    assert (ca.value_bits.tolist(), ca.counts.tolist(), ca.total_hits, ca.hits_with_value, ca.overflowed) == \
        (cb.value_bits.tolist(), cb.counts.tolist(), cb.total_hits, cb.hits_with_value, cb.overflowed)
    assert ca.total_hits == masked.total_hits and len(ca.counts) > 0


def test_in_set_and_exists_masks_over_the_multi_valued_column_on_the_routes(index):
    sr = index.searcher
    tags = ("in_set", "int", np.array([3, 7, 7, 11, 29, 1000], np.int32).view(np.uint32))
    n_mask = index.build([(TAGS, index.tags, tags), (RATING, index.rating, ("exists",))])
    assert 0 < n_mask < index.corpus.n_docs
    top = [api.TopScoreDocCollectorManager(20)] * 3
    same_topdocs("filter", sr.search_batch(text_queries(A), top), sr.search_batch(text_queries(B), top))
    same_topdocs("knn", sr.knn_search(VEC, "cosine", index.queries, 10, filter=MF(A)), sr.knn_search(VEC, "cosine", index.queries, 10, filter=MF(B)))


def test_lifecycle_rebuild_fork_drop(index):
    sr = index.searcher
    top = [api.TopScoreDocCollectorManager(20)]
    q = [api.BooleanQuery((api.TermQuery(0, T_ALL),), 1, (MF(A),))]
    low, high = ("range", "int", i32(0), i32(2)), ("range", "int", i32(7), i32(9))
    index.build([(RATING, index.rating, low)])
    first = sr.search_batch(q, top)[0]
    index.build([(RATING, index.rating, high)])   # the same id, another clause: the accept set combined from the old words is gone
    second = sr.search_batch(q, top)[0]
    same_topdocs("rebuilt", [second], sr.search_batch([api.BooleanQuery((api.TermQuery(0, T_ALL),), 1, (MF(B),))], top))
    assert first.total_hits > 0 and second.total_hits > 0 and not set(first.docs.tolist()) & set(second.docs.tolist())
    # a fork builds its own A over the shared column; the parent's stays
    forks = [g.fork(seg.live_bits) for g, seg in zip(index.leaves, index.corpus.segments)]
    try:
        with pytest.raises(_lib.NrtGpuError):
            forks[0].get_mask(A)
        parent_words = [g.get_mask(A).tolist() for g in index.leaves]
        index.build([(RATING, index.rating, low)], leaves=forks)
        assert [g.get_mask(A).tolist() for g in index.leaves] == parent_words
        fsr = api.GpuIndexSearcher(index.searcher.ctx, forks, api.IndexStatistics.from_corpus(index.corpus))
        same_topdocs("fork", fsr.search_batch(q, top), [first])
        same_topdocs("parent", sr.search_batch(q, top), [second])
    finally:
        for f in forks:
            f.release()
    # dropped like any mask: a query that names it is refused, as it is today
    for g in index.leaves:
        g.set_mask(A, None)
    assert sr.supported(q[0], top[0]) is False
    with pytest.raises(_lib.NrtGpuError) as e:
        sr.search_batch(q, top)
    assert e.value.code == _lib.NRTGPU_ERR_UNSUPPORTED


# ---- seeded fuzz ---------------------------------------------------------------------------------------------------------------
def fuzz_clause(rng, kind, pool):
    which = rng.integers(4)
    if which == 0:
        return ("exists",)
    if which == 1:
        lo, hi = rng.choice(pool, size=2)
        if rng.random() < 0.7 and fs.order_key(kind, [lo])[0] > fs.order_key(kind, [hi])[0]:
            lo, hi = hi, lo
        return ("range", kind, int(lo), int(hi))
    m = int(rng.choice([1, 2, 7, 100]))
    listed = rng.choice(pool, size=m)
    if which == 3:   # members no column holds beside the pool's
        listed = np.concatenate([listed, rng.integers(0, 2**32, size=m, dtype=np.uint64).astype(np.uint32)])
    return ("in_set", kind, listed.astype(np.uint32))


@pytest.mark.parametrize("seed", range(40))
def test_seeded_fuzz(ctx, seed):
    rng = np.random.default_rng(52_000 + seed)
    kind = ("int", "float")[seed % 2]
    n = int(rng.choice([1, 64, 65, 700, 1024, 1025, 3000, 5000]))
    pool = POOL[kind] if rng.random() < 0.5 else np.unique(rng.integers(0, 2**32, size=int(rng.choice([3, 40])), dtype=np.uint64).astype(np.uint32))
    columns = make_columns(rng, n, kind, pool)
    g = upload_columns(ctx, n, kind, columns)
    names = list(ARITIES)[:3]
    try:
        for trial in range(6):
            pairs = []
            for _ in range(int(rng.integers(1, 5))):
                aname = names[int(rng.integers(3))]
                pairs.append((ARITIES[aname], columns[aname], fuzz_clause(rng, kind, pool)))
            check(f"seed {seed} (rng {52_000 + seed}), trial {trial}, max_doc {n}, {kind}: {[(f, cl) for f, _, cl in pairs]}", g, n, 43, pairs)
    finally:
        g.release()
