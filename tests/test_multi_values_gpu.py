"""Multi-valued doc value columns (nrtgpu_segment_add_doc_values_multi) under the terms counts and the doc-set range clauses,
through the C ABI on the device, against tests/_multi_values_ref.py.  Every comparison is exact equality of every output field.
The shapes are the sort tests' smallest (leaves of 3000 / 1500 / 40 docs, 1 % deletes).  Needs a real MI355X."""
import numpy as np
import pytest

from nrtsearch_amd import _lib, api, synth

from tests import _docset_ref as dsr
from tests import _field_sort_ref as fs
from tests import _multi_values_ref as mref
from tests import _terms_count_ref as tcr
from tests import test_docset_gpu as dg   # its pools of value bits, doc sets, the fourteen range sets and the comparisons

pytestmark = pytest.mark.gpu
ALL = dsr.ALL
T = {t: api.TermQuery(0, t) for t in (ALL, 2, 3, 4, 99)}
TERMS = {ALL: 1.0, 2: 0.3, 3: 0.2, 4: 0.5}
# the sort tests' eight shapes over this corpus's terms: (name, query, clauses, clauses a hit matches at least, reads the masks)
QUERIES = [
    ("term", T[4], (4,), 1, False),
    ("or3", api.BooleanQuery((T[4], T[2], T[3])), (4, 2, 3), 1, False),
    ("msm2of3", api.BooleanQuery((T[4], T[2], T[3]), 2), (4, 2, 3), 2, False),
    ("must2", api.BooleanQuery((), 0, (), (), (T[4], T[2])), (4, 2), 2, False),
    ("masks", api.BooleanQuery((T[4], T[2], T[3]), 1, (api.MaskFilter(5),), (api.MaskFilter(6),)), (4, 2, 3), 1, True),
    ("nowhere", T[99], (99,), 1, False),
    ("msm2_dup", api.BooleanQuery((T[2], T[2], T[3]), 2), (2, 2, 3), 2, False),
    ("must3_dup", api.BooleanQuery((), 0, (), (), (T[4], T[4], T[2])), (4, 4, 2), 3, False),
]
SIZES = (3000, 1500, 40)
KINDS = ("int", "float")
I5, F5, IE, FE = dg.I5, dg.F5, dg.IE, dg.FE
# multi-valued columns: (kind, name) -> field id.  "five" and "edge" carry the doc-set tests' field ids: their range sets name them.
NAMES = ("mixed", "one", "sparse", "dup", "holes", "edge", "five")
MULTI = {(k, n): (dg.FIELD[(k, n)] if n in ("five", "edge") else 60 + 10 * ki + ni) for ki, k in enumerate(KINDS) for ni, n in enumerate(NAMES)}
SINGLE = {("int", "one"): 90, ("float", "one"): 91, ("int", "sort"): 92, ("float", "sort"): 93, ("int", "count"): 94, ("float", "count"): 95}


def _spread(rng, size, per_doc, pool):
    docs = np.repeat(np.arange(size, dtype=np.int32), per_doc)
    return docs, rng.choice(pool, size=len(docs)).astype(np.uint32)


def multi_columns(kind):
    """name -> per leaf None or (value_docs, value bits).  (a) mixed: 0..3 values per doc; (b) one: exactly one per doc; (c) sparse:
    mostly empty, a doc of 70 values and one of 300, docs 63, 64, 1023 and every leaf's LAST doc; (d) dup: the same value three
    times in a doc; (e) holes: n_values == 0 on leaf 1, absent from leaf 2; (f) edge: the edge values, 0..3 per doc."""
    rng = np.random.default_rng(11 if kind == "int" else 12)
    many, five, edge = dg.POOLS[(kind, "many")], dg.POOLS[(kind, "five")], dg.POOLS[(kind, "edge")]
    cols = {}
    cols["mixed"] = [_spread(rng, n, rng.integers(0, 4, size=n), many) for n in SIZES]
    cols["one"] = [_spread(rng, n, np.ones(n, dtype=np.int64), many) for n in SIZES]
    sparse = []
    for n in SIZES:
        per = np.zeros(n, dtype=np.int64)
        per[n - 1] = 2
        if n == 3000:
            per[[63, 64, 1023]] = (1, 2, 1)
            per[100], per[2000] = 70, 300
        docs = np.repeat(np.arange(n, dtype=np.int32), per)
        vals = rng.choice(five, size=len(docs)).astype(np.uint32)
        if n == 3000:   # the long docs: rising values, so that a range keeps a doc by its LAST value alone
            vals[docs == 100] = many[:70]
            vals[docs == 2000] = many[100:400]
        sparse.append((docs, vals))
    cols["sparse"] = sparse
    dup = []
    for n in SIZES:
        per = np.where(np.arange(n) % 7 == 0, 3, 1)
        docs, vals = _spread(rng, n, per, five)
        first = np.searchsorted(docs, np.arange(0, n, 7))
        vals[first + 1] = vals[first]
        vals[first + 2] = vals[first]
        dup.append((docs, vals))
    cols["dup"] = dup
    cols["holes"] = [_spread(rng, 3000, rng.integers(0, 3, size=3000), five), (np.zeros(0, np.int32), np.zeros(0, np.uint32)), None]
    cols["edge"] = [_spread(rng, n, rng.integers(0, 4, size=n), edge) for n in SIZES]
    cols["five"] = [_spread(rng, n, rng.integers(0, 4, size=n), five) for n in SIZES]
    return cols


def single_columns(kind, multi):
    rng = np.random.default_rng(21 if kind == "int" else 22)
    d0 = np.nonzero(rng.random(3000) < 0.8)[0].astype(np.int32)
    return {"one": [(None, c[1]) for c in multi["one"]],   # (b): the same values, single-valued
            "sort": [(d0, rng.choice(dg.POOLS[(kind, "edge")], size=len(d0))), (None, rng.choice(dg.POOLS[(kind, "edge")], size=1500)), None],
            "count": [(d0, rng.choice(dg.POOLS[(kind, "five")], size=len(d0))), (None, rng.choice(dg.POOLS[(kind, "five")], size=1500)), None]}


@pytest.fixture(scope="module", autouse=True)
def two_column_postings():
    """The text routes over a column refuse packed postings: the contexts here keep the two-column layout whatever the suite runs under."""
    mp = pytest.MonkeyPatch()
    mp.delenv("NRTGPU_PACKED_POSTINGS", raising=False)
    yield
    mp.undo()


@pytest.fixture(scope="module")
def ctx(two_column_postings):
    c = api.GpuContext(device_id=0, max_batch=256)
    yield c
    c.close()


same_docs, same_counts, release = dg.same_docs, dg.same_counts, dg.release


class Index:
    def __init__(self, ctx, corpus):
        self.corpus = corpus
        self.multi = {(k, n): cols for k in KINDS for n, cols in multi_columns(k).items()}
        self.single = {(k, n): cols for k in KINDS for n, cols in single_columns(k, {n2: self.multi[(k, n2)] for n2 in NAMES}).items()}
        self.masks = {mid: [synth.random_mask(seg.max_doc, dens, 40 * mid + si) for si, seg in enumerate(corpus.segments)]
                      for mid, dens in dg.MASK_DENSITY.items()}
        self.accept = [synth.accept_words(seg, self.masks[5][si], self.masks[6][si]) for si, seg in enumerate(corpus.segments)]
        self.leaves = []
        for si, seg in enumerate(corpus.segments):
            g = api.GpuSegment(ctx, seg.max_doc, seg.doc_base)
            g.add_field_norms(0, seg.norms)
            g.add_terms(0, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
            for key, cols in self.multi.items():
                if cols[si] is not None:
                    g.add_doc_values_multi(MULTI[key], key[0], cols[si][1], cols[si][0])
            for key, cols in self.single.items():
                if cols[si] is not None:
                    g.add_doc_values(SINGLE[key], key[0], np.asarray(cols[si][1], dtype=np.uint32), cols[si][0])
            g.seal()
            g.set_live_docs(seg.live_bits)
            for mid, words in self.masks.items():
                g.set_mask(mid, words[si])
            self.leaves.append(g)
        self.searcher = api.GpuIndexSearcher(ctx, self.leaves, api.IndexStatistics.from_corpus(corpus))
        self._hits = {}

    # ---- text queries
    def text_hits(self, shape, live=None):
        _, _, clauses, need, masked = shape
        return mref.text_hits(self.corpus, clauses, need, accept=self.accept if masked else None, live=live)

    # ---- doc sets whose range clauses name MULTI-VALUED columns (mrs) and single-valued ones (srs): [(key, lower bits, upper bits)]
    def hits(self, ds_name, mrs=(), srs=(), live=None):
        memo = (ds_name, tuple(mrs), tuple(srs), None if live is None else id(live))
        if memo not in self._hits:
            f, mn = dg.DOCSETS[ds_name]
            filters = [self.masks[m] for m in f] + [mref.any_in_range(self.corpus, key[0], self.multi[key], lo, hi) for key, lo, hi in mrs]
            self._hits[memo] = dsr.hit_set(self.corpus, filters, [self.masks[m] for m in mn], [(key[0], self.single[key], lo, hi) for key, lo, hi in srs], live)
        return self._hits[memo]

    @staticmethod
    def query(ds_name, mrs=(), srs=()):
        f, mn = dg.DOCSETS[ds_name]
        clauses = [api.RangeClause(MULTI[key], key[0], fs.value_of(key[0], lo), fs.value_of(key[0], hi)) for key, lo, hi in mrs]
        clauses += [api.RangeClause(SINGLE[key], key[0], fs.value_of(key[0], lo), fs.value_of(key[0], hi)) for key, lo, hi in srs]
        return api.DocSetQuery(tuple(api.MaskFilter(m) for m in f), tuple(api.MaskFilter(m) for m in mn), tuple(clauses))

    @staticmethod
    def sort(kind, reverse, missing_bits):
        return api.SortField(SINGLE[(kind, "sort")], kind, reverse, fs.value_of(kind, missing_bits))

    @staticmethod
    def mcoll(key):
        return api.TermsCollector(MULTI[key], 10, True, key[0])

    @staticmethod
    def scoll(key):
        return api.TermsCollector(SINGLE[key], 10, True, key[0])


@pytest.fixture(scope="module")
def corpus_a():
    c = fs.make_corpus(SIZES, TERMS, seed=5, delete_fraction=0.01)
    assert all(seg.live_bits is not None for seg in c.segments)
    return c


@pytest.fixture(scope="module")
def ix(ctx, corpus_a):
    x = Index(ctx, corpus_a)
    yield x
    release(x.leaves)


def as_expected(tc):
    return (tc.value_bits, tc.counts, len(tc.counts), tc.total_hits, tc.hits_with_value, int(tc.overflowed))


# ---- counts -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_counts_under_the_eight_text_shapes(ix, kind):
    keys = [(kind, n) for n in NAMES]
    cases = [(key, q) for key in keys for q in QUERIES]
    before = ix.searcher.ctx.stats()
    got = api.count_terms_batch(ix.searcher, [q[1] for _, q in cases], [ix.mcoll(key) for key, _ in cases], 1024)
    after = ix.searcher.ctx.stats()
    assert after["scan_launches"] == before["scan_launches"] + 1 and after["maxscore_launches"] == before["maxscore_launches"]
    for (key, q), tc in zip(cases, got):
        exp = mref.count(ix.corpus, ix.text_hits(q), ix.multi[key], kind, 1024)
        same_counts(f"{key}_{q[0]}", tc, exp)
        assert exp[5] == 0 and (exp[3] == 0) == (q[0] == "nowhere")
    by = {(key[1], q[0]): tc for (key, q), tc in zip(cases, got)}
    assert by[("mixed", "or3")].hits_with_value > by[("mixed", "or3")].total_hits       # value instances, not docs
    assert by[("one", "or3")].hits_with_value == by[("one", "or3")].total_hits
    assert 0 < by[("sparse", "or3")].hits_with_value and by[("holes", "or3")].hits_with_value < by[("holes", "or3")].total_hits
    assert by[("dup", "or3")].hits_with_value > by[("dup", "or3")].total_hits
    # (b): the same values single-valued under another field: every output equal
    single = api.count_terms_batch(ix.searcher, [q[1] for q in QUERIES], [ix.scoll((kind, "one"))] * len(QUERIES), 1024)
    for q, tc in zip(QUERIES, single):
        same_counts(f"one_single_{q[0]}", by[("one", q[0])], as_expected(tc))
    # (f): three NaN payloads are one bucket, reported canonical and last; the zeros two buckets
    edge = by[("edge", "or3")]
    if kind == "float":
        assert edge.value_bits.tolist() == dg._f([-np.inf, -1.5, -0.0, 0.0, 1e-45, 3.25, np.inf]).tolist() + [dg.NAN]
    else:
        assert edge.values.tolist() == [fs.INT32_MIN, -1, 0, 1, fs.INT32_MAX]
    assert api.count_terms_supported(ix.searcher, QUERIES[2][1], ix.mcoll(keys[0]), 1024) is True


@pytest.mark.parametrize("kind", KINDS)
def test_counts_under_the_four_doc_sets(ix, kind):
    keys = [(kind, n) for n in NAMES]
    cases = [(key, ds) for key in keys for ds in dg.DOCSETS]
    got = api.count_docset_terms_batch(ix.searcher, [ix.query(ds) for _, ds in cases], [ix.mcoll(key) for key, _ in cases], 1024)
    assert api.GpuContext.last_diagnostics()["postings"] == 0
    for (key, ds), tc in zip(cases, got):
        exp = mref.count(ix.corpus, ix.hits(ds), ix.multi[key], kind, 1024)
        same_counts(f"{key}_{ds}", tc, exp)
        assert (exp[3] == 0) == (ds == "empty")
    by = {(key[1], ds): tc for (key, ds), tc in zip(cases, got)}
    # (c): the docs of 70 and 300 values, docs 63, 64, 1023 and the three last docs, unless deleted
    live = [fs._bits(seg.live_bits, seg.max_doc) for seg in ix.corpus.segments]
    want = sum(c for d, c in ((63, 1), (64, 2), (1023, 1), (100, 70), (2000, 300), (2999, 2)) if live[0][d]) + 2 * int(live[1][1499]) + 2 * int(live[2][39])
    assert by[("sparse", "all")].hits_with_value == want >= 300
    single = api.count_docset_terms_batch(ix.searcher, [ix.query(ds) for ds in dg.DOCSETS], [ix.scoll((kind, "one"))] * 4, 1024)
    for ds, tc in zip(dg.DOCSETS, single):
        same_counts(f"one_single_{ds}", by[("one", ds)], as_expected(tc))
    assert api.count_docset_terms_supported(ix.searcher, ix.query("masks"), ix.mcoll(keys[0]), 1024) is True


def test_the_overflow_boundary(ix):
    text, sets = [], []
    for kind in KINDS:
        for name in ("mixed", "edge", "dup"):
            key = (kind, name)
            d1 = mref.count(ix.corpus, ix.text_hits(QUERIES[1]), ix.multi[key], kind)[2]
            d2 = mref.count(ix.corpus, ix.hits("masks"), ix.multi[key], kind)[2]
            text += [(key, b) for b in (d1, d1 - 1, d1 + 1)]
            sets += [(key, b) for b in (d2, d2 - 1, d2 + 1)]
    got = api.count_terms_batch(ix.searcher, [QUERIES[1][1]] * len(text), [ix.mcoll(k) for k, _ in text], [b for _, b in text])
    for (key, b), tc in zip(text, got):
        same_counts(f"text_{key}_{b}", tc, mref.count(ix.corpus, ix.text_hits(QUERIES[1]), ix.multi[key], key[0], b))
    assert [int(tc.overflowed) for tc in got] == [0, 1, 0] * 6
    got = api.count_docset_terms_batch(ix.searcher, [ix.query("masks")] * len(sets), [ix.mcoll(k) for k, _ in sets], [b for _, b in sets])
    for (key, b), tc in zip(sets, got):
        same_counts(f"docset_{key}_{b}", tc, mref.count(ix.corpus, ix.hits("masks"), ix.multi[key], key[0], b))
    assert [int(tc.overflowed) for tc in got] == [0, 1, 0] * 6


# ---- 13 000 docs, about 3 values each over more than 8192 distinct values: the LDS probe bound, the straight-to-global path ------------
@pytest.fixture(scope="module")
def ix_b(ctx):
    n = 13_000
    corpus = fs.make_corpus([n], {ALL: 1.0, 4: 0.6}, seed=8)
    seg = corpus.segments[0]
    rng = np.random.default_rng(9)
    docs = np.repeat(np.arange(n, dtype=np.int32), rng.integers(1, 6, size=n))
    wide = rng.integers(0, 20_000, size=len(docs)).astype(np.int32)
    few = (wide % 5).astype(np.int32)
    g = api.GpuSegment(ctx, n, 0)
    g.add_field_norms(0, seg.norms)
    g.add_terms(0, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
    g.add_doc_values_multi(7, "int", wide, docs)
    g.add_doc_values_multi(8, "int", few, docs)
    g.add_doc_values(9, "int", (np.arange(n, dtype=np.int32) % 3))
    g.seal()
    searcher = api.GpuIndexSearcher(ctx, [g], api.IndexStatistics.from_corpus(corpus))
    columns = {7: [(docs, wide.view(np.uint32))], 8: [(docs, few.view(np.uint32))]}
    yield corpus, searcher, columns
    g.release()


def test_more_distinct_values_than_the_workgroup_table_takes(ix_b):
    corpus, searcher, columns = ix_b
    routes = (("text", mref.text_hits(corpus, (4,)), lambda cols, bounds: api.count_terms_batch(searcher, [T[4]] * len(cols), [api.TermsCollector(c, 10) for c in cols], bounds)),
              ("docset", dsr.hit_set(corpus), lambda cols, bounds: api.count_docset_terms_batch(searcher, [api.DocSetQuery()] * len(cols), [api.TermsCollector(c, 10) for c in cols], bounds)))
    for name, hits, run in routes:
        distinct = mref.count(corpus, hits, columns[7], "int")[2]
        assert distinct > 8192
        for bound, over in ((4, 1), (32_768, 0)):
            exp = mref.count(corpus, hits, columns[7], "int", bound)
            assert exp[5] == over
            same_counts(f"{name}_alone_{bound}", run([7], [bound])[0], exp)
        # in a batch whose other queries stay exact (query 2 counts a SINGLE-valued column beside the multi-valued ones)
        cols, bounds = [7, 8, 9, 7, 8], [4, 8, 4, 32_768, 5]
        got = run(cols, bounds)
        single9 = [(None, (np.arange(13_000, dtype=np.int32) % 3).view(np.uint32))]
        exps = [mref.count(corpus, hits, columns[c], "int", b) if c != 9 else
                tcr.count(corpus, single9, "int", (4,) if name == "text" else (ALL,), 1, b) for c, b in zip(cols, bounds)]
        assert [e[5] for e in exps] == [1, 0, 0, 0, 0]
        for i, (tc, exp) in enumerate(zip(got, exps)):
            same_counts(f"{name}_batch_{i}", tc, exp)


# ---- 300 000 docs cut into several items whose counts meet in one table -----------------------------------------------------------------
def test_several_items_share_the_query_table(ctx):
    n = 300_000
    corpus = fs.make_corpus([n], {ALL: 1.0}, seed=10)
    seg = corpus.segments[0]
    docs = np.repeat(np.arange(n, dtype=np.int32), 3)
    vals = ((docs.astype(np.int64) * 7 + np.tile(np.arange(3), n) * 331) % 1000).astype(np.int32)
    g = api.GpuSegment(ctx, n, 0)
    try:
        g.add_field_norms(0, seg.norms)
        g.add_terms(0, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
        g.add_doc_values_multi(7, "int", vals, docs)
        g.seal()
        searcher = api.GpuIndexSearcher(ctx, [g], api.IndexStatistics.from_corpus(corpus))
        cols = [(docs, vals.view(np.uint32))]
        hits = dsr.hit_set(corpus)
        half = api.DocSetQuery((), (), (api.RangeClause(7, "int", 0, 9),))
        half_hits = dsr.hit_set(corpus, [mref.any_in_range(corpus, "int", cols, 0, 9)])
        text = api.count_terms_batch(searcher, [T[ALL], T[ALL]], [api.TermsCollector(7, 10)] * 2, [1024, 999])
        assert api.GpuContext.last_diagnostics()["items_scan"] >= 4
        sets = api.count_docset_terms_batch(searcher, [api.DocSetQuery(), api.DocSetQuery(), half], [api.TermsCollector(7, 10)] * 3, [1024, 999, 1024])
        assert api.GpuContext.last_diagnostics()["items_scan"] >= 6
        for name, tc, h, b in (("text", text[0], hits, 1024), ("text_999", text[1], hits, 999), ("docset", sets[0], hits, 1024), ("docset_999", sets[1], hits, 999),
                               ("docset_half", sets[2], half_hits, 1024)):
            same_counts(name, tc, mref.count(corpus, h, cols, "int", b))
        assert len(text[0].counts) == 1000 and text[0].hits_with_value == 3 * n and text[1].overflowed and text[1].total_hits == n
        assert 0 < sets[2].total_hits < n
    finally:
        g.release()


# ---- ranges -----------------------------------------------------------------------------------------------------------------------------
def clause_sets(kind):
    """the fourteen range sets of the doc-set tests; every clause names the MULTI-VALUED column of its key"""
    return dg.range_sets(dg.EDGE[kind])


@pytest.mark.parametrize("kind", KINDS)
def test_sorted_by_a_single_valued_column_under_multi_valued_clauses(ix, kind):
    sets = clause_sets(kind)
    assert len(sets) == 14
    cases = [(ds, rn, k, rev) for ds in dg.DOCSETS for rn in sets for rev in (False, True) for k in ((10,) if ds != "all" else (10, 1024))]
    mb = fs.KIND_MAX[kind]
    got = dg.sorted_batch(ix.searcher, [ix.query(ds, sets[rn]) for ds, rn, _, _ in cases], [api.TopScoreDocCollectorManager(k) for _, _, k, _ in cases],
                          [ix.sort(kind, rev, mb) for _, _, _, rev in cases])
    totals = {}
    for (ds, rn, k, rev), td in zip(cases, got):
        exp = dsr.search(ix.corpus, ix.hits(ds, sets[rn]), ix.single[(kind, "sort")], kind, k, rev, mb)
        same_docs(f"{kind}_{ds}_{rn}_k{k}_rev{int(rev)}", td, exp)
        totals[(ds, rn)] = exp[2]
    live = sum(fs.live_count(s) for s in ix.corpus.segments)
    assert totals[("all", "none")] == live and all(totals[(ds, rn)] == 0 for ds in dg.DOCSETS for rn in ("empty_range", "zeros_reversed"))
    assert 0 < totals[("all", "full_int")] < live and 0 < totals[("all", "up_to_inf")] < totals[("all", "full_float")] < live   # docs without a value fail
    assert all(totals[("all", rn)] > 0 for rn in ("nan_only", "neg_zero_only", "from_pos_zero", "int_min_only", "int_max_only", "four_over_three"))
    assert api.docset_sorted_supported(ix.searcher, ix.query("masks", sets["four_over_three"]), api.TopScoreDocCollectorManager(10), ix.sort(kind, False, 0)) is True


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("reverse", [False, True])
def test_pages_of_7_equal_one_page_of_70(ix, kind, reverse):
    rs = clause_sets(kind)["on_another"]
    q, hits, mb = ix.query("filter", rs), ix.hits("filter", rs), int(fs.VALUES[kind][2])
    sort, cols = ix.sort(kind, reverse, mb), ix.single[(kind, "sort")]
    full = api.search_docset_sorted_batch(ix.searcher, [q], [api.TopScoreDocCollectorManager(70)], [sort])[0]
    same_docs(f"{kind}_page70", full, dsr.search(ix.corpus, hits, cols, kind, 70, reverse, mb))
    after, docs = None, []
    for page in range(10):
        got = api.search_docset_sorted_batch(ix.searcher, [q], [api.TopScoreDocCollectorManager(7)], [sort], [after])[0]
        exp = dsr.search(ix.corpus, hits, cols, kind, 7, reverse, mb, after=None if after is None else (after.doc, fs.bits_of(kind, after.value)))
        same_docs(f"{kind}_page7_{page}", got, exp)
        assert got.total_hits == full.total_hits
        docs += got.docs.tolist()
        after = api.FieldDoc(int(got.docs[-1]), fs.value_of(kind, int(got.value_bits[-1])))
    assert docs == full.docs.tolist()


@pytest.mark.parametrize("kind", KINDS)
def test_counted_by_either_arity_under_multi_valued_clauses(ix, kind):
    sets = clause_sets(kind)
    cases = [(ds, rn) for ds in dg.DOCSETS for rn in sets]
    queries = [ix.query(ds, sets[rn]) for ds, rn in cases]
    multi = dg.counted_batch(ix.searcher, queries, [ix.mcoll((kind, "mixed"))] * len(cases), [1024] * len(cases))
    single = dg.counted_batch(ix.searcher, queries, [ix.scoll((kind, "count"))] * len(cases), [1024] * len(cases))
    for (ds, rn), m, s in zip(cases, multi, single):
        hits = ix.hits(ds, sets[rn])
        same_counts(f"multi_{ds}_{rn}", m, mref.count(ix.corpus, hits, ix.multi[(kind, "mixed")], kind, 1024))
        same_counts(f"single_{ds}_{rn}", s, tcr.count(ix.corpus, ix.single[(kind, "count")], kind, (ALL,), 1, 1024, accept=hits))
        assert m.total_hits == s.total_hits


def test_one_single_valued_and_one_multi_valued_clause_and_a_doc_kept_by_its_last_value(ix):
    many = dg.POOLS[("int", "many")]
    five_lo, five_hi = int(dg._i([3])[0]), int(dg._i([9])[0])
    edge_lo, edge_hi = int(dg._i([-1])[0]), int(dg._i([fs.INT32_MAX])[0])
    mrs, srs = [(I5, five_lo, five_hi)], [(("int", "sort"), edge_lo, edge_hi)]
    last70, last300 = [(("int", "sparse"), int(many[69]), int(many[69]))], [(("int", "sparse"), int(many[399]), int(many[399]))]
    queries = [ix.query("all", mrs, srs), ix.query("masks", mrs, srs), ix.query("all", last70), ix.query("all", last300)]
    hit_sets = [ix.hits("all", mrs, srs), ix.hits("masks", mrs, srs), ix.hits("all", last70), ix.hits("all", last300)]
    got = api.search_docset_sorted_batch(ix.searcher, queries, [api.TopScoreDocCollectorManager(10)] * 4, [ix.sort("int", False, 0)] * 4)
    cnt = api.count_docset_terms_batch(ix.searcher, queries, [ix.mcoll(("int", "sparse"))] * 4, 1024)
    for i, (td, tc, hits) in enumerate(zip(got, cnt, hit_sets)):
        same_docs(f"mixed_clauses_{i}", td, dsr.search(ix.corpus, hits, ix.single[("int", "sort")], "int", 10, False, 0))
        same_counts(f"mixed_clauses_{i}", tc, mref.count(ix.corpus, hits, ix.multi[("int", "sparse")], "int", 1024))
    live0 = fs._bits(ix.corpus.segments[0].live_bits, 3000)
    assert 0 < got[1].total_hits < got[0].total_hits < min(tc.total_hits for tc in api.count_docset_terms_batch(
        ix.searcher, [ix.query("all", mrs), ix.query("all", (), srs)], [ix.mcoll(("int", "sparse"))] * 2, 1024))   # each clause narrows
    assert got[2].docs.tolist() == ([100] if live0[100] else []) and got[3].docs.tolist() == ([2000] if live0[2000] else [])
    assert cnt[2].hits_with_value == 70 * int(live0[100]) and cnt[3].hits_with_value == 300 * int(live0[2000])


# ---- mixed batches: the dispatch ----------------------------------------------------------------------------------------------------------
def test_a_batch_that_mixes_arities_equals_the_separate_calls(ix):
    shape = QUERIES[1]
    # text: query 0 counts a single-valued column, query 1 a multi-valued one
    both = api.count_terms_batch(ix.searcher, [shape[1]] * 2, [ix.scoll(("int", "count")), ix.mcoll(("int", "mixed"))], 1024)
    alone = [api.count_terms_batch(ix.searcher, [shape[1]], [c], 1024)[0] for c in (ix.scoll(("int", "count")), ix.mcoll(("int", "mixed")))]
    for i in range(2):
        same_counts(f"text_{i}", both[i], as_expected(alone[i]))
    same_counts("text_single", both[0], tcr.count(ix.corpus, ix.single[("int", "count")], "int", shape[2], shape[3], 1024))
    same_counts("text_multi", both[1], mref.count(ix.corpus, ix.text_hits(shape), ix.multi[("int", "mixed")], "int", 1024))
    # doc sets: query 0 names single-valued columns only, query 1 multi-valued ones
    rs = [(I5, int(dg._i([3])[0]), int(dg._i([9])[0]))]
    srs = [(("int", "count"), int(dg._i([3])[0]), int(dg._i([9])[0]))]
    qs = [ix.query("filter", (), srs), ix.query("filter", rs)]
    hs = [ix.hits("filter", (), srs), ix.hits("filter", rs)]
    colls = [ix.scoll(("int", "count")), ix.mcoll(("int", "mixed"))]
    both = api.count_docset_terms_batch(ix.searcher, qs, colls, 1024)
    alone = [api.count_docset_terms_batch(ix.searcher, [q], [c], 1024)[0] for q, c in zip(qs, colls)]
    for i in range(2):
        same_counts(f"docset_{i}", both[i], as_expected(alone[i]))
    same_counts("docset_single", both[0], tcr.count(ix.corpus, ix.single[("int", "count")], "int", (ALL,), 1, 1024, accept=hs[0]))
    same_counts("docset_multi", both[1], mref.count(ix.corpus, hs[1], ix.multi[("int", "mixed")], "int", 1024))
    sorts = [ix.sort("int", True, 0)] * 2
    both = api.search_docset_sorted_batch(ix.searcher, qs, [api.TopScoreDocCollectorManager(50)] * 2, sorts)
    alone = [api.search_docset_sorted_batch(ix.searcher, [q], [api.TopScoreDocCollectorManager(50)], sorts[:1])[0] for q in qs]
    for i in range(2):
        same_docs(f"sorted_{i}", both[i], (alone[i].docs, alone[i].value_bits, alone[i].total_hits, alone[i].relation_gte))
        same_docs(f"sorted_ref_{i}", both[i], dsr.search(ix.corpus, hs[i], ix.single[("int", "sort")], "int", 50, True, 0))


def test_a_batch_of_single_valued_queries_only_is_the_single_valued_route(ix):
    """The index holds multi-valued columns, the call names none: it launches the kernels it always launched and answers as they do."""
    for kind in KINDS:
        key = (kind, "count")
        got = api.count_terms_batch(ix.searcher, [q[1] for q in QUERIES], [ix.scoll(key)] * len(QUERIES), 1024)
        for q, tc in zip(QUERIES, got):
            same_counts(f"text_{kind}_{q[0]}", tc, tcr.count(ix.corpus, ix.single[key], kind, q[2], q[3], 1024, accept=ix.accept if q[4] else None))
        srs = [(key, int(dg.POOLS[(kind, "five")][0]), int(dg.POOLS[(kind, "five")][0]))]
        got = api.count_docset_terms_batch(ix.searcher, [ix.query(ds, (), srs) for ds in dg.DOCSETS], [ix.scoll(key)] * 4, 1024)
        for ds, tc in zip(dg.DOCSETS, got):
            same_counts(f"docset_{kind}_{ds}", tc, tcr.count(ix.corpus, ix.single[key], kind, (ALL,), 1, 1024, accept=ix.hits(ds, (), srs)))
            assert len(tc.counts) <= 1


# ---- also -------------------------------------------------------------------------------------------------------------------------------
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
        key, rs = ("float", "mixed"), clause_sets("float")["four_over_three"]
        hits = ix.hits("masks", rs, (), live=lives)
        cnt = api.count_docset_terms_batch(searcher, [ix.query("masks", rs)], [ix.mcoll(key)], 1024)[0]
        same_counts("fork_docset", cnt, mref.count(corpus, hits, ix.multi[key], "float", 1024))
        td = api.search_docset_sorted_batch(searcher, [ix.query("masks", rs)], [api.TopScoreDocCollectorManager(100)], [ix.sort("float", True, 0)])[0]
        same_docs("fork_sorted", td, dsr.search(corpus, hits, ix.single[("float", "sort")], "float", 100, True, 0))
        txt = api.count_terms_batch(searcher, [QUERIES[1][1]], [ix.mcoll(key)], 1024)[0]
        same_counts("fork_text", txt, mref.count(corpus, ix.text_hits(QUERIES[1], live=lives), ix.multi[key], "float", 1024))
        parent = api.count_terms_batch(ix.searcher, [QUERIES[1][1]], [ix.mcoll(key)], 1024)[0]
        assert parent.total_hits > txt.total_hits > 0 and parent.hits_with_value > txt.hits_with_value > 0
    finally:
        release(forks)


def test_device_bytes_grow_by_the_layout(ctx):
    g = api.GpuSegment(ctx, 2500, 0)
    try:
        before = g.device_bytes
        docs = np.array([0, 0, 7, 2499, 2499, 2499], dtype=np.int32)
        g.add_doc_values_multi(7, "int", np.arange(6, dtype=np.int32), docs)
        start_bytes = (3 * 1024 + 1) * 4   # one entry per doc, padded to whole 1024-doc sub-tiles, plus one
        assert g.device_bytes == before + start_bytes + 6 * 4
        g.add_doc_values_multi(8, "float", np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.int32))   # a valid column: nobody has a value
        assert g.device_bytes == before + 2 * start_bytes + 6 * 4
    finally:
        g.release()


@pytest.mark.parametrize("flag", [_lib.NRTGPU_FLAG_PACKED_POSTINGS, _lib.NRTGPU_FLAG_NO_FIXED_POINT])
def test_doc_set_calls_under_the_two_context_flags(flag, corpus_a):
    c = api.GpuContext(device_id=0, max_batch=16, flags=flag)
    x = None
    try:
        x = Index(c, corpus_a)
        rs = clause_sets("float")["four_over_three"]
        q, hits = x.query("masks", rs), x.hits("masks", rs)
        td = api.search_docset_sorted_batch(x.searcher, [q], [api.TopScoreDocCollectorManager(50)], [x.sort("float", True, 0)])[0]
        same_docs(f"flag{flag}", td, dsr.search(x.corpus, hits, x.single[("float", "sort")], "float", 50, True, 0))
        cnt = api.count_docset_terms_batch(x.searcher, [q], [x.mcoll(("float", "edge"))], 64)[0]
        same_counts(f"flag{flag}", cnt, mref.count(x.corpus, hits, x.multi[("float", "edge")], "float", 64))
        assert api.count_terms_supported(x.searcher, T[4], x.mcoll(("float", "edge")), 64) is False   # (the text route's known limit)
    finally:
        if x is not None:
            release(x.leaves)
        c.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def _add_multi(seg, field, kind, n, docs, values):
    d = None if docs is None else np.ascontiguousarray(docs, dtype=np.int32)      # (named: alive until the call returns)
    v = None if values is None else np.ascontiguousarray(values, dtype=np.uint32)
    return _lib.load().nrtgpu_segment_add_doc_values_multi(seg._h, field, kind, n, None if d is None else d.ctypes.data, None if v is None else v.ctypes.data)


def test_refusals_of_the_upload(ctx):
    inv, state = _lib.NRTGPU_ERR_INVALID_ARG, _lib.NRTGPU_ERR_STATE
    seg = fs.make_corpus([100], {ALL: 1.0}, seed=2).segments[0]
    g = api.GpuSegment(ctx, 100, 0)
    try:
        ok_docs, ok_vals = [0, 0, 5, 99], [1, 2, 3, 4]
        for name, args in (("kind -1", (7, -1, 4, ok_docs, ok_vals)), ("kind 2", (7, 2, 4, ok_docs, ok_vals)), ("n_values -1", (7, 0, -1, ok_docs, ok_vals)),
                           ("NULL value_docs", (7, 0, 4, None, ok_vals)), ("NULL values", (7, 0, 4, ok_docs, None)),
                           ("decreasing", (7, 0, 4, [0, 5, 4, 99], ok_vals)), ("a docid at max_doc", (7, 0, 4, [0, 0, 5, 100], ok_vals)),
                           ("a negative docid", (7, 0, 4, [-1, 0, 5, 99], ok_vals))):
            assert _add_multi(g, *args) == inv, name
        assert _add_multi(g, 7, 0, 4, ok_docs, ok_vals) == 0
        assert _add_multi(g, 7, 0, 4, ok_docs, ok_vals) == inv and _add_multi(g, 7, 1, 0, None, None) == inv   # a second column on the field
        with pytest.raises(_lib.NrtGpuError) as e:
            g.add_doc_values(7, "int", np.arange(100, dtype=np.int32))   # ... of the other arity
        assert e.value.code == inv
        g.add_doc_values(8, "int", np.arange(100, dtype=np.int32))
        assert _add_multi(g, 8, 0, 4, ok_docs, ok_vals) == inv and _add_multi(g, 9, 0, 0, None, None) == 0
        g.add_field_norms(0, seg.norms)
        g.add_terms(0, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
        g.seal()
        assert _add_multi(g, 10, 0, 4, ok_docs, ok_vals) == state
    finally:
        g.release()


def test_refusals_of_the_calls(ctx, ix):
    s, inv, uns = ix.searcher, _lib.NRTGPU_ERR_INVALID_ARG, _lib.NRTGPU_ERR_UNSUPPORTED
    top = api.TopScoreDocCollectorManager(10)
    multi_sort = api.SortField(MULTI[("int", "mixed")], "int", False, 0)
    # a sort names ONE value per doc: both sorted entries and their predicates
    with pytest.raises(_lib.NrtGpuError) as e:
        api.search_sorted_batch(s, [T[4]], [top], [multi_sort])
    assert e.value.code == uns and "query 0" in str(e.value) and "selector" in str(e.value)
    with pytest.raises(_lib.NrtGpuError) as e:
        api.search_docset_sorted_batch(s, [api.DocSetQuery()], [top], [multi_sort])
    assert e.value.code == uns and "query 0" in str(e.value) and "selector" in str(e.value)
    assert api.sorted_supported(s, T[4], top, multi_sort) is False and api.docset_sorted_supported(s, api.DocSetQuery(), top, multi_sort) is False
    # an invalid argument in query 1 comes before the unsupported query 0
    with pytest.raises(_lib.NrtGpuError) as e:
        api.search_docset_sorted_batch(s, [api.DocSetQuery(), api.DocSetQuery()], [top, api.TopScoreDocCollectorManager(0)], [multi_sort, ix.sort("int", False, 0)])
    assert e.value.code == inv and "query 1" in str(e.value)
    with pytest.raises(_lib.NrtGpuError) as e:
        api.search_sorted_batch(s, [T[4], T[4]], [top, api.TopScoreDocCollectorManager(0)], [multi_sort, ix.sort("int", False, 0)])
    assert e.value.code == inv and "query 1" in str(e.value)
    # arity differing across the leaves of a call: where "different kinds" is refused
    corpus = fs.make_corpus([100, 100], {ALL: 1.0}, seed=2)
    leaves = []
    try:
        for si, seg in enumerate(corpus.segments):
            g = api.GpuSegment(ctx, seg.max_doc, seg.doc_base)
            leaves.append(g)
            g.add_field_norms(0, seg.norms)
            g.add_terms(0, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
            if si == 0:
                g.add_doc_values(7, "int", np.arange(100, dtype=np.int32))
            else:
                g.add_doc_values_multi(7, "int", np.arange(100, dtype=np.int32), np.arange(100, dtype=np.int32))
            g.add_doc_values(8, "int", np.arange(100, dtype=np.int32))
            g.seal()
        two = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics.from_corpus(corpus))
        coll7, sort8 = api.TermsCollector(7, 10), api.SortField(8, "int", False, 0)
        ranged = api.DocSetQuery((), (), (api.RangeClause(7, "int", 0, 5),))
        for name, call in (("text count", lambda: api.count_terms_batch(two, [T[ALL]], [coll7], 64)),
                           ("docset count", lambda: api.count_docset_terms_batch(two, [api.DocSetQuery()], [coll7], 64)),
                           ("range clause", lambda: api.search_docset_sorted_batch(two, [ranged], [top], [sort8])),
                           ("text sort", lambda: api.search_sorted_batch(two, [T[ALL]], [top], [api.SortField(7, "int", False, 0)])),
                           ("behind an unsupported query 0", lambda: api.count_docset_terms_batch(two, [api.DocSetQuery((api.MaskFilter(77),)), api.DocSetQuery()],
                                                                                                    [api.TermsCollector(8, 10), coll7], 64))):
            with pytest.raises(_lib.NrtGpuError) as e:
                call()
            assert e.value.code == inv and "single-valued and multi-valued" in str(e.value), f"{name}: {e.value}"
        with pytest.raises(_lib.NrtGpuError):
            api.count_terms_supported(two, T[ALL], coll7, 64)
        with pytest.raises(_lib.NrtGpuError):
            api.count_docset_terms_supported(two, ranged, api.TermsCollector(8, 10), 64)
        got = api.count_docset_terms_batch(two, [api.DocSetQuery()], [api.TermsCollector(8, 10)], 128)[0]   # and the route still answers
        assert got.total_hits == 200 and len(got.counts) == 100
    finally:
        release(leaves)
