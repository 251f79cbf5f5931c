"""A text query beside knn clauses (a request's `query` + `knn`) through the C ABI on the device, against tests/_text_knn_ref.py
(the oracle's BM25 arithmetic, exact vector search, collectors and merge around the BooleanQuery's sum).  Bit-exact like every
BM25 test -- docids, ranks, float32 score bits -- plus the exact total_hits and the relation.  Needs a real MI355X."""
import numpy as np
import pytest

from nrtsearch_amd import _lib, api, synth
from oracle import oracle

from tests import _text_knn_ref as ref
from tests.test_final_score_rounds_gpu import corpus_of
from tests.test_parity_gpu import assert_same

pytestmark = pytest.mark.gpu
f32 = np.float32
TERMS = (1, 2)
MASK = 7
VEC_FIELD, DIM = 1, 8


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
    c = api.GpuContext(device_id=0, max_batch=64)
    yield c
    c.close()


class Ix:
    """A corpus on the device: text in field 0, optionally vectors in field 1, mask MASK = a random 60 % of every leaf."""

    def __init__(self, ctx, corpus, vectors=None, mask_density=0.6):
        self.corpus = corpus
        self.leaves = []
        for si, seg in enumerate(corpus.segments):
            g = api.GpuSegment(ctx, seg.max_doc, seg.doc_base)
            g.add_field_norms(0, seg.norms)
            g.add_terms(0, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
            if vectors is not None:
                g.add_vectors(VEC_FIELD, vectors[si])
            g.seal()
            if seg.live_bits is not None:
                g.set_live_docs(seg.live_bits)
            self.leaves.append(g)
        self.mask_words = [synth.random_mask(seg.max_doc, mask_density, 500 + si) for si, seg in enumerate(corpus.segments)]
        for leaf, w in zip(self.leaves, self.mask_words):
            leaf.set_mask(MASK, w)
        self.accept = [synth.accept_words(seg, w) for seg, w in zip(corpus.segments, self.mask_words)]
        self.searcher = api.GpuIndexSearcher(ctx, self.leaves, api.IndexStatistics.from_corpus(corpus))

    def close(self):
        for leaf in self.leaves:
            leaf.release()


def text_query(terms, masked=False):
    cl = tuple(api.TermQuery(0, int(t)) for t in terms)
    if masked:   # FILTER: no pure disjunction, the NESTED form
        return api.BooleanQuery(cl, 1, (api.MaskFilter(MASK),))
    return cl[0] if len(cl) == 1 else api.BooleanQuery(cl)


def clauses(lists):
    return [api.KnnClause(np.asarray(d, np.int32), np.asarray(s, np.float32), float(b)) for d, s, b in lists]


def same(name, got, exp, k, thr=1000):
    assert_same(name, got, exp, k, thr)
    assert got.total_hits == exp[2], f"{name}: total_hits {got.total_hits}, the reference counts {exp[2]}"


def check(x, name, cases):
    """cases: dicts (terms, k, lists, masked, after, thr); one batch; every answer against the reference, bit for bit."""
    qs = [text_query(c["terms"], c.get("masked", False)) for c in cases]
    mgrs = [api.TopScoreDocCollectorManager(c["k"], None if c.get("after") is None else api.ScoreDoc(*c["after"]), c.get("thr", 1000)) for c in cases]
    got = x.searcher.search_text_knn_batch(qs, [clauses(c["lists"]) for c in cases], mgrs)
    infos = []
    for i, (c, td) in enumerate(zip(cases, got)):
        info = {}
        exp = ref.search(oracle, x.corpus, list(c["terms"]), c["k"], c["lists"], nested=c.get("masked", False),
                         accept=x.accept if c.get("masked") else None, after=c.get("after"), total_hits_threshold=c.get("thr", 1000), info=info)
        same(f"{name}_{i}", td, exp, c["k"], c.get("thr", 1000))
        infos.append(info)
        assert x.searcher.text_knn_supported(qs[i], clauses(c["lists"]), mgrs[i])
    return got, infos


def scores_for(docs, seed, lo=0.05, hi=3.0):
    rng = np.random.Generator(np.random.PCG64(seed))
    return (lo + (hi - lo) * rng.random(len(docs))).astype(f32)


def docs_of_every_kind(x, terms, per_kind=3):
    """Global docids of every leaf, up to per_kind each of: matching the text inside the mask, not matching, matching outside the
    mask (live), deleted."""
    out = []
    for si, seg in enumerate(x.corpus.segments):
        matched, _ = ref.text_sums(oracle, x.corpus, terms)[si]
        live = ref._bits(seg.live_bits, seg.max_doc) if seg.live_bits is not None else np.ones(seg.max_doc, dtype=bool)
        inside = ref._bits(x.mask_words[si], seg.max_doc)
        for flags in (matched & live & inside, ~matched & live & inside, matched & live & ~inside, ~matched & live & ~inside, ~live):
            out += (seg.doc_base + np.nonzero(flags)[0][:per_kind]).tolist()
    return np.array(sorted(set(out)), dtype=np.int32)


# ---- 1. mixed leaves ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed(ctx):
    corpus = ref.make_corpus([3000, 1500, 40], [1, 2, 30], delete_fraction=0.01)
    x = Ix(ctx, corpus, ref.leaf_vectors(corpus, DIM))
    yield x
    x.close()


def test_mixed_leaves_flat_and_nested(mixed):
    """Three leaves (3000 / 1500 / 40 docs), 1 % deletes, two-term queries, both forms.  Every case lists docs that match the text,
    docs that do not, and deleted docs; the NESTED cases (one FILTER mask) also live docs outside the mask.  (Without a mask the
    accept set IS liveDocs: that fourth kind cannot exist in a FLAT case.)"""
    x = mixed
    vectors = ref.leaf_vectors(x.corpus, DIM)
    kd = docs_of_every_kind(x, TERMS)
    l0 = (kd, scores_for(kd, 1), 1.0)
    l1 = (kd[::2], scores_for(kd[::2], 2, 0.5, 1.0), 50.0)
    kl = ref.knn_list(oracle, x.corpus, vectors, 0, np.linspace(-1, 1, DIM).astype(f32), 15)
    l2 = (kl[0], kl[1], 7.5)
    kd30 = docs_of_every_kind(x, (30,))
    l30 = (kd30, scores_for(kd30, 13, 0.5, 1.0), 50.0)
    cases = []
    for masked in (False, True):
        for k in (10, 1024):
            cases.append(dict(terms=TERMS, k=k, lists=[l0], masked=masked))
            cases.append(dict(terms=TERMS, k=k, lists=[l2, l0, l1], masked=masked, thr=api.INT_MAX))
        cases.append(dict(terms=(30,), k=50, lists=[l30, l2], masked=masked))
    _, infos = check(x, "mixed", cases)
    for c, info in zip(cases, infos):
        kinds = info["kinds"]
        assert kinds["text"] > 0 and kinds["no_text"] > 0 and kinds["deleted"] > 0, kinds
        assert (kinds["outside"] > 0) == bool(c["masked"]), kinds


# ---- 2. sub-tile edges ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_doc", [1, 1023, 1024, 1025, 12 * 1024 + 1])
def test_sub_tile_edges(ctx, max_doc):
    corpus = ref.make_corpus([max_doc], [1, 2], delete_fraction=0.01 if max_doc > 64 else 0.0, seed=77)
    x = Ix(ctx, corpus)
    try:
        edge = np.array(sorted({d for d in (0, 63, 64, 1023, 1024, max_doc - 1) if d < max_doc}), dtype=np.int32)
        lists = [(edge, scores_for(edge, 3), 1.0), (edge[::-1].copy(), scores_for(edge, 4), 2.0)]
        cases = [dict(terms=TERMS, k=k, lists=lists, masked=m) for k in (3, 1024) for m in (False, True)]
        check(x, f"edges_{max_doc}", cases)
    finally:
        x.close()


def _is_live(corpus, doc):
    for seg in corpus.segments:
        if seg.doc_base <= doc < seg.doc_base + seg.max_doc:
            return seg.live_bits is None or bool(ref._bits(seg.live_bits, seg.max_doc)[doc - seg.doc_base])
    return False


# ---- 3. leaves without text -----------------------------------------------------------------------------------------
def test_leaves_and_queries_without_text(ctx):
    """A leaf that holds none of the query's terms but has listed docs (its second half only: the kept part is narrowed), and a
    query whose terms no leaf holds but that has lists: the listed docs are hits all the same."""
    corpus = ref.make_corpus([2000, 5000, 300], [1, 2], delete_fraction=0.01, without=[(1, 1), (1, 2)])
    x = Ix(ctx, corpus)
    try:
        assert all(len(corpus.segments[1].postings(t)[0]) == 0 for t in TERMS)
        d1 = np.array([2000 + 2500, 2000 + 2600, 2000 + 4999, 10, 7100], dtype=np.int32)
        lists = [(d1, scores_for(d1, 5), 1.0)]
        got, _ = check(x, "no_text_leaf", [dict(terms=TERMS, k=1024, lists=lists)])
        assert api.GpuContext.last_diagnostics()["items_scan"] >= 1
        live = [d for d in d1.tolist() if _is_live(corpus, d)]
        got, _ = check(x, "no_text_query", [dict(terms=(99,), k=10, lists=lists), dict(terms=(98, 99), k=10, lists=lists, masked=True)])
        assert api.GpuContext.last_diagnostics()["items_scan"] >= 1
        assert sorted(got[0].docs.tolist()) == sorted(live) and got[0].total_hits == len(live)
        got, _ = check(x, "nothing", [dict(terms=(99,), k=10, lists=[])])
        assert got[0].total_hits == 0 and api.GpuContext.last_diagnostics()["items_scan"] == 0
    finally:
        x.close()


# ---- 4. dense lists -------------------------------------------------------------------------------------------------
def test_dense_lists_and_the_overflow_path(ctx):
    """1024 listed docs in one 1024-doc sub-tile (more than 64 entries per step, and waves whose 64 entries all lie below their
    sub-tile); the same doc in all 8 lists; k = 1024 with every doc a hit: the round's candidates overflow the buffer."""
    corpus = corpus_of(12 * 1024 + 1)
    x = Ix(ctx, corpus)
    try:
        tile = np.arange(1024, 2048, dtype=np.int32)
        lists = [(tile, scores_for(tile, 6), 1.0)]
        for li in range(1, 8):
            d = np.array([1500, 100 * li, 12 * 1024], dtype=np.int32)
            lists.append((d, scores_for(d, 10 + li), float(li)))
        cases = [dict(terms=(1,), k=1024, lists=lists, masked=m) for m in (False, True)] + [dict(terms=(1,), k=5, lists=lists)]
        got, _ = check(x, "dense", cases)
        assert got[0].total_hits == 12 * 1024 + 1
    finally:
        x.close()


# ---- 5. several items -----------------------------------------------------------------------------------------------
def test_a_query_cut_into_several_items(ctx):
    corpus = corpus_of(300_000)
    x = Ix(ctx, corpus)
    try:
        d = np.array([5, 1023, 1024, 70_000, 149_999, 150_000, 150_001, 220_000, 299_999], dtype=np.int32)
        lists = [(d, scores_for(d, 8, 1.0, 9.0), 1.0), (d[::3].copy(), scores_for(d[::3], 9), 3.0)]
        check(x, "items", [dict(terms=(1,), k=100, lists=lists)])
        assert api.GpuContext.last_diagnostics()["items_scan"] >= 2
    finally:
        x.close()


# ---- 6. paging and threshold ----------------------------------------------------------------------------------------
def test_paging_and_thresholds(mixed):
    x = mixed
    kd = docs_of_every_kind(x, (30,), per_kind=4)
    lists = [(kd, scores_for(kd, 12), 1.0)]
    whole = ref.search(oracle, x.corpus, [30], 1024, lists)
    n = whole[2]
    assert 50 < n < 1024 and len(whole[0]) == n
    after, seen = None, []
    for page in range(n // 25 + 2):
        got, _ = check(x, f"page_{page}", [dict(terms=(30,), k=25, lists=lists, after=after)])
        if len(got[0].docs) == 0:
            break
        seen += got[0].docs.tolist()
        after = (int(got[0].docs[-1]), float(got[0].scores[-1]))
    assert seen == whole[0].tolist()   # no duplicate, no gap
    check(x, "thresholds", [dict(terms=(30,), k=5, lists=lists, thr=thr, masked=m) for thr in (10, n - 1, n, 100_000) for m in (False, True)])


# ---- 7. empty lists -------------------------------------------------------------------------------------------------
def test_no_lists_is_the_function_score_entry_without_functions(mixed):
    x = mixed
    for masked in (False, True):
        qs = [text_query(TERMS, masked), text_query((30,), masked)]
        mgrs = [api.TopScoreDocCollectorManager(100), api.TopScoreDocCollectorManager(1024, None, api.INT_MAX)]
        a = x.searcher.search_text_knn_batch(qs, [[], []], mgrs)
        b = x.searcher.search_function_score_batch([api.FunctionScoreQuery(q) for q in qs], mgrs)
        for ta, tb in zip(a, b):
            assert ta.docs.tolist() == tb.docs.tolist() and ta.scores.view(np.uint32).tolist() == tb.scores.view(np.uint32).tolist()
            assert ta.total_hits == tb.total_hits and ta.relation_gte == tb.relation_gte
    check(x, "no_lists", [dict(terms=TERMS, k=100, lists=[], masked=m) for m in (False, True)])


# ---- 8. the whole request -------------------------------------------------------------------------------------------
def test_search_with_knn_end_to_end(mixed):
    """`query` + two `knn` clauses as a caller writes them: the knn pass on the device (knn_search_requests), its lists beside the
    text query.  The reference: oracle.knn_exact per clause, then the BooleanQuery's sum."""
    x = mixed
    vectors = ref.leaf_vectors(x.corpus, DIM)
    q0, q1 = np.linspace(-1, 1, DIM).astype(f32), np.cos(np.arange(DIM)).astype(f32)
    for masked in (False, True):
        got = x.searcher.search_with_knn(text_query((2,), masked), api.TopScoreDocCollectorManager(30),
                                         knn=[(VEC_FIELD, "cosine", q0, 15, 50.0, None), (VEC_FIELD, "l2_norm", q1, 10, 2.0, api.MaskFilter(MASK))])
        lists = [ref.knn_list(oracle, x.corpus, vectors, 0, q0, 15, boost=50.0) + (1.0,),
                 ref.knn_list(oracle, x.corpus, vectors, 2, q1, 10, boost=2.0, accept=x.accept) + (1.0,)]
        exp = ref.search(oracle, x.corpus, [2], 30, lists, nested=masked, accept=x.accept if masked else None)
        same(f"with_knn_{masked}", got, exp, 30)
        assert sorted(got.docs[:15].tolist()) == sorted(lists[0][0].tolist())   # boost 50 puts the first clause's docs on top


# ---- 9. refusals ----------------------------------------------------------------------------------------------------
def _refused(x, q, kcl, mgr, code, supported_agrees=True):
    with pytest.raises(_lib.NrtGpuError) as e:
        x.searcher.search_text_knn_batch([q], [kcl], [mgr])
    assert e.value.code == code, str(e.value)
    assert len(str(e.value)) > 20
    if supported_agrees:
        if code == _lib.NRTGPU_ERR_UNSUPPORTED:
            assert x.searcher.text_knn_supported(q, kcl, mgr) is False
        else:
            with pytest.raises(_lib.NrtGpuError) as e2:
                x.searcher.text_knn_supported(q, kcl, mgr)
            assert e2.value.code == code


def test_refusals(mixed):
    x = mixed
    mgr = api.TopScoreDocCollectorManager(10)
    ok = clauses([([5, 3100, 4510], [1.0, 2.0, 0.5], 1.0)])
    q = text_query(TERMS)
    UNS, INV = _lib.NRTGPU_ERR_UNSUPPORTED, _lib.NRTGPU_ERR_INVALID_ARG
    should = tuple(api.TermQuery(0, t) for t in TERMS)
    for bad_q in (api.DisjunctionMaxQuery(should), api.BooleanQuery(should[1:], 0, (), (), should[:1]), api.BooleanQuery(should, 2),
                  api.BooleanQuery((api.BoostQuery(should[0], 1.0), api.BoostQuery(should[1], 1e9)))):   # the last: no common fixed-point scale
        _refused(x, bad_q, ok, mgr, UNS)
    _refused(x, q, ok, api.TopScoreDocCollectorManager(10, None, 1000, 0.5), UNS)   # min_competitive_score
    _refused(x, q, clauses([([5], [0.0], 1.0)]), mgr, UNS)          # a clause value <= 0
    _refused(x, q, clauses([([5], [-1.0], 2.0)]), mgr, UNS)
    _refused(x, q, clauses([([5], [1e-20], 1.0)]), mgr, UNS)        # the exactness test
    assert "53" in _lib.load().nrtgpu_last_error().decode()
    _refused(x, q, clauses([([5], [1.0], 1.0)] * 9), mgr, INV)      # n_lists
    _refused(x, q, clauses([(np.arange(1025), np.ones(1025), 1.0)]), mgr, INV)   # n
    _refused(x, q, clauses([([5], [1.0], 0.0)]), mgr, INV)
    _refused(x, q, clauses([([5], [1.0], float("inf"))]), mgr, INV)
    _refused(x, q, clauses([([5], [float("nan")], 1.0)]), mgr, INV)
    _refused(x, q, clauses([([5, 6, 5], [1.0, 1.0, 1.0], 1.0)]), mgr, INV)       # a doc twice in one list
    _refused(x, q, clauses([([5, 4540], [1.0, 1.0], 1.0)]), mgr, INV, supported_agrees=False)   # past the last leaf (the predicate has no doc_bases)
    _refused(x, q, clauses([([-1], [1.0], 1.0)]), mgr, INV, supported_agrees=False)
    _refused(x, q, ok, api.TopScoreDocCollectorManager(0), INV)     # validate_query's
    # text_nested == 0 with a mask, and NULL arrays: only a caller of the C ABI can say that
    s = x.searcher
    m = s._marshal([text_query(TERMS, True)], [mgr])
    kc = s._marshal_knn_clauses([ok], m)
    outs, _, _ = api._topdocs_outputs(1, 10)
    lib = _lib.load()
    assert kc[0].text_nested == 1
    kc[0].text_nested = 0
    assert lib.nrtgpu_search_text_knn_batch(s.ctx._h, s._segs, s._bases, len(s.leaves), m.queries, kc, 1, outs) == INV
    assert "text_nested" in lib.nrtgpu_last_error().decode()
    assert lib.nrtgpu_text_knn_supported(s.ctx._h, s._segs, len(s.leaves), m.queries, kc) == INV
    kc[0].text_nested = 1
    kc[0].lists[0].docs = None
    assert lib.nrtgpu_search_text_knn_batch(s.ctx._h, s._segs, s._bases, len(s.leaves), m.queries, kc, 1, outs) == INV
    kc[0].lists = None
    assert lib.nrtgpu_search_text_knn_batch(s.ctx._h, s._segs, s._bases, len(s.leaves), m.queries, kc, 1, outs) == INV
    # and the route still runs
    check(x, "after_refusals", [dict(terms=TERMS, k=10, lists=[([5, 3100, 4510], [1.0, 2.0, 0.5], 1.0)])])


@pytest.mark.parametrize("flag", [_lib.NRTGPU_FLAG_PACKED_POSTINGS, _lib.NRTGPU_FLAG_NO_FIXED_POINT])
def test_contexts_the_route_refuses(flag):
    corpus = ref.make_corpus([500], [1, 2])
    c = api.GpuContext(device_id=0, max_batch=16, flags=flag)
    x = None
    try:
        x = Ix(c, corpus)
        _refused(x, text_query(TERMS), clauses([([5], [1.0], 1.0)]), api.TopScoreDocCollectorManager(10), _lib.NRTGPU_ERR_UNSUPPORTED)
        got = x.searcher.search_batch([text_query(TERMS)], [api.TopScoreDocCollectorManager(10)])[0]
        assert_same("plain_after_refusal", got, oracle.search_bm25(corpus, list(TERMS), 10), 10, 1000)
    finally:
        if x is not None:
            x.close()
        c.close()
