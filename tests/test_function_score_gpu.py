"""Function-score queries (MultiFunctionScoreQuery with weight functions over a BM25 disjunction) through the C ABI on the
device, against tests/_function_score_ref.py (the oracle's BM25 arithmetic, collectors and merge around the reference's
function-score rules).  Bit-exact like every BM25 test -- docids, ranks, float32 score bits -- plus the exact total_hits: the
count is never a lower bound on this route.  Needs a real MI355X."""
import numpy as np
import pytest

from nrtsearch_amd import _lib, api, synth
from oracle import oracle

from tests import _function_score_ref as ref
from tests.test_parity_gpu import Index, assert_same

pytestmark = pytest.mark.gpu
f32 = np.float32
INT_MAX = 2**31 - 1
RANKS = [1, 2, 4, 9, 30, 120, 700, 4000]
TERM_SETS = ((1, 2, 30), (2, 30, 700))
FUNCTIONS = ((7, 2.5), (0, 1.25), (9, 0.5), (11, 3.0))
MODE_PAIRS = [(s, b) for s in ("multiply", "sum") for b in ("multiply", "sum", "replace")]


def fsq(terms, functions=(), score_mode="multiply", boost_mode="multiply", min_score=0.0, min_excluded=False, inner=None):
    if inner is None:
        cl = tuple(api.TermQuery(0, int(t)) for t in terms)
        inner = cl[0] if len(cl) == 1 else api.BooleanQuery(cl)
    return api.FunctionScoreQuery(inner, tuple(api.WeightFunction(float(w), int(m)) for m, w in functions), score_mode, boost_mode,
                                  float(min_score), bool(min_excluded))


def same(name, got, exp, k, thr):
    assert_same(name, got, exp, k, thr)
    assert got.total_hits == exp[2], f"{name}: total_hits {got.total_hits}, the reference counts {exp[2]}"


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


def make_masks(corpus):
    masks = {}
    for si, seg in enumerate(corpus.segments):
        masks[(si, 7)] = synth.random_mask(seg.max_doc, 0.30, 100 + si)
        masks[(si, 9)] = synth.random_mask(seg.max_doc, 0.05, 200 + si)
        masks[(si, 11)] = synth.random_mask(seg.max_doc, 0.0005, 300 + si)
    return masks


def set_masks(leaves, masks):
    for (si, mid), bits in masks.items():
        leaves[si].set_mask(mid, bits)


@pytest.fixture(scope="module")
def corpus():
    c = synth.build_corpus(60_000, RANKS, n_segments=3, delete_fraction=0.02)
    # a posting with freq > 12 among term 1's: the kernel's escape decode runs
    assert sum(int((seg.postings(1)[1] > 12).sum()) for seg in c.segments) >= 1
    return c


@pytest.fixture(scope="module")
def masks(corpus):
    return make_masks(corpus)


@pytest.fixture(scope="module")
def ix(ctx, corpus, masks):
    x = Index(ctx, corpus)
    set_masks(x.leaves, masks)
    yield x
    x.close()


# ---- 1. the reference's own constants through the device ---------------------------------------------
def test_reference_constants_through_the_device(ctx):
    g = ref.golden()
    corpus = ref.golden_corpus(g)
    x = Index(ctx, corpus)
    try:
        queries, exps = [], []
        for ci, case in enumerate(g["cases"]):
            funcs = ref.golden_functions(g, case)
            fl = []
            for i, (docs, w) in enumerate(funcs):
                mask_id = 100 + 10 * ci + i   # (a mask of its own per case and function: all cases run in one batch)
                if docs is not None:
                    x.leaves[0].set_mask(mask_id, ref.doc_set_words(docs, 4))
                fl.append((0 if docs is None else mask_id, w))
            term = int(g["corpus"]["term_ids"][case["inner"]])
            queries.append(fsq([term], fl, case["score_mode"], case["boost_mode"], case["min_score"], case["min_excluded"]))
            exps.append(sorted(((f32(s), int(d)) for d, s in case["expected"].items()), key=lambda e: (-e[0], e[1])))
        got = x.searcher.search_function_score_batch(queries, [api.TopScoreDocCollectorManager(10)] * len(queries))
        for case, td, exp in zip(g["cases"], got, exps):
            assert td.docs.tolist() == [d for _, d in exp], case["name"]
            assert td.scores.view(np.uint32).tolist() == [int(s.view(np.uint32)) for s, _ in exp], case["name"]
            assert td.total_hits == len(exp) and not td.relation_gte, case["name"]
        for q in queries:
            assert x.searcher.function_score_supported(q, api.TopScoreDocCollectorManager(10))
    finally:
        x.close()


# ---- 3. every mode pair ----------------------------------------------------------------------------------
@pytest.mark.parametrize("score_mode,boost_mode", MODE_PAIRS)
def test_modes(ix, corpus, masks, score_mode, boost_mode):
    cases = [(terms, k, thr) for terms in TERM_SETS for k in (1, 100, 1024) for thr in (1000, INT_MAX)]
    qs = [fsq(t, FUNCTIONS, score_mode, boost_mode) for t, _, _ in cases]
    got = ix.searcher.search_function_score_batch(qs, [api.TopScoreDocCollectorManager(k, None, thr) for _, k, thr in cases])
    d = api.GpuContext.last_diagnostics()
    assert d["items_maxscore"] == 0 and d["items_scan"] >= len(cases)
    for (terms, k, thr), td in zip(cases, got):
        exp = ref.search(oracle, corpus, terms, k, FUNCTIONS, score_mode, boost_mode, masks=masks, total_hits_threshold=thr)
        same(f"fs_{score_mode}_{boost_mode}_{terms}_{k}_{thr}", td, exp, k, thr)


def test_eight_functions(ix, corpus, masks):
    funcs = ((7, 2.5), (0, 1.25), (9, 0.5), (11, 3.0), (7, 0.75), (9, 7.0), (0, 0.3), (11, 1.5))
    for sm, bm in (("multiply", "multiply"), ("sum", "sum")):
        got = ix.searcher.search_function_score_batch([fsq(TERM_SETS[0], funcs, sm, bm)], [api.TopScoreDocCollectorManager(100)])[0]
        exp = ref.search(oracle, corpus, TERM_SETS[0], 100, funcs, sm, bm, masks=masks)
        same(f"fs_eight_{sm}", got, exp, 100, 1000)


# ---- 4. REPLACE: keys that differ only in the docid --------------------------------------------------------
def test_replace_selects_among_equal_scores(ix, corpus, masks):
    exp = ref.search(oracle, corpus, TERM_SETS[0], 100, FUNCTIONS, "multiply", "replace", masks=masks, total_hits_threshold=INT_MAX)
    assert int((np.diff(exp[1]) == 0).sum()) >= 90
    got = ix.searcher.search_function_score_batch([fsq(TERM_SETS[0], FUNCTIONS, "multiply", "replace")],
                                                  [api.TopScoreDocCollectorManager(100, None, INT_MAX)])[0]
    same("fs_replace_ties", got, exp, 100, INT_MAX)


# ---- 5. more candidates than the buffer holds before the first compaction --------------------------------------
def test_compaction_at_k_1024(ix, corpus, masks):
    # weights that grow the score with the docid's mask membership do not matter here: theta starts at 0, so every one of the
    # first hits is a candidate and the buffer (a few thousand keys) overflows long before the >= 20 000 hits are through
    for terms in TERM_SETS:
        exp = ref.search(oracle, corpus, terms, 1024, FUNCTIONS, "sum", "multiply", masks=masks, total_hits_threshold=INT_MAX)
        assert exp[2] >= 20_000
        got = ix.searcher.search_function_score_batch([fsq(terms, FUNCTIONS, "sum", "multiply")],
                                                      [api.TopScoreDocCollectorManager(1024, None, INT_MAX)])[0]
        same(f"fs_compaction_{terms}", got, exp, 1024, INT_MAX)


# ---- 6. a query cut into several items, several searcher slices ------------------------------------------------
def test_split_items_and_slices(corpus, masks):
    c = api.GpuContext(device_id=0, max_batch=64, target_items=4096)
    x = None
    try:
        c.set_slicing(20_000, 5)
        slicing = (20_000, 5)
        assert len(oracle.corpus_slices(corpus, slicing)) >= 2
        x = Index(c, corpus)
        set_masks(x.leaves, masks)
        # the planner cuts by cost (postings; an item is never cheaper than 2^17): duplicate clauses make one query three items' worth
        terms = [1] * 8 + [2] * 8 + [30] * 2
        info = {}
        ref.search(oracle, corpus, terms, 100, FUNCTIONS, "multiply", "sum", masks=masks, total_hits_threshold=INT_MAX, slicing=slicing,
                   info=info)
        per_slice = info["slice_hits"]
        assert len(per_slice) >= 2 and min(per_slice) > 100
        # total_hits exceeds this threshold, no slice does: EQUAL_TO by the per-slice rule
        thr_equal = max(per_slice)
        for k, thr in ((100, 1000), (100, thr_equal), (1024, INT_MAX), (1, 0)):
            exp = ref.search(oracle, corpus, terms, k, FUNCTIONS, "multiply", "sum", masks=masks, total_hits_threshold=thr, slicing=slicing)
            got = x.searcher.search_function_score_batch([fsq(terms, FUNCTIONS, "multiply", "sum")],
                                                          [api.TopScoreDocCollectorManager(k, None, thr)])[0]
            assert api.GpuContext.last_diagnostics()["items_scan"] >= 3
            same(f"fs_split_{k}_{thr}", got, exp, k, thr)
            if thr == thr_equal:
                assert got.total_hits > thr and not got.relation_gte
            if thr == 1000:
                assert got.relation_gte
    finally:
        if x is not None:
            x.close()
        c.close()


# ---- 7. what the inner query keeps ----------------------------------------------------------------------------
def test_inner_filter_and_must_not_next_to_function_masks(ix, corpus, masks):
    terms = TERM_SETS[1]
    should = tuple(api.TermQuery(0, t) for t in terms)
    # FILTER mask 7 is also the first function's mask; MUST_NOT mask 9 is also the third's (never matches a hit then)
    inner = api.BooleanQuery(should, 1, (api.MaskFilter(7),), (api.MaskFilter(9),))
    acc = [synth.accept_words(seg, masks[(si, 7)], masks[(si, 9)]) for si, seg in enumerate(corpus.segments)]
    for sm, bm in (("multiply", "multiply"), ("sum", "replace")):
        got = ix.searcher.search_function_score_batch([fsq(terms, FUNCTIONS, sm, bm, inner=inner)], [api.TopScoreDocCollectorManager(200)])[0]
        exp = ref.search(oracle, corpus, terms, 200, FUNCTIONS, sm, bm, masks=masks, accept=acc)
        same(f"fs_inner_masks_{sm}", got, exp, 200, 1000)


@pytest.mark.parametrize("boost_mode", ["multiply", "replace"])
def test_search_after_pages(ix, corpus, masks, boost_mode):
    terms = TERM_SETS[0]
    full = ref.search(oracle, corpus, terms, 150, FUNCTIONS, "multiply", boost_mode, masks=masks, total_hits_threshold=INT_MAX)
    after, docs, scores = None, [], []
    for page in range(3):
        got = ix.searcher.search_function_score_batch([fsq(terms, FUNCTIONS, "multiply", boost_mode)],
                                                      [api.TopScoreDocCollectorManager(50, after, INT_MAX)])[0]
        exp = ref.search(oracle, corpus, terms, 50, FUNCTIONS, "multiply", boost_mode, masks=masks, total_hits_threshold=INT_MAX,
                         after=(after.doc, after.score) if after else None)
        same(f"fs_after_{boost_mode}_{page}", got, exp, 50, INT_MAX)
        docs += got.docs.tolist()
        scores += got.scores.view(np.uint32).tolist()
        after = api.ScoreDoc(int(got.docs[-1]), float(got.scores[-1]))
    assert docs == full[0].tolist() and scores == full[1].view(np.uint32).tolist()


@pytest.mark.parametrize("min_excluded", [False, True])
def test_min_score_at_the_500th_final_score(ix, corpus, masks, min_excluded):
    terms = TERM_SETS[0]
    top = ref.search(oracle, corpus, terms, 1024, FUNCTIONS, "multiply", "multiply", masks=masks, total_hits_threshold=INT_MAX)
    ms = float(top[1][499])
    exp = ref.search(oracle, corpus, terms, 1024, FUNCTIONS, "multiply", "multiply", ms, min_excluded, masks=masks, total_hits_threshold=INT_MAX)
    assert 0 < exp[2] < top[2]
    got = ix.searcher.search_function_score_batch([fsq(terms, FUNCTIONS, "multiply", "multiply", ms, min_excluded)],
                                                  [api.TopScoreDocCollectorManager(1024, None, INT_MAX)])[0]
    same(f"fs_min_score_{min_excluded}", got, exp, 1024, INT_MAX)
    assert (f32(ms) in got.scores) == (not min_excluded)


def test_fork_with_other_live_docs(ctx, ix, corpus, masks):
    """A second reader version: its deletes are tested as a mask instead of folded into the postings."""
    lives, forks = [], []
    try:
        for si, (seg, leaf) in enumerate(zip(corpus.segments, ix.leaves)):
            n = (seg.max_doc + 63) // 64
            base = seg.live_bits[:n].copy() if seg.live_bits is not None else np.full(n, ~np.uint64(0), dtype=np.uint64)
            live = base & ~synth.random_mask(seg.max_doc, 0.05, 900 + si)[:n]
            lives.append(live)
            forks.append(leaf.fork(live))
        set_masks(forks, masks)
        searcher = api.GpuIndexSearcher(ctx, forks, api.IndexStatistics.from_corpus(corpus))
        for terms in TERM_SETS:
            got = searcher.search_function_score_batch([fsq(terms, FUNCTIONS, "sum", "sum")], [api.TopScoreDocCollectorManager(100, None, INT_MAX)])[0]
            exp = ref.search(oracle, corpus, terms, 100, FUNCTIONS, "sum", "sum", masks=masks, total_hits_threshold=INT_MAX, live=lives)
            same(f"fs_fork_{terms}", got, exp, 100, INT_MAX)
        # the first version still sees its own liveDocs
        got = ix.searcher.search_function_score_batch([fsq(TERM_SETS[1], FUNCTIONS, "sum", "sum")], [api.TopScoreDocCollectorManager(100, None, INT_MAX)])[0]
        same("fs_fork_parent", got, ref.search(oracle, corpus, TERM_SETS[1], 100, FUNCTIONS, "sum", "sum", masks=masks, total_hits_threshold=INT_MAX),
             100, INT_MAX)
    finally:
        for f in forks:
            f.release()


def test_mixed_batch_of_64(ix, corpus, masks):
    rng = np.random.default_rng(64)
    qs, mgrs, specs = [], [], []
    for i in range(64):
        n = int(rng.integers(0, 9))
        funcs = tuple((int(rng.choice([0, 7, 9, 11])), float(f32(rng.choice([0.25, 0.5, 1.25, 2.5, 3.0, 11.0])))) for _ in range(n))
        sm, bm = MODE_PAIRS[int(rng.integers(0, 6))]
        k = int(rng.choice([1, 10, 100, 300]))
        thr = int(rng.choice([0, 1000, INT_MAX]))
        terms = TERM_SETS[i % 2]
        ms = float(rng.choice([0.0, 0.0, 1.0]))
        qs.append(fsq(terms, funcs, sm, bm, ms, bool(i % 3 == 0)))
        mgrs.append(api.TopScoreDocCollectorManager(k, None, thr))
        specs.append((terms, k, funcs, sm, bm, ms, bool(i % 3 == 0), thr))
    got = ix.searcher.search_function_score_batch(qs, mgrs)
    for i, (terms, k, funcs, sm, bm, ms, mex, thr) in enumerate(specs):
        exp = ref.search(oracle, corpus, terms, k, funcs, sm, bm, ms, mex, masks=masks, total_hits_threshold=thr)
        same(f"fs_mixed_{i}", got[i], exp, k, thr)


# ---- 8. refusals ------------------------------------------------------------------------------------------------
def _refused(searcher, q, mgr, code=_lib.NRTGPU_ERR_UNSUPPORTED):
    with pytest.raises(_lib.NrtGpuError) as e:
        searcher.search_function_score_batch([q], [mgr])
    assert e.value.code == code, str(e.value)
    assert len(str(e.value)) > 20


def _plain_search_works(searcher, corpus, terms):
    cl = tuple(api.TermQuery(0, int(t)) for t in terms)
    got = searcher.search_batch([cl[0] if len(cl) == 1 else api.BooleanQuery(cl)], [api.TopScoreDocCollectorManager(10)])[0]
    assert_same("fs_plain_after_refusal", got, oracle.search_bm25(corpus, list(terms), 10), 10, 1000)


def test_refusals(ix, corpus, masks):
    mgr = api.TopScoreDocCollectorManager(10)
    ix.leaves[0].set_mask(13, masks[(0, 7)])   # resident on ONE leaf of the call only
    try:
        q = fsq(TERM_SETS[0], ((13, 2.0),))
        _refused(ix.searcher, q, mgr)
        assert ix.searcher.function_score_supported(q, mgr) is False
        assert "13" in _lib.load().nrtgpu_last_error().decode()
        _plain_search_works(ix.searcher, corpus, TERM_SETS[0])
    finally:
        ix.leaves[0].set_mask(13, None)
    should = tuple(api.TermQuery(0, t) for t in TERM_SETS[0])
    for inner in (api.DisjunctionMaxQuery(should), api.BooleanQuery(should[1:], 0, (), (), should[:1]), api.BooleanQuery(should, 2)):
        q = fsq(None, FUNCTIONS, inner=inner)
        _refused(ix.searcher, q, mgr)
        assert ix.searcher.function_score_supported(q, mgr) is False
    _refused(ix.searcher, fsq(TERM_SETS[0], FUNCTIONS), api.TopScoreDocCollectorManager(10, None, 1000, 0.5))   # min_competitive_score
    _refused(ix.searcher, fsq(TERM_SETS[0], ((0, -2.0),)), mgr)
    _refused(ix.searcher, fsq(TERM_SETS[0], ((0, 0.0),)), mgr, _lib.NRTGPU_ERR_INVALID_ARG)
    _refused(ix.searcher, fsq(TERM_SETS[0], FUNCTIONS), api.TopScoreDocCollectorManager(0), _lib.NRTGPU_ERR_INVALID_ARG)   # validate_query's
    _plain_search_works(ix.searcher, corpus, TERM_SETS[1])
    assert ix.searcher.function_score_supported(fsq(TERM_SETS[0], FUNCTIONS), mgr) is True


@pytest.mark.parametrize("flag", [_lib.NRTGPU_FLAG_PACKED_POSTINGS, _lib.NRTGPU_FLAG_NO_FIXED_POINT])
def test_contexts_the_route_refuses(flag):
    g = ref.golden()
    small = ref.golden_corpus(g)
    c = api.GpuContext(device_id=0, max_batch=16, flags=flag)
    x = None
    try:
        x = Index(c, small)
        q = fsq([104], ((0, 1.5),))
        mgr = api.TopScoreDocCollectorManager(10)
        _refused(x.searcher, q, mgr)
        assert x.searcher.function_score_supported(q, mgr) is False
        _plain_search_works(x.searcher, small, [104])
    finally:
        if x is not None:
            x.close()
        c.close()
