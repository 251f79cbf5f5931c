"""A function score over multi-match queries (MultiFunctionScoreQuery with weight functions around the cross_fields / best_fields
shapes) through the C ABI on the device, against tests/_function_score_multi_match_ref.py (the two existing NumPy references
composed) and, where the query degenerates to one of the two existing routes, against those routes on the device.  Bit-exact:
docids, ranks, float32 score bits, the exact total_hits and the relation.  Needs a real MI355X."""
import numpy as np
import pytest

from nrtsearch_amd import _lib, api, synth
from oracle import oracle

from tests import _function_score_multi_match_ref as ref
from tests import _multi_match_ref as mm_ref
from tests.test_parity_gpu import assert_same

pytestmark = pytest.mark.gpu
f32 = np.float32
INT_MAX = 2**31 - 1
TIES = (0.0, 1.0, 0.3, float(np.nextafter(f32(1), f32(0))))
TOKENS = (2, 4, 7)
FUNCTIONS = ((7, 1.5), (9, 3.0), (0, 0.5))
EIGHT = ((7, 2.5), (0, 1.25), (9, 0.5), (7, 3.0), (9, 0.75), (0, 7.0), (7, 0.3), (9, 1.5))
MODE_PAIRS = [(s, b) for s in ("multiply", "sum") for b in ("multiply", "sum", "replace")]
MM_KEYS = ("operator", "msm", "tie_breaker")
FS_KEYS = ("functions", "score_mode", "boost_mode", "min_score", "min_excluded")


def same(name, got, exp, k, thr):
    assert_same(name, got, exp, k, thr)
    assert got.total_hits == exp[2], f"{name}: total_hits {got.total_hits}, the reference counts {exp[2]}"


def device_equal(name, got, other):
    assert got.docs.tolist() == other.docs.tolist(), f"{name}: docids"
    assert got.scores.view(np.uint32).tolist() == other.scores.view(np.uint32).tolist(), f"{name}: score bits"
    assert (got.total_hits, got.relation_gte) == (other.total_hits, other.relation_gte), f"{name}: {got.total_hits} vs {other.total_hits}"


@pytest.fixture(scope="module", autouse=True)
def two_column_postings():
    """The route refuses packed postings (tested below): these contexts keep the two-column layout also where the whole suite
    runs with NRTGPU_PACKED_POSTINGS=1, which packs every api.GpuContext."""
    mp = pytest.MonkeyPatch()
    mp.delenv("NRTGPU_PACKED_POSTINGS", raising=False)
    yield
    mp.undo()


def query_of(s):
    return ref.to_query(api, s["groups"], s["shape"], s.get("operator", "should"), s.get("msm", 0), s.get("tie_breaker", 0.0), s.get("functions", ()),
                        s.get("score_mode", "multiply"), s.get("boost_mode", "multiply"), s.get("min_score", 0.0), s.get("min_excluded", False),
                        s.get("filter", ()), s.get("must_not", ()))


def manager_of(s):
    return api.TopScoreDocCollectorManager(s["k"], api.ScoreDoc(*s["after"]) if s.get("after") else None, s.get("total_hits_threshold", 1000))


class Ix:
    def __init__(self, ctx, fields, masks):
        self.ctx = ctx
        self.leaves, self.stats = mm_ref.upload(api, ctx, fields)
        for (si, mid), bits in masks.items():
            self.leaves[si].set_mask(mid, bits)
        self.searcher = api.GpuIndexSearcher(ctx, self.leaves, self.stats)

    def run(self, specs):
        """specs: dicts of ref.search's arguments -> TopDocs."""
        return self.searcher.search_function_score_multi_match_batch([query_of(s) for s in specs], [manager_of(s) for s in specs])

    def close(self):
        for leaf in self.leaves:
            leaf.release()


def expected(fields, masks, s, **kw):
    return ref.search(oracle, fields, s["groups"], s["shape"], s["k"], masks=masks, after=s.get("after"),
                      total_hits_threshold=s.get("total_hits_threshold", 1000), **{key: s[key] for key in MM_KEYS + FS_KEYS if key in s}, **kw)


def check(ix, fields, masks, specs, name, **kw):
    got = ix.run(specs)
    for i, (s, td) in enumerate(zip(specs, got)):
        same(f"{name}_{i}", td, expected(fields, masks, s, **kw), s["k"], s.get("total_hits_threshold", 1000))
    return got


@pytest.fixture(scope="module")
def fields():
    return mm_ref.build_index()


@pytest.fixture(scope="module")
def masks(fields):
    return ref.function_masks(fields)


@pytest.fixture(scope="module")
def ctx(two_column_postings):
    c = api.GpuContext(device_id=0, max_batch=256)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ix(ctx, fields, masks):
    x = Ix(ctx, fields, masks)
    yield x
    x.close()


def shapes(tokens=TOKENS, field_ids=(0, 1, 2)):
    return (("cross_fields", mm_ref.cross_fields_groups(tokens, field_ids)), ("best_fields", mm_ref.best_fields_groups(tokens, field_ids)))


# ---- 1. shapes x operator x minima x tie breakers x the six mode pairs --------------------------------------------------------------
@pytest.mark.parametrize("score_mode,boost_mode", MODE_PAIRS)
def test_modes(ix, fields, masks, score_mode, boost_mode):
    specs = []
    for shape, groups in shapes():
        n = 3   # cross_fields: groups; best_fields: clauses per group
        for op, m in [("must", 0)] + [("should", m) for m in range(0, n + 2)]:
            for tb, k, thr in zip(TIES, (10, 100, 300, 1), (1000, INT_MAX, 0, 1000)):
                specs.append(dict(groups=groups, shape=shape, k=k, operator=op, msm=m, tie_breaker=tb, total_hits_threshold=thr, functions=FUNCTIONS,
                                  score_mode=score_mode, boost_mode=boost_mode))
    got = check(ix, fields, masks, specs, f"modes_{score_mode}_{boost_mode}")
    d = api.GpuContext.last_diagnostics()
    assert d["items_maxscore"] == 0 and d["items_scan"] >= len(specs)
    for s, td in zip(specs, got):
        if s["operator"] == "should" and s["msm"] == 4:
            assert td.total_hits == 0 and len(td.docs) == 0          # a minimum above what there is: no hits, no error
    assert any(td.total_hits > 0 for s, td in zip(specs, got) if s["operator"] == "must")
    assert ix.searcher.function_score_multi_match_supported(query_of(specs[0]), manager_of(specs[0]))


def test_eight_functions(ix, fields, masks):
    specs = [dict(groups=groups, shape=shape, k=100, tie_breaker=0.3, functions=EIGHT, score_mode=sm, boost_mode=bm)
             for shape, groups in shapes() for sm, bm in (("multiply", "multiply"), ("sum", "sum"))]
    check(ix, fields, masks, specs, "eight")


# ---- 2. REPLACE: keys that differ only in the docid -------------------------------------------------------------------------------------
def test_replace_selects_among_equal_scores(ix, fields, masks):
    for shape, groups in shapes():
        s = dict(groups=groups, shape=shape, k=100, tie_breaker=0.3, functions=FUNCTIONS, boost_mode="replace", total_hits_threshold=INT_MAX)
        exp = expected(fields, masks, s)
        assert int((np.diff(exp[1]) == 0).sum()) >= 90
        same(f"replace_{shape}", ix.run([s])[0], exp, 100, INT_MAX)


# ---- 3. the degenerate forms against the device's two existing routes -----------------------------------------------------------------------
def test_zero_functions_is_the_multi_match_route(ix, fields, masks):
    specs = [dict(groups=groups, shape=shape, k=k, operator=op, msm=m, tie_breaker=0.3, total_hits_threshold=thr)
             for shape, groups in shapes() for op, m in (("should", 0), ("should", 2), ("must", 0)) for k, thr in ((10, 1000), (1024, INT_MAX))]
    got = check(ix, fields, masks, specs, "zero_functions")
    plain = ix.searcher.search_multi_match_batch([query_of(s).inner for s in specs], [manager_of(s) for s in specs])
    for i, (a, b) in enumerate(zip(got, plain)):
        device_equal(f"zero_functions_{i}", a, b)
    # n_functions == 0 and a min_score: the test still applies
    s = dict(groups=specs[0]["groups"], shape="cross_fields", k=100, tie_breaker=0.3, min_score=float(got[0].scores[5]), min_excluded=True,
             total_hits_threshold=INT_MAX)
    td = check(ix, fields, masks, [s], "zero_functions_min_score")[0]
    assert td.total_hits == 5


def test_one_should_group_is_the_function_score_route(ix, fields, masks):
    one_group = [[(0, t, 1.0) for t in TOKENS]]
    inner = api.BooleanQuery(tuple(api.TermQuery(0, t) for t in TOKENS))
    for sm, bm in MODE_PAIRS:
        for k, thr, ms, mex in ((10, 1000, 0.0, False), (1024, INT_MAX, 1.0, True)):
            s = dict(groups=one_group, shape="best_fields", k=k, tie_breaker=0.3, functions=FUNCTIONS, score_mode=sm, boost_mode=bm, min_score=ms,
                     min_excluded=mex, total_hits_threshold=thr)
            flat = api.FunctionScoreQuery(inner, query_of(s).functions, sm, bm, ms, mex)
            device_equal(f"flat_{sm}_{bm}_{k}", ix.run([s])[0], ix.searcher.search_function_score_batch([flat], [manager_of(s)])[0])


def test_the_flat_shapes_the_function_score_entry_refuses(ix, fields, masks):
    clauses = [(0, 2, 1.0), (1, 3, 2.0), (2, 1, 1.0), (0, 4, 1.0)]   # dense enough for the conjunction to have hits
    tq = tuple(api.BoostQuery(api.TermQuery(f, t), b) if b != 1.0 else api.TermQuery(f, t) for f, t, b in clauses)
    cases = [("must", dict(shape="best_fields", operator="must"), api.BooleanQuery(must=tq)),
             ("msm", dict(shape="best_fields", msm=(3,)), api.BooleanQuery(tq, 3)),
             ("dismax", dict(shape="cross_fields", tie_breaker=0.3), api.DisjunctionMaxQuery(tq, 0.3))]
    for name, kw, flat_inner in cases:
        specs = [dict(groups=[clauses], k=k, total_hits_threshold=thr, functions=FUNCTIONS, score_mode=sm, boost_mode=bm, **kw)
                 for k, thr in ((100, 1000), (1024, INT_MAX)) for sm, bm in (("multiply", "multiply"), ("sum", "sum"))]
        got = check(ix, fields, masks, specs, f"flat_{name}")
        assert all(td.total_hits > 0 for td in got)
        old = api.FunctionScoreQuery(flat_inner, query_of(specs[0]).functions)
        assert ix.searcher.function_score_supported(old, manager_of(specs[0])) is False          # the old entry still says no
        assert ix.searcher.function_score_multi_match_supported(query_of(specs[0]), manager_of(specs[0])) is True


# ---- 4. more candidates than the buffer holds -----------------------------------------------------------------------------------------------
def test_compaction_at_k_1024(ix, fields, masks):
    specs = [dict(groups=groups, shape=shape, k=1024, tie_breaker=0.3, total_hits_threshold=INT_MAX, functions=FUNCTIONS, score_mode="sum")
             for shape, groups in shapes((1, 2, 3))]
    got = check(ix, fields, masks, specs, "compaction")
    assert all(td.total_hits >= 12_000 for td in got)   # theta starts at 0: the first round alone brings 8 sub-tiles of candidates


# ---- 5. a query cut into several items, several searcher slices: theta_g carries FINAL keys between the items ----------------------------------
def test_split_items_and_slices(fields, masks):
    c = api.GpuContext(device_id=0, max_batch=64, target_items=4096)
    x = None
    try:
        slicing = (2_000, 2)
        c.set_slicing(*slicing)
        assert len(oracle.corpus_slices(fields[0], slicing)) == 3
        x = Ix(c, fields, masks)
        # the planner cuts by cost (postings; an item is never cheaper than 2^17): the dense terms many times over
        cross = [[(f, t, 1.0) for f in (0, 1, 2, 0)] for t in (1, 2, 1, 2, 1, 2, 1, 2)]
        best = [[(f, t, 1.0) for t in (1, 2, 1, 2, 1, 2, 1, 2)] for f in (0, 1, 2, 0)]
        for shape, groups in (("cross_fields", cross), ("best_fields", best)):
            base = dict(groups=groups, shape=shape, tie_breaker=0.3, functions=FUNCTIONS, boost_mode="sum")
            info = {}
            expected(fields, masks, dict(base, k=100, total_hits_threshold=100), slicing=slicing, info=info)
            per_slice = info["slice_hits"]
            assert len(per_slice) == 3 and min(per_slice) > 100
            for k, thr in ((100, 100), (100, max(per_slice)), (1024, INT_MAX), (1, 0)):
                s = dict(base, k=k, total_hits_threshold=thr)
                got = x.run([s])[0]
                assert api.GpuContext.last_diagnostics()["items_scan"] >= 2
                same(f"split_{shape}_{k}_{thr}", got, expected(fields, masks, s, slicing=slicing), k, thr)
                if thr == max(per_slice):
                    assert got.total_hits > thr and not got.relation_gte      # total_hits exceeds it, no slice does: EQUAL_TO
                if thr == 100:
                    assert got.relation_gte and got.total_hits == sum(per_slice)
    finally:
        if x is not None:
            x.close()
        c.close()


# ---- 6. what queries[i] keeps: masks, another reader version, searchAfter, and the min_score test ------------------------------------------------
def test_inner_filter_and_must_not_next_to_function_masks(ix, fields, masks):
    # FILTER mask 7 is also the first function's mask; MUST_NOT mask 9 is also the second's (never matches a hit then)
    acc = [synth.accept_words(seg, masks[(si, 7)], masks[(si, 9)]) for si, seg in enumerate(fields[0].segments)]
    acc_f = [synth.accept_words(seg, masks[(si, 9)], None) for si, seg in enumerate(fields[0].segments)]
    for shape, groups in shapes(field_ids=(0, 1)):
        s = dict(groups=groups, shape=shape, k=200, tie_breaker=0.3, filter=(7,), must_not=(9,), functions=FUNCTIONS)
        same(f"masks_{shape}", ix.run([s])[0], expected(fields, masks, s, accept=acc), 200, 1000)
        s = dict(groups=groups, shape=shape, k=50, operator="must", tie_breaker=0.3, filter=(9,), total_hits_threshold=INT_MAX, functions=FUNCTIONS,
                 score_mode="sum", boost_mode="replace")
        same(f"filter_{shape}", ix.run([s])[0], expected(fields, masks, s, accept=acc_f), 50, INT_MAX)


def test_fork_with_other_live_docs(ctx, ix, fields, masks):
    lives, forks = [], []
    try:
        for si, (seg, leaf) in enumerate(zip(fields[0].segments, ix.leaves)):
            n = (seg.max_doc + 63) // 64
            live = seg.live_bits[:n] & ~synth.random_mask(seg.max_doc, 0.05, 900 + si)[:n]
            lives.append(live)
            forks.append(leaf.fork(live))
        for (si, mid), bits in masks.items():
            forks[si].set_mask(mid, bits)
        searcher = api.GpuIndexSearcher(ctx, forks, ix.stats)
        for shape, groups in shapes(field_ids=(0, 1)):
            s = dict(groups=groups, shape=shape, k=100, tie_breaker=0.3, total_hits_threshold=INT_MAX, functions=FUNCTIONS, score_mode="sum", boost_mode="sum")
            got = searcher.search_function_score_multi_match_batch([query_of(s)], [manager_of(s)])[0]
            same(f"fork_{shape}", got, expected(fields, masks, s, live=lives), 100, INT_MAX)
            same(f"fork_parent_{shape}", ix.run([s])[0], expected(fields, masks, s), 100, INT_MAX)   # the first version still sees its own liveDocs
    finally:
        for f in forks:
            f.release()


@pytest.mark.parametrize("boost_mode", ["multiply", "sum", "replace"])
def test_search_after_pages(ix, fields, masks, boost_mode):
    for shape, groups in shapes(field_ids=(0, 1)):
        base = dict(groups=groups, shape=shape, tie_breaker=0.3, total_hits_threshold=INT_MAX, functions=FUNCTIONS, boost_mode=boost_mode)
        full = ix.run([dict(base, k=150)])[0]
        after, docs, scores = None, [], []
        for page in range(3):
            s = dict(base, k=50, after=after)
            got = ix.run([s])[0]
            same(f"after_{shape}_{boost_mode}_{page}", got, expected(fields, masks, s), 50, INT_MAX)
            docs += got.docs.tolist()
            scores += got.scores.view(np.uint32).tolist()
            after = (int(got.docs[-1]), float(got.scores[-1]))
        assert docs == full.docs.tolist() and scores == full.scores.view(np.uint32).tolist()   # three pages == the first 3k of one call


@pytest.mark.parametrize("min_excluded", [False, True])
def test_min_score_at_the_500th_final_score(ix, fields, masks, min_excluded):
    for shape, groups in shapes():
        base = dict(groups=groups, shape=shape, k=1024, tie_breaker=0.3, total_hits_threshold=INT_MAX, functions=FUNCTIONS)
        top = expected(fields, masks, base)
        ms = float(top[1][499])
        s = dict(base, min_score=ms, min_excluded=min_excluded)
        exp = expected(fields, masks, s)
        assert 0 < exp[2] < top[2]
        got = ix.run([s])[0]
        same(f"min_score_{shape}_{min_excluded}", got, exp, 1024, INT_MAX)
        assert (f32(ms) in got.scores) == (not min_excluded)


# ---- 7. a mixed batch -------------------------------------------------------------------------------------------------------------------------
def test_mixed_batch_of_64(ix, fields, masks):
    rng = np.random.default_rng(640)
    specs = []
    for i in range(64):
        tokens = tuple(int(t) for t in rng.choice([1, 2, 3, 4, 5, 6, 7, 9, 11, 12, 13], size=int(rng.integers(1, 5)), replace=False))
        fids = tuple(int(f) for f in rng.choice([0, 1, 2], size=int(rng.integers(1, 4)), replace=False))
        boosts = {int(f): float(rng.choice([1.0, 2.0, 0.5])) for f in fids}
        shape = ("cross_fields", "best_fields")[i % 2]
        groups = (mm_ref.cross_fields_groups if i % 2 == 0 else mm_ref.best_fields_groups)(tokens, fids, boosts)
        op = "must" if i % 5 == 0 else "should"
        msm = 0 if op == "must" else int(rng.integers(0, 3))
        n = i % 9   # 0..8 functions
        funcs = tuple((int(rng.choice([0, 7, 9])), float(f32(rng.choice([0.25, 0.5, 1.25, 2.5, 3.0, 11.0])))) for _ in range(n))
        sm, bm = MODE_PAIRS[int(rng.integers(0, 6))]
        specs.append(dict(groups=groups, shape=shape, k=int(rng.choice([1, 10, 100, 300, 1024])), operator=op, msm=msm,
                          tie_breaker=float(rng.choice(TIES)), total_hits_threshold=int(rng.choice([0, 100, 1000, INT_MAX])), functions=funcs,
                          score_mode=sm, boost_mode=bm, min_score=float(rng.choice([0.0, 0.0, 1.0])), min_excluded=bool(i % 3 == 0)))
    check(ix, fields, masks, specs, "mixed")


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------------
def _refused(searcher, q, mgr, code=_lib.NRTGPU_ERR_UNSUPPORTED, tweak=None):
    m, gs, fs = searcher._marshal_function_score_multi_match([q], [mgr])
    if tweak:
        tweak(m.queries[0], gs[0], fs[0])
    out = (_lib.TopDocs * 1)()
    L = _lib.load()
    assert L.nrtgpu_search_function_score_multi_match_batch(searcher.ctx._h, searcher._segs, searcher._bases, len(searcher.leaves), m.queries, gs, fs, 1,
                                                            out) == code
    assert len(L.nrtgpu_last_error().decode()) > 20
    assert L.nrtgpu_function_score_multi_match_supported(searcher.ctx._h, searcher._segs, len(searcher.leaves), m.queries, gs, fs) == code


def _plain_search_works(searcher, fields):
    got = searcher.search_batch([api.BooleanQuery((api.TermQuery(0, 2), api.TermQuery(0, 7)))], [api.TopScoreDocCollectorManager(10)])[0]
    assert_same("plain_after_refusal", got, oracle.search_bm25(fields[0], [2, 7], 10), 10, 1000)


def test_refusals(ix, fields, masks):
    mgr = api.TopScoreDocCollectorManager(10)
    INV = _lib.NRTGPU_ERR_INVALID_ARG
    cross_groups, best_groups = mm_ref.cross_fields_groups(TOKENS), mm_ref.best_fields_groups(TOKENS)
    cross = ref.to_query(api, cross_groups, "cross_fields", "should", 0, 0.3, FUNCTIONS)
    best_must = ref.to_query(api, best_groups, "best_fields", "must", 0, 0.3, FUNCTIONS)
    ix.leaves[0].set_mask(13, masks[(0, 7)])   # resident on ONE leaf of the call only
    try:
        _refused(ix.searcher, ref.to_query(api, cross_groups, "cross_fields", functions=((13, 2.0),)), mgr)         # as a function's mask
        assert "13" in _lib.load().nrtgpu_last_error().decode()
        _refused(ix.searcher, ref.to_query(api, cross_groups, "cross_fields", functions=FUNCTIONS, filter=(13,)), mgr)   # as the inner FILTER
        _plain_search_works(ix.searcher, fields)
    finally:
        ix.leaves[0].set_mask(13, None)
    # the multi-match entry's
    _refused(ix.searcher, cross, api.TopScoreDocCollectorManager(10, None, 1000, 0.5))                       # min_competitive_score
    _refused(ix.searcher, best_must, mgr, tweak=lambda q, g, f: setattr(q.terms[1], "occur", 0))            # MUST next to SHOULD in a group
    _refused(ix.searcher, ref.to_query(api, [[(0, 2, 1.0), (1, 2, 2.0 ** -20)], [(0, 4, 1.0)]], "cross_fields", functions=FUNCTIONS), mgr)   # fixed point
    _refused(ix.searcher, ref.to_query(api, [[(0, 1 + i % 12, 1.0) for i in range(33)]], "best_fields", functions=FUNCTIONS), mgr)
    _refused(ix.searcher, cross, mgr, INV, tweak=lambda q, g, f: setattr(q, "disjunction_max", 1))
    _refused(ix.searcher, cross, mgr, INV, tweak=lambda q, g, f: setattr(q.terms[0], "occur", 1))           # SUM_OF_MAX with an occur
    _refused(ix.searcher, best_must, mgr, INV, tweak=lambda q, g, f: setattr(q, "min_should_match", 1))
    _refused(ix.searcher, cross, mgr, INV, tweak=lambda q, g, f: setattr(g, "n_groups", 9))
    _refused(ix.searcher, cross, mgr, INV, tweak=lambda q, g, f: setattr(g, "tie_breaker", 1.5))
    _refused(ix.searcher, cross, api.TopScoreDocCollectorManager(0), INV)                                    # validate_query's
    # the function-score entry's
    _refused(ix.searcher, ref.to_query(api, cross_groups, "cross_fields", functions=((0, -2.0),)), mgr)
    _refused(ix.searcher, ref.to_query(api, cross_groups, "cross_fields", functions=((0, 0.0),)), mgr, INV)
    _refused(ix.searcher, cross, mgr, INV, tweak=lambda q, g, f: setattr(f, "n_functions", 9))
    _refused(ix.searcher, cross, mgr, INV, tweak=lambda q, g, f: setattr(f, "boost_mode", 3))
    _refused(ix.searcher, cross, mgr, INV, tweak=lambda q, g, f: setattr(f, "min_score", -1.0))
    # the groups are checked before the functions
    _refused(ix.searcher, ref.to_query(api, best_groups, "best_fields", "must", functions=((0, 0.0),)), mgr,
             tweak=lambda q, g, f: setattr(q.terms[1], "occur", 0))
    _plain_search_works(ix.searcher, fields)
    assert ix.searcher.function_score_multi_match_supported(cross, mgr) is True
    assert ix.searcher.function_score_multi_match_supported(best_must, mgr) is True
    s = dict(groups=cross_groups, shape="cross_fields", k=10, tie_breaker=0.3, functions=FUNCTIONS)
    same("after_refusals", ix.run([s])[0], expected(fields, masks, s), 10, 1000)


@pytest.mark.parametrize("flag", [_lib.NRTGPU_FLAG_PACKED_POSTINGS, _lib.NRTGPU_FLAG_NO_FIXED_POINT])
def test_contexts_the_route_refuses(fields, masks, flag):
    c = api.GpuContext(device_id=0, max_batch=16, flags=flag)
    x = None
    try:
        x = Ix(c, fields, masks)
        q = ref.to_query(api, mm_ref.cross_fields_groups(TOKENS), "cross_fields", "should", 0, 0.3, FUNCTIONS)
        mgr = api.TopScoreDocCollectorManager(10)
        _refused(x.searcher, q, mgr)
        assert x.searcher.function_score_multi_match_supported(q, mgr) is False
        _plain_search_works(x.searcher, fields)
    finally:
        if x is not None:
            x.close()
        c.close()
