"""Multi-match queries (cross_fields: a BooleanQuery over DisjunctionMaxQuery groups; best_fields: a DisjunctionMaxQuery over
BooleanQuery groups) through the C ABI on the device, against tests/_multi_match_ref.py (the oracle's BM25 arithmetic, collectors
and merge around the two-level rules) and, where a grouping degenerates to a flat query, against the device's existing routes.
Bit-exact: docids, ranks, float32 score bits, the exact total_hits and the relation.  Needs a real MI355X."""
import numpy as np
import pytest

from nrtsearch_amd import _lib, api, synth
from oracle import oracle

from tests import _multi_match_ref as ref
from tests.test_parity_gpu import assert_same

pytestmark = pytest.mark.gpu
f32 = np.float32
INT_MAX = 2**31 - 1
TIES = (0.0, 1.0, 0.3, float(np.nextafter(f32(1), f32(0))))
TOKENS = (2, 4, 7)


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


class Ix:
    def __init__(self, ctx, fields):
        self.ctx = ctx
        self.leaves, self.stats = ref.upload(api, ctx, fields)
        self.searcher = api.GpuIndexSearcher(ctx, self.leaves, self.stats)

    def run(self, specs):
        """specs: dicts of ref.search's arguments (groups, shape, k, operator, msm, tie_breaker, total_hits_threshold, after) -> TopDocs."""
        qs = [ref.to_query(api, s["groups"], s["shape"], s.get("operator", "should"), s.get("msm", 0), s.get("tie_breaker", 0.0),
                           s.get("filter", ()), s.get("must_not", ())) for s in specs]
        mgrs = [api.TopScoreDocCollectorManager(s["k"], api.ScoreDoc(*s["after"]) if s.get("after") else None, s.get("total_hits_threshold", 1000))
                for s in specs]
        return self.searcher.search_multi_match_batch(qs, mgrs)

    def close(self):
        for leaf in self.leaves:
            leaf.release()


def expected(fields, s, **kw):
    return ref.search(oracle, fields, s["groups"], s["shape"], s["k"], s.get("operator", "should"), s.get("msm", 0), s.get("tie_breaker", 0.0),
                      after=s.get("after"), total_hits_threshold=s.get("total_hits_threshold", 1000), **kw)


def check(ix, fields, specs, name, **kw):
    got = ix.run(specs)
    for i, (s, td) in enumerate(zip(specs, got)):
        same(f"{name}_{i}", td, expected(fields, s, **kw), s["k"], s.get("total_hits_threshold", 1000))
    return got


@pytest.fixture(scope="module")
def fields():
    return ref.build_index()


@pytest.fixture(scope="module")
def ctx(two_column_postings):
    c = api.GpuContext(device_id=0, max_batch=256)
    yield c
    c.close()


@pytest.fixture(scope="module")
def masks(fields):
    return {(si, mid): synth.random_mask(seg.max_doc, dens, 10 * mid + si) for si, seg in enumerate(fields[0].segments)
            for mid, dens in ((7, 0.4), (9, 0.1))}


@pytest.fixture(scope="module")
def ix(ctx, fields, masks):
    x = Ix(ctx, fields)
    for (si, mid), bits in masks.items():
        x.leaves[si].set_mask(mid, bits)
    yield x
    x.close()


# ---- 1. shapes x operator x minima x tie breakers ----------------------------------------------------------------------------
def test_cross_fields(ix, fields):
    g3 = ref.cross_fields_groups(TOKENS, (0, 1, 2), {1: 2.0})                                  # three tokens x three fields, a boosted field
    g2 = ref.cross_fields_groups((1, 13, ref.TERM_NOWHERE, 12), (0, 1))                      # a term one leaf lacks, one no leaf holds
    specs = [dict(groups=g, shape="cross_fields", k=k, operator=op, msm=m, tie_breaker=tb, total_hits_threshold=thr)
             for g, n in ((g3, 3), (g2, 4)) for op, m in [("must", 0)] + [("should", m) for m in range(0, n + 2)]
             for tb, k, thr in zip(TIES, (10, 100, 300, 1), (1000, INT_MAX, 0, 1000))]
    got = check(ix, fields, specs, "cross")
    d = api.GpuContext.last_diagnostics()
    assert d["items_maxscore"] == 0 and d["items_scan"] >= len(specs)
    for s, td in zip(specs, got):
        if s["operator"] == "should" and s["msm"] > len(s["groups"]):
            assert td.total_hits == 0 and len(td.docs) == 0          # a minimum above n_groups: no hits, no error
        if s["groups"] is g2 and s["operator"] == "must":
            assert td.total_hits == 0                                # a MUST group whose terms no leaf holds
    assert any(td.total_hits > 0 for s, td in zip(specs, got) if s["operator"] == "must")
    for s in specs[:4]:
        assert ix.searcher.multi_match_supported(ref.to_query(api, s["groups"], "cross_fields", s["operator"], s["msm"], s["tie_breaker"]),
                                                 api.TopScoreDocCollectorManager(10))


def test_best_fields(ix, fields):
    g3 = ref.best_fields_groups(TOKENS, (0, 1, 2), {2: 3.0})
    g2 = ref.best_fields_groups((1, 13, ref.TERM_NOWHERE, 12), (0, 1))
    variants = [("must", 0), ("should", 0), ("should", 1), ("should", 2), ("should", (1, 3, 2)), ("should", (4, 1, 0)), ("should", 5)]
    specs = []
    for g in (g3, g2):
        for op, m in variants:
            if isinstance(m, tuple):
                m = m[:len(g)]
            for tb, k, thr in zip(TIES, (10, 100, 300, 1), (1000, INT_MAX, 0, 1000)):
                specs.append(dict(groups=g, shape="best_fields", k=k, operator=op, msm=m, tie_breaker=tb, total_hits_threshold=thr))
    got = check(ix, fields, specs, "best")
    for s, td in zip(specs, got):
        if s["operator"] == "must" and s["groups"] is g2:
            assert td.total_hits == 0                                # every group holds the term no leaf holds
        if s["msm"] == 5:
            assert td.total_hits == 0                                # more than any group holds
    assert any(td.total_hits > 0 for s, td in zip(specs, got) if s["operator"] == "must")


# ---- 2. degenerate groupings against the device's existing routes (not through the new reference) -------------------------------
def _flat_equal(name, got, flat):
    assert got.docs.tolist() == flat.docs.tolist(), f"{name}: docids"
    assert got.scores.view(np.uint32).tolist() == flat.scores.view(np.uint32).tolist(), f"{name}: score bits"
    assert (got.total_hits, got.relation_gte) == (flat.total_hits, flat.relation_gte), f"{name}: {got.total_hits} vs {flat.total_hits}"


def test_degenerate_groupings_are_the_existing_routes(ix, fields, masks):
    c = api.GpuContext(device_id=0, max_batch=64, flags=_lib.NRTGPU_FLAG_NO_PRUNE)
    x = None
    try:
        x = Ix(c, fields)
        clauses = [(0, 2, 1.0), (1, 5, 2.0), (2, 9, 1.0), (0, 13, 1.0), (1, 1, 1.0)]
        tq = tuple(api.BoostQuery(api.TermQuery(f, t), b) if b != 1.0 else api.TermQuery(f, t) for f, t, b in clauses)
        singles = [[cl] for cl in clauses]
        for k, thr in ((10, 1000), (200, 100), (1024, INT_MAX)):
            mgr = api.TopScoreDocCollectorManager(k, None, thr)
            flat = x.searcher.search_batch([api.BooleanQuery(tq), api.BooleanQuery(tq, 3), api.BooleanQuery(must=tq), api.DisjunctionMaxQuery(tq, 0.0)], [mgr] * 4)
            assert api.GpuContext.last_diagnostics()["items_maxscore"] == 0
            got = x.run([dict(groups=singles, shape="cross_fields", k=k, tie_breaker=0.7, total_hits_threshold=thr),       # one clause per group
                         dict(groups=singles, shape="cross_fields", k=k, msm=3, total_hits_threshold=thr),
                         dict(groups=singles, shape="cross_fields", k=k, operator="must", total_hits_threshold=thr),
                         dict(groups=singles, shape="best_fields", k=k, tie_breaker=0.0, total_hits_threshold=thr),
                         dict(groups=[clauses], shape="best_fields", k=k, tie_breaker=0.3, total_hits_threshold=thr),      # one group
                         dict(groups=[clauses], shape="best_fields", k=k, msm=3, total_hits_threshold=thr),
                         dict(groups=[clauses], shape="best_fields", k=k, operator="must", total_hits_threshold=thr),
                         dict(groups=[clauses], shape="cross_fields", k=k, tie_breaker=0.0, total_hits_threshold=thr)])
            for name, g, f in (("singles_sum", 0, 0), ("singles_msm", 1, 1), ("singles_must", 2, 2), ("singles_dismax", 3, 3),
                               ("one_group_sum", 4, 0), ("one_group_msm", 5, 1), ("one_group_must", 6, 2), ("one_group_dismax", 7, 3)):
                _flat_equal(f"{name}_{k}", got[g], flat[f])
    finally:
        if x is not None:
            x.close()
        c.close()
    # a tie breaker > 0 runs on the flat route that prunes: ScoreMode.COMPLETE keeps its count exact
    mgr = api.TopScoreDocCollectorManager(100, None, INT_MAX)
    flat = ix.searcher.search_batch([api.DisjunctionMaxQuery(tq, 0.3)], [mgr])[0]
    got = ix.run([dict(groups=singles, shape="best_fields", k=100, tie_breaker=0.3, total_hits_threshold=INT_MAX),
                  dict(groups=[clauses], shape="cross_fields", k=100, tie_breaker=0.3, total_hits_threshold=INT_MAX)])
    _flat_equal("singles_tie", got[0], flat)
    _flat_equal("one_group_tie", got[1], flat)


# ---- 3. more candidates than the buffer holds ------------------------------------------------------------------------------------
def test_compaction_at_k_1024(ix, fields):
    specs = [dict(groups=ref.cross_fields_groups((1, 2, 3), (0, 1, 2)), shape="cross_fields", k=1024, tie_breaker=0.3, total_hits_threshold=INT_MAX),
             dict(groups=ref.best_fields_groups((1, 2, 3), (0, 1, 2)), shape="best_fields", k=1024, tie_breaker=0.3, total_hits_threshold=INT_MAX)]
    got = check(ix, fields, specs, "compaction")
    assert all(td.total_hits >= 12_000 for td in got)   # theta starts at 0: the first round alone brings 8 sub-tiles of candidates


# ---- 4. a query cut into several items, several searcher slices --------------------------------------------------------------------
def test_split_items_and_slices(fields):
    c = api.GpuContext(device_id=0, max_batch=64, target_items=4096)
    x = None
    try:
        slicing = (2_000, 2)
        c.set_slicing(*slicing)
        assert len(oracle.corpus_slices(fields[0], slicing)) == 3
        x = Ix(c, fields)
        # the planner cuts by cost (postings; an item is never cheaper than 2^17): the dense terms many times over
        cross = [[(f, t, 1.0) for f in (0, 1, 2, 0)] for t in (1, 2, 1, 2, 1, 2, 1, 2)]
        best = [[(f, t, 1.0) for t in (1, 2, 1, 2, 1, 2, 1, 2)] for f in (0, 1, 2, 0)]
        for shape, groups in (("cross_fields", cross), ("best_fields", best)):
            info = {}
            ref.search(oracle, fields, groups, shape, 100, tie_breaker=0.3, total_hits_threshold=100, slicing=slicing, info=info)
            per_slice = info["slice_hits"]
            assert len(per_slice) == 3 and min(per_slice) > 100
            for k, thr in ((100, 100), (100, max(per_slice)), (1024, INT_MAX), (1, 0)):
                s = dict(groups=groups, shape=shape, k=k, tie_breaker=0.3, total_hits_threshold=thr)
                got = x.run([s])[0]
                assert api.GpuContext.last_diagnostics()["items_scan"] >= 2
                same(f"split_{shape}_{k}_{thr}", got, expected(fields, s, slicing=slicing), k, thr)
                if thr == max(per_slice):
                    assert got.total_hits > thr and not got.relation_gte      # total_hits exceeds it, no slice does: EQUAL_TO
                if thr == 100:
                    assert got.relation_gte and got.total_hits == sum(per_slice)
    finally:
        if x is not None:
            x.close()
        c.close()


# ---- 5. what queries[i] keeps: masks, another reader version, searchAfter ------------------------------------------------------------
def test_filter_and_must_not_masks(ix, fields, masks):
    acc = [synth.accept_words(seg, masks[(si, 7)], masks[(si, 9)]) for si, seg in enumerate(fields[0].segments)]
    acc_f = [synth.accept_words(seg, masks[(si, 7)], None) for si, seg in enumerate(fields[0].segments)]
    for shape, groups in (("cross_fields", ref.cross_fields_groups(TOKENS)), ("best_fields", ref.best_fields_groups(TOKENS))):
        s = dict(groups=groups, shape=shape, k=200, tie_breaker=0.3, filter=(7,), must_not=(9,))
        same(f"masks_{shape}", ix.run([s])[0], expected(fields, s, accept=acc), 200, 1000)
        s = dict(groups=groups, shape=shape, k=50, operator="must", tie_breaker=0.3, filter=(7,), total_hits_threshold=INT_MAX)
        same(f"filter_{shape}", ix.run([s])[0], expected(fields, s, accept=acc_f), 50, INT_MAX)


def test_fork_with_other_live_docs(ctx, ix, fields):
    lives, forks = [], []
    try:
        for si, (seg, leaf) in enumerate(zip(fields[0].segments, ix.leaves)):
            n = (seg.max_doc + 63) // 64
            live = seg.live_bits[:n] & ~synth.random_mask(seg.max_doc, 0.05, 900 + si)[:n]
            lives.append(live)
            forks.append(leaf.fork(live))
        searcher = api.GpuIndexSearcher(ctx, forks, ix.stats)
        for shape, groups in (("cross_fields", ref.cross_fields_groups(TOKENS)), ("best_fields", ref.best_fields_groups(TOKENS))):
            q = ref.to_query(api, groups, shape, "should", 0, 0.3)
            got = searcher.search_multi_match_batch([q], [api.TopScoreDocCollectorManager(100, None, INT_MAX)])[0]
            exp = ref.search(oracle, fields, groups, shape, 100, tie_breaker=0.3, total_hits_threshold=INT_MAX, live=lives)
            same(f"fork_{shape}", got, exp, 100, INT_MAX)
            # the first version still sees its own liveDocs
            s = dict(groups=groups, shape=shape, k=100, tie_breaker=0.3, total_hits_threshold=INT_MAX)
            same(f"fork_parent_{shape}", ix.run([s])[0], expected(fields, s), 100, INT_MAX)
    finally:
        for f in forks:
            f.release()


@pytest.mark.parametrize("shape", ["cross_fields", "best_fields"])
def test_search_after_pages(ix, fields, shape):
    groups = ref.cross_fields_groups(TOKENS) if shape == "cross_fields" else ref.best_fields_groups(TOKENS)
    full = ix.run([dict(groups=groups, shape=shape, k=150, tie_breaker=0.3, total_hits_threshold=INT_MAX)])[0]
    after, docs, scores = None, [], []
    for page in range(3):
        s = dict(groups=groups, shape=shape, k=50, tie_breaker=0.3, total_hits_threshold=INT_MAX, after=after)
        got = ix.run([s])[0]
        same(f"after_{shape}_{page}", got, expected(fields, s), 50, INT_MAX)
        docs += got.docs.tolist()
        scores += got.scores.view(np.uint32).tolist()
        after = (int(got.docs[-1]), float(got.scores[-1]))
    assert docs == full.docs.tolist() and scores == full.scores.view(np.uint32).tolist()   # three pages == the first 3k of one call


# ---- 6. a clause in two groups; a mixed batch ------------------------------------------------------------------------------------------
def test_a_clause_in_two_groups(ix, fields):
    shared = (0, 4, 1.0)
    specs = [dict(groups=[[shared, (1, 2, 1.0)], [shared, (1, 7, 1.0)], [(2, 4, 1.0)]], shape="cross_fields", k=100, tie_breaker=0.3, msm=2),
             dict(groups=[[shared, (1, 2, 1.0)], [shared, (1, 7, 1.0)], [(2, 4, 1.0)]], shape="best_fields", k=100, tie_breaker=0.3, msm=(2, 1, 1)),
             dict(groups=[[shared, shared], [(1, 4, 1.0)]], shape="cross_fields", k=100, tie_breaker=1.0, operator="must")]
    check(ix, fields, specs, "shared_clause")


def test_mixed_batch_of_64(ix, fields):
    rng = np.random.default_rng(64)
    specs = []
    for i in range(64):
        tokens = tuple(int(t) for t in rng.choice([1, 2, 3, 4, 5, 6, 7, 9, 11, 12, 13], size=int(rng.integers(1, 5)), replace=False))
        fids = tuple(int(f) for f in rng.choice([0, 1, 2], size=int(rng.integers(1, 4)), replace=False))
        boosts = {int(f): float(rng.choice([1.0, 2.0, 0.5])) for f in fids}
        shape = ("cross_fields", "best_fields")[i % 2]
        groups = (ref.cross_fields_groups if i % 2 == 0 else ref.best_fields_groups)(tokens, fids, boosts)
        op = "must" if i % 5 == 0 else "should"
        msm = 0 if op == "must" else int(rng.integers(0, 3))
        specs.append(dict(groups=groups, shape=shape, k=int(rng.choice([1, 10, 100, 300, 1024])), operator=op, msm=msm,
                          tie_breaker=float(rng.choice(TIES)), total_hits_threshold=int(rng.choice([0, 100, 1000, INT_MAX]))))
    check(ix, fields, specs, "mixed")


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------------
def _refused(searcher, q, mgr, code=_lib.NRTGPU_ERR_UNSUPPORTED, tweak=None):
    m, gs = searcher._marshal_multi_match([q], [mgr])
    if tweak:
        tweak(m.queries[0], gs[0])
    out = (_lib.TopDocs * 1)()
    L = _lib.load()
    assert L.nrtgpu_search_multi_match_batch(searcher.ctx._h, searcher._segs, searcher._bases, len(searcher.leaves), m.queries, gs, 1, out) == code
    assert len(L.nrtgpu_last_error().decode()) > 20
    assert L.nrtgpu_multi_match_supported(searcher.ctx._h, searcher._segs, len(searcher.leaves), m.queries, gs) == code


def _plain_search_works(searcher, fields):
    got = searcher.search_batch([api.BooleanQuery((api.TermQuery(0, 2), api.TermQuery(0, 7)))], [api.TopScoreDocCollectorManager(10)])[0]
    assert_same("plain_after_refusal", got, oracle.search_bm25(fields[0], [2, 7], 10), 10, 1000)


def test_refusals(ix, fields, masks):
    mgr = api.TopScoreDocCollectorManager(10)
    INV = _lib.NRTGPU_ERR_INVALID_ARG
    cross = ref.to_query(api, ref.cross_fields_groups(TOKENS), "cross_fields", "should", 0, 0.3)
    best_must = ref.to_query(api, ref.best_fields_groups(TOKENS), "best_fields", "must", 0, 0.3)
    ix.leaves[0].set_mask(13, masks[(0, 7)])   # resident on ONE leaf of the call only
    try:
        _refused(ix.searcher, ref.to_query(api, ref.cross_fields_groups(TOKENS), "cross_fields", filter=(13,)), mgr)
        _plain_search_works(ix.searcher, fields)
    finally:
        ix.leaves[0].set_mask(13, None)
    _refused(ix.searcher, cross, api.TopScoreDocCollectorManager(10, None, 1000, 0.5))                       # min_competitive_score
    _refused(ix.searcher, best_must, mgr, tweak=lambda q, g: setattr(q.terms[1], "occur", 0))               # MUST next to SHOULD in a group
    _refused(ix.searcher, ref.to_query(api, [[(0, 2, 1.0), (1, 2, 2.0 ** -20)], [(0, 4, 1.0)]], "cross_fields"), mgr)   # outside the fixed-point range
    _refused(ix.searcher, ref.to_query(api, [[(0, 1 + i % 12, 1.0) for i in range(33)]], "best_fields"), mgr)
    _refused(ix.searcher, cross, mgr, INV, tweak=lambda q, g: setattr(q, "disjunction_max", 1))
    _refused(ix.searcher, cross, mgr, INV, tweak=lambda q, g: setattr(q, "tie_breaker", 0.5))
    _refused(ix.searcher, cross, mgr, INV, tweak=lambda q, g: setattr(q.terms[0], "occur", 1))              # SUM_OF_MAX with an occur
    _refused(ix.searcher, best_must, mgr, INV, tweak=lambda q, g: setattr(q, "min_should_match", 1))
    _refused(ix.searcher, cross, mgr, INV, tweak=lambda q, g: setattr(g, "n_groups", 9))
    _refused(ix.searcher, cross, mgr, INV, tweak=lambda q, g: setattr(g, "n_groups", 4))                    # an empty group
    _refused(ix.searcher, cross, mgr, INV, tweak=lambda q, g: setattr(g, "tie_breaker", 1.5))
    _refused(ix.searcher, cross, mgr, INV, tweak=lambda q, g: setattr(g, "shape", 2))
    _refused(ix.searcher, cross, api.TopScoreDocCollectorManager(0), INV)                                    # validate_query's
    _plain_search_works(ix.searcher, fields)
    assert ix.searcher.multi_match_supported(cross, mgr) is True and ix.searcher.multi_match_supported(best_must, mgr) is True
    s = dict(groups=ref.cross_fields_groups(TOKENS), shape="cross_fields", k=10, tie_breaker=0.3)
    same("after_refusals", ix.run([s])[0], expected(fields, s), 10, 1000)


@pytest.mark.parametrize("flag", [_lib.NRTGPU_FLAG_PACKED_POSTINGS, _lib.NRTGPU_FLAG_NO_FIXED_POINT])
def test_contexts_the_route_refuses(fields, flag):
    c = api.GpuContext(device_id=0, max_batch=16, flags=flag)
    x = None
    try:
        x = Ix(c, fields)
        q = ref.to_query(api, ref.cross_fields_groups(TOKENS), "cross_fields", "should", 0, 0.3)
        mgr = api.TopScoreDocCollectorManager(10)
        _refused(x.searcher, q, mgr)
        assert x.searcher.multi_match_supported(q, mgr) is False
        _plain_search_works(x.searcher, fields)
    finally:
        if x is not None:
            x.close()
        c.close()
