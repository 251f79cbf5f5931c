"""The gather route of the filtered knn requests (nrtgpu_set_knn_gather; vectors_gather.cpp, knn_accept_rows_kernel,
knn_gather_score_kernel, knn_gather_bytes_kernel) on the GPU.

Every case runs the same request three ways -- knob 0 (the full pass over every row), knob 1000 (only the accepted rows) and a
reference in numpy that scores the accepted, live rows that have a vector with the oracle's vector_score (float fields) or
nrtgpu_byte_vector_score (byte fields) -- and the three agree with == on docids, score BITS and total_hits: no tolerance anywhere.
Each case also reads the route off the statistics: the full pass adds every row of the field to knn_rows, the gather route exactly
the accepted rows, and nothing to knn_sketch_launches / knn_second_passes."""
import ctypes as C

import numpy as np
import pytest

from nrtsearch_amd import _lib, api

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
F = 3
FLOAT_SIMS = ["cosine", "dot_product", "l2_norm", "max_inner_product", "normalized_cosine"]
BYTE_SIMS = ["cosine", "dot_product", "l2_norm", "max_inner_product"]
COUNTERS = ("knn_panels", "knn_score_launches", "knn_rows", "knn_sketch_launches", "knn_second_passes")
M_MAIN, M_5PCT, M_HALF_PCT, M_NOTHING = 1, 2, 3, 4
KNN_CAP = 1 << 18     # keys of one candidate list (vectors.cpp: kKnnCap, vectors_bytes.cpp: kKnnBytesCap)


@pytest.fixture(scope="module")
def ctx():
    c = api.GpuContext(device_id=0, max_batch=64, collect_timing=True)
    yield c
    c.close()


def pack_bits(flags):
    padded = np.zeros(((len(flags) + 63) // 64) * 64, dtype=bool)
    padded[: len(flags)] = flags
    return np.packbits(padded.reshape(-1, 64), axis=1, bitorder="little").view(np.uint64).reshape(-1)


def gen_rows(rng, kind, n, dim):
    if kind == "float":
        return rng.standard_normal((n, dim)).astype(f32)
    return rng.integers(-128, 128, size=(n, dim), dtype=np.int8)


class Leaf:
    def __init__(self, base, max_doc, rows, o2d, live, masks):
        self.base, self.max_doc, self.rows, self.o2d, self.live, self.masks = base, max_doc, rows, o2d, live, masks


class Index:
    """Five leaves: 4 097 docs, a row each; 70 100 docs, a row on every third (a sparse ord -> doc map); 1 doc; 500 docs WITHOUT the
    field; 300 docs with rows none of which any mask accepts.  Masks: M_MAIN (bits at docs 0, 63, 64 and max_doc - 1 of the two
    large leaves, docs without a vector, docs liveDocs delete, eight docs that hold one identical row, on byte fields a zero row),
    M_5PCT / M_HALF_PCT (4.95 % / 0.5 % of the field's rows), M_NOTHING."""

    def __init__(self, ctx, kind, dim, seed=1):
        rng = np.random.default_rng(seed * 1000 + dim)
        self.kind, self.dim = kind, dim
        n0, n1 = 4097, 70100
        o2d1 = np.arange(0, n1, 3, dtype=np.int32)
        rows0, rows1 = gen_rows(rng, kind, n0, dim), gen_rows(rng, kind, len(o2d1), dim)
        # M_MAIN
        m0 = np.zeros(n0, dtype=bool)
        m0[[0, 63, 64, n0 - 1]] = True
        m0[rng.choice(n0, size=40, replace=False)] = True
        m1 = np.zeros(n1, dtype=bool)
        m1[[0, 63, 64, n1 - 1]] = True                  # (63 and 0 hold a row, 64 and 70 099 do not)
        m1[rng.choice(n1, size=200, replace=False)] = True
        assert (np.flatnonzero(m1) % 3 != 0).sum() > 50  # accepted docs that have no vector
        # eight accepted docs with one identical row, in both leaves
        self.tie_row = gen_rows(rng, kind, 1, dim)[0]
        tie0 = np.array([5, 700, 4000])
        tie1 = np.array([9, 3003, 30000, 60000, 69999])
        m0[tie0] = True
        m1[tie1] = True
        rows0[tie0] = self.tie_row
        rows1[tie1 // 3] = self.tie_row
        self.tie_docs = sorted(tie0.tolist() + (n0 + tie1).tolist())
        self.zero_doc = None
        if kind == "byte":
            m0[77] = True
            rows0[77] = 0
            self.zero_doc = 77
        # liveDocs: a twentieth of the docs deleted, among them accepted ones; the named docs stay
        live0, live1 = rng.random(n0) > 0.05, rng.random(n1) > 0.05
        keep0 = np.concatenate([[0, 63, 64, n0 - 1, 77], tie0])
        keep1 = np.concatenate([[0, 63, 64, n1 - 1], tie1])
        live0[keep0] = True
        live1[keep1] = True
        acc0 = np.setdiff1d(np.flatnonzero(m0), keep0)
        acc1 = np.setdiff1d(np.flatnonzero(m1 & (np.arange(n1) % 3 == 0)), keep1)
        live0[acc0[:3]] = False
        live1[acc1[:5]] = False                          # accepted docs WITH a row that liveDocs delete
        m5_0, m5_1 = np.arange(n0) % 20 == 0, np.arange(n1) % 60 == 0
        mh_0, mh_1 = np.arange(n0) % 200 == 0, np.arange(n1) % 600 == 0
        none = lambda n: np.zeros(n, dtype=bool)         # noqa: E731
        m3 = none(500)
        m3[rng.choice(500, size=20, replace=False)] = True
        self.leaves = [
            Leaf(0, n0, rows0, None, live0, {M_MAIN: m0, M_5PCT: m5_0, M_HALF_PCT: mh_0, M_NOTHING: none(n0)}),
            Leaf(n0, n1, rows1, o2d1, live1, {M_MAIN: m1, M_5PCT: m5_1, M_HALF_PCT: mh_1, M_NOTHING: none(n1)}),
            Leaf(n0 + n1, 1, gen_rows(rng, kind, 1, dim), None, None,
                 {M_MAIN: np.ones(1, dtype=bool), M_5PCT: np.ones(1, dtype=bool), M_HALF_PCT: none(1), M_NOTHING: none(1)}),
            Leaf(n0 + n1 + 1, 500, None, None, None, {M_MAIN: m3, M_5PCT: m3, M_HALF_PCT: m3, M_NOTHING: none(500)}),
            Leaf(n0 + n1 + 501, 300, gen_rows(rng, kind, 300, dim), None, None, {m: none(300) for m in (M_MAIN, M_5PCT, M_HALF_PCT, M_NOTHING)}),
        ]
        self.all_rows = sum(len(lf.rows) for lf in self.leaves if lf.rows is not None)
        self.handles = []
        for lf in self.leaves:
            g = api.GpuSegment(ctx, lf.max_doc, lf.base)
            if lf.rows is None:
                g.add_vectors(F + 1, np.ones((lf.max_doc, 16), dtype=f32))    # another field: this leaf lacks F
            elif kind == "float":
                g.add_vectors(F, lf.rows, lf.o2d)
            else:
                g.add_byte_vectors(F, lf.rows, lf.o2d)
            g.seal()
            if lf.live is not None:
                g.set_live_docs(pack_bits(lf.live))
            for mid, flags in lf.masks.items():
                g.set_mask(mid, pack_bits(flags))
            self.handles.append(g)
        self.searcher = api.GpuIndexSearcher(ctx, self.handles, api.IndexStatistics())
        self._accepted = {}

    def accepted(self, mask_id):
        """(global docids int64[n], rows[n, dim]) of the accepted, live docs that have a vector, in doc order."""
        if mask_id not in self._accepted:
            docs, rows = [], []
            for lf in self.leaves:
                if lf.rows is None:
                    continue
                local = (lf.o2d if lf.o2d is not None else np.arange(len(lf.rows))).astype(np.int64)
                ok = lf.masks[mask_id][local]
                if lf.live is not None:
                    ok = ok & lf.live[local]
                docs.append(lf.base + local[ok])
                rows.append(lf.rows[ok])
            self._accepted[mask_id] = (np.concatenate(docs), np.ascontiguousarray(np.concatenate(rows)))
        return self._accepted[mask_id]

    def release(self):
        for g in self.handles:
            g.release()


def unboosted_scores(oracle, kind, sim, dim, Q, V):
    """float32[n_q, n_rows], every pair by the reference function itself: the oracle's vector_score / nrtgpu_byte_vector_score."""
    out = np.zeros((len(Q), len(V)), dtype=f32)
    if kind == "float":
        Q = np.ascontiguousarray(Q, dtype=f32)
        if sim == "normalized_cosine":       # unit-normalised query + dot product (the api does the same before the call)
            Q = np.ascontiguousarray(Q / np.linalg.norm(Q, axis=1, keepdims=True).astype(f32), dtype=f32)
        sid = api.GpuIndexSearcher.SIMILARITY[sim]
        for qi in range(len(Q)):
            for r in range(len(V)):
                out[qi, r] = oracle.vector_score(sid, Q[qi], V[r])
        return out
    L = _lib.load()
    sid = api.GpuIndexSearcher.BYTE_SIMILARITY[sim]
    Qd, Vd = Q.astype(np.int64), V.astype(np.int64)
    dot, nq, nv = Qd @ Vd.T, (Qd * Qd).sum(1), (Vd * Vd).sum(1)
    one = C.c_float()
    for qi in range(len(Q)):
        for r in range(len(V)):
            assert L.nrtgpu_byte_vector_score(sid, dim, int(dot[qi, r]), int(nq[qi]), int(nv[r]), C.byref(one)) == 0
            out[qi, r] = one.value
    return out


def top_k(scores, docs, k, boost=1.0, min_score=0.0):
    """The knn request's semantics: min_score on the unboosted score, the k best by (score desc, doc asc), the boost afterwards."""
    if min_score > 0:
        keep = scores >= f32(min_score)
        scores, docs = scores[keep], docs[keep]
    order = np.lexsort((docs, -scores.astype(f64)))[:k]
    s, d = scores[order], docs[order]
    if boost != 1.0:
        s = (s * f32(boost)).astype(f32)
        order = np.lexsort((d, -s.astype(f64)))     # distinct scores can round to one product: (score desc, doc asc) among equals
        s, d = s[order], d[order]
    return s, d


def search(index, sim, Q, k, mask_id, boost=1.0, min_score=0.0):
    sr = index.searcher
    fn = sr.knn_search if index.kind == "float" else sr.knn_search_bytes
    return fn(F, sim, Q, k, boost, api.MaskFilter(mask_id), min_score)


def with_stats(ctx, fn):
    before = ctx.stats()
    got = fn()
    after = ctx.stats()
    return got, {c: after[c] - before[c] for c in COUNTERS}


def assert_full_pass(d, all_rows):
    assert d["knn_panels"] >= 1 and d["knn_rows"] >= all_rows * d["knn_panels"] and d["knn_rows"] % all_rows == 0, d


def assert_gather(d, n_queries, n_accepted):
    panels = (n_queries + 63) // 64
    assert d == {"knn_panels": panels, "knn_score_launches": panels, "knn_rows": panels * n_accepted, "knn_sketch_launches": 0,
                 "knn_second_passes": 0}, d


def same(a, s, d):
    assert a.docs.tolist() == d.tolist()
    assert a.scores.view(np.uint32).tolist() == s.view(np.uint32).tolist()
    assert a.total_hits == len(d) and not a.relation_gte


def three_ways(ctx, oracle, index, sim, Q, ks, mask_id=M_MAIN, boost=1.0, min_score=0.0, expect_gather=True):
    """knob 0, knob 1000 and the reference for every k of `ks`; the reference scores are computed once."""
    docs, rows = index.accepted(mask_id)
    ref = unboosted_scores(oracle, index.kind, sim, index.dim, Q, rows)
    for k in ks:
        try:
            ctx.set_knn_gather(0)
            full, d0 = with_stats(ctx, lambda: search(index, sim, Q, k, mask_id, boost, min_score))
            ctx.set_knn_gather(1000)
            gath, d1 = with_stats(ctx, lambda: search(index, sim, Q, k, mask_id, boost, min_score))
        finally:
            ctx.set_knn_gather(0)
        assert_full_pass(d0, index.all_rows)
        if expect_gather:
            assert_gather(d1, len(Q), len(docs))
        else:
            assert_full_pass(d1, index.all_rows)
        assert len(full) == len(gath) == len(Q)
        for qi in range(len(Q)):
            s, d = top_k(ref[qi], docs, k, boost, min_score)
            same(gath[qi], s, d)
            same(full[qi], s, d)
    return ref, docs


def queries_of(rng, kind, n, dim):
    return gen_rows(rng, kind, n, dim)


@pytest.fixture(scope="module")
def float16(ctx):
    ix = Index(ctx, "float", 16)
    yield ix
    ix.release()


@pytest.fixture(scope="module")
def byte64(ctx):
    ix = Index(ctx, "byte", 64)
    yield ix
    ix.release()


def test_the_setter_checks_its_argument(ctx):
    for bad in (-1, 1001):
        with pytest.raises(api.NrtGpuError) as e:
            ctx.set_knn_gather(bad)
        assert e.value.code == _lib.NRTGPU_ERR_INVALID_ARG
    ctx.set_knn_gather(1000)
    ctx.set_knn_gather(0)


@pytest.mark.parametrize("dim", [3, 16, 100, 768, 2048])
def test_float_fields_at_every_dimension_and_similarity(ctx, oracle, float16, dim):
    ix = float16 if dim == 16 else Index(ctx, "float", dim)
    try:
        Q = queries_of(np.random.default_rng(dim), "float", 17, dim)
        for sim in FLOAT_SIMS:
            three_ways(ctx, oracle, ix, sim, Q, [10])
    finally:
        if ix is not float16:
            ix.release()


@pytest.mark.parametrize("dim", [3, 64, 65, 513, 2048])
def test_byte_fields_at_every_dimension_and_similarity(ctx, oracle, byte64, dim):
    ix = byte64 if dim == 64 else Index(ctx, "byte", dim)
    try:
        Q = queries_of(np.random.default_rng(dim), "byte", 17, dim)
        for sim in BYTE_SIMS:
            three_ways(ctx, oracle, ix, sim, Q, [10])
    finally:
        if ix is not byte64:
            ix.release()


@pytest.mark.parametrize("n_queries", [1, 17, 64, 65, 130])
@pytest.mark.parametrize("kind", ["float", "byte"])
def test_query_counts_and_k(ctx, oracle, float16, byte64, kind, n_queries):
    """1 .. 130 queries: the second and third pass of 64 and the last partial panel; k = 1, 10, 1024 -- the last one larger than
    the accepted rows, so every accepted row comes back."""
    ix = float16 if kind == "float" else byte64
    Q = queries_of(np.random.default_rng(n_queries), kind, n_queries, ix.dim)
    assert len(ix.accepted(M_MAIN)[0]) < 1024
    three_ways(ctx, oracle, ix, "l2_norm" if kind == "float" else "dot_product", Q, [1, 10, 1024])


@pytest.mark.parametrize("kind", ["float", "byte"])
def test_the_named_filter_bits_and_the_docs_that_must_not_come_back(ctx, oracle, float16, byte64, kind):
    ix = float16 if kind == "float" else byte64
    docs, _ = ix.accepted(M_MAIN)
    n0, n1 = ix.leaves[0].max_doc, ix.leaves[1].max_doc
    have = set(docs.tolist())
    assert {0, 63, 64, n0 - 1, n0 + 0, n0 + 63, ix.leaves[2].base} <= have      # docs 0, 63, 64, max_doc - 1; the one-doc leaf
    assert n0 + 64 not in have and n0 + n1 - 1 not in have                      # accepted, but no vector
    m0, l0 = ix.leaves[0].masks[M_MAIN], ix.leaves[0].live
    assert (m0 & ~l0).sum() >= 3                                                # accepted, but deleted
    assert not any(ix.leaves[3].base <= d < ix.leaves[3].base + 500 for d in have)   # the leaf without the field
    Q = queries_of(np.random.default_rng(2), kind, 3, ix.dim)
    three_ways(ctx, oracle, ix, "cosine", Q, [1024])
    ctx.set_knn_gather(1000)
    try:
        got = search(ix, "cosine", Q, 1024, M_MAIN)
    finally:
        ctx.set_knn_gather(0)
    for t in got:
        assert sorted(t.docs.tolist()) == sorted(have)


@pytest.mark.parametrize("kind", ["float", "byte"])
def test_eight_docs_with_one_row_come_out_in_doc_order(ctx, oracle, float16, byte64, kind):
    ix = float16 if kind == "float" else byte64
    Q = np.stack([ix.tie_row, ix.tie_row])
    three_ways(ctx, oracle, ix, "l2_norm", Q, [8, 10])
    ctx.set_knn_gather(1000)
    try:
        got = search(ix, "l2_norm", Q, 8, M_MAIN)
    finally:
        ctx.set_knn_gather(0)
    for t in got:
        assert t.docs.tolist() == ix.tie_docs and len(set(t.scores.view(np.uint32).tolist())) == 1


def test_a_byte_zero_row_scores_zero_under_cosine(ctx, oracle, byte64):
    Q = queries_of(np.random.default_rng(4), "byte", 2, 64)
    three_ways(ctx, oracle, byte64, "cosine", Q, [1024])
    ctx.set_knn_gather(1000)
    try:
        got = search(byte64, "cosine", Q, 1024, M_MAIN)
    finally:
        ctx.set_knn_gather(0)
    for t in got:
        at = t.docs.tolist().index(byte64.zero_doc)
        assert t.scores.view(np.uint32)[at] == 0


@pytest.mark.parametrize("kind", ["float", "byte"])
def test_min_score_cuts_on_the_unboosted_score(ctx, oracle, float16, byte64, kind):
    ix = float16 if kind == "float" else byte64
    Q = queries_of(np.random.default_rng(6), kind, 5, ix.dim)
    docs, rows = ix.accepted(M_MAIN)
    ref = unboosted_scores(oracle, kind, "cosine", ix.dim, Q, rows)
    cut = float(np.median(ref[0]))
    assert 0 < cut and 0 < (ref[0] >= f32(cut)).sum() < len(docs)
    assert (ref[0] * f32(2.5) >= f32(cut)).sum() > (ref[0] >= f32(cut)).sum()      # a cut on the boosted score would keep more
    three_ways(ctx, oracle, ix, "cosine", Q, [10, 1024], boost=2.5, min_score=cut)


@pytest.mark.parametrize("kind", ["float", "byte"])
def test_the_knob_is_a_share_of_the_rows(ctx, oracle, float16, byte64, kind):
    """Knob 10 (1 %): a filter accepting 5 % of the rows takes the full pass, one accepting 0.5 % the gather route."""
    ix = float16 if kind == "float" else byte64
    Q = queries_of(np.random.default_rng(8), kind, 3, ix.dim)
    sim = "dot_product"
    for mask_id, gathers in ((M_5PCT, False), (M_HALF_PCT, True)):
        docs, rows = ix.accepted(mask_id)
        share = len(docs) / ix.all_rows
        assert (0.04 < share < 0.06) if not gathers else (0.003 < share < 0.006)
        ref = unboosted_scores(oracle, kind, sim, ix.dim, Q, rows)
        ctx.set_knn_gather(10)
        try:
            got, d = with_stats(ctx, lambda: search(ix, sim, Q, 10, mask_id))
        finally:
            ctx.set_knn_gather(0)
        if gathers:
            assert_gather(d, len(Q), len(docs))
        else:
            assert_full_pass(d, ix.all_rows)
        for qi in range(len(Q)):
            same(got[qi], *top_k(ref[qi], docs, 10))


@pytest.mark.parametrize("kind", ["float", "byte"])
def test_a_filter_that_accepts_nothing_launches_nothing(ctx, float16, byte64, kind):
    ix = float16 if kind == "float" else byte64
    Q = queries_of(np.random.default_rng(9), kind, 70, ix.dim)
    ctx.set_knn_gather(1000)
    try:
        got, d = with_stats(ctx, lambda: search(ix, "l2_norm", Q, 10, M_NOTHING))
    finally:
        ctx.set_knn_gather(0)
    assert d == {c: 0 for c in COUNTERS}
    assert len(got) == 70 and all(len(t.docs) == 0 and len(t.scores) == 0 and t.total_hits == 0 and not t.relation_gte for t in got)
    full = search(ix, "l2_norm", Q, 10, M_NOTHING)
    assert all(len(t.docs) == 0 and t.total_hits == 0 for t in full)


@pytest.mark.parametrize("kind", ["float", "byte"])
def test_a_fork_with_further_deletes_next_to_its_parent(ctx, oracle, kind):
    rng = np.random.default_rng(12)
    dim, n = (16, 4097) if kind == "float" else (64, 4097)
    rows = gen_rows(rng, kind, n, dim)
    mask = rng.random(n) < 0.05
    live_parent = rng.random(n) > 0.1
    live_fork = live_parent & (rng.random(n) > 0.3)        # a reader version's deletes only accumulate
    assert (mask & live_parent & ~live_fork).sum() > 10
    g = api.GpuSegment(ctx, n, 0)
    (g.add_vectors if kind == "float" else g.add_byte_vectors)(F, rows)
    g.seal()
    g.set_live_docs(pack_bits(live_parent))
    g.set_mask(M_MAIN, pack_bits(mask))
    fork = g.fork(pack_bits(live_fork))
    fork.set_mask(M_MAIN, pack_bits(mask))
    Q = queries_of(rng, kind, 3, dim)
    try:
        for handle, live in ((g, live_parent), (fork, live_fork), (g, live_parent)):
            ok = mask & live
            docs, V = np.flatnonzero(ok).astype(np.int64), np.ascontiguousarray(rows[ok])
            ref = unboosted_scores(oracle, kind, "l2_norm", dim, Q, V)
            sr = api.GpuIndexSearcher(ctx, [handle], api.IndexStatistics())
            fn = sr.knn_search if kind == "float" else sr.knn_search_bytes
            for knob in (0, 1000):
                ctx.set_knn_gather(knob)
                got, d = with_stats(ctx, lambda: fn(F, "l2_norm", Q, 50, 1.0, api.MaskFilter(M_MAIN), 0.0))
                if knob:
                    assert_gather(d, len(Q), len(docs))
                else:
                    assert_full_pass(d, n)
                for qi in range(len(Q)):
                    same(got[qi], *top_k(ref[qi], docs, 50))
    finally:
        ctx.set_knn_gather(0)
        fork.release()
        g.release()


@pytest.mark.parametrize("kind", ["float", "byte"])
def test_more_accepted_rows_than_a_candidate_list_holds_take_the_full_pass(ctx, oracle, kind):
    rng = np.random.default_rng(14)
    dim, n = 3, KNN_CAP + 8000
    rows = gen_rows(rng, kind, n, dim)
    mask = np.ones(n, dtype=bool)
    mask[rng.choice(n, size=5000, replace=False)] = False           # the estimate: n - 5 000 > the list's capacity
    assert mask.sum() > KNN_CAP
    g = api.GpuSegment(ctx, n, 0)
    (g.add_vectors if kind == "float" else g.add_byte_vectors)(F, rows)
    g.seal()
    g.set_mask(M_MAIN, pack_bits(mask))
    sr = api.GpuIndexSearcher(ctx, [g], api.IndexStatistics())
    fn = sr.knn_search if kind == "float" else sr.knn_search_bytes
    Q = queries_of(rng, kind, 1, dim)
    docs, V = np.flatnonzero(mask).astype(np.int64), np.ascontiguousarray(rows[mask])
    ref = unboosted_scores(oracle, kind, "l2_norm", dim, Q, V)
    try:
        for knob in (0, 1000):
            ctx.set_knn_gather(knob)
            got, d = with_stats(ctx, lambda: fn(F, "l2_norm", Q, 10, 1.0, api.MaskFilter(M_MAIN), 0.0))
            assert_full_pass(d, n)
            same(got[0], *top_k(ref[0], docs, 10))
    finally:
        ctx.set_knn_gather(0)
        g.release()


@pytest.mark.parametrize("kind", ["float", "byte"])
def test_an_expired_deadline_times_out_on_the_gather_route(ctx, float16, byte64, kind):
    ix = float16 if kind == "float" else byte64
    Q = queries_of(np.random.default_rng(15), kind, 2, ix.dim)
    ctx.set_knn_gather(1000)
    try:
        api.GpuContext.set_thread_deadline(-1.0)
        with pytest.raises(api.NrtGpuError) as e:
            search(ix, "l2_norm", Q, 10, M_MAIN)
        assert e.value.code == _lib.NRTGPU_ERR_TIMEOUT
    finally:
        api.GpuContext.set_thread_deadline(None)
        ctx.set_knn_gather(0)
    got = search(ix, "l2_norm", Q, 10, M_MAIN)      # the thread and the context are as before
    assert len(got) == 2 and len(got[0].docs) == 10
