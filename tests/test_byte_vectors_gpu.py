"""Exact search over byte (int8) vector fields on the GPU (knn_bytes.hip) against a brute force in numpy.

The truth: dot = Q.astype(float64) @ V.astype(float64).T (BLAS, and exact: every partial sum is an integer far below 2^53), the
norms likewise, cast to int64; scores by include/nrtgpu.h's table with float32 scalars, one rounding per operation; * float32(boost);
sorted by (-score, doc).  Compared with == on docids and on score BITS: the matrix cores return the integers exactly, so no
tolerance exists anywhere in this file."""
import numpy as np
import pytest

from nrtsearch_amd import api

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
SIMS = ["cosine", "dot_product", "l2_norm", "max_inner_product"]
F = 3


@pytest.fixture(scope="module")
def ctx():
    c = api.GpuContext(device_id=0, max_batch=64)
    yield c
    c.close()


def unboosted(sim, dim, Q, V):
    """float32[n_q, n_rows]: the table, vectorised (numpy's float32 array operations round once each)."""
    Qd, Vd = Q.astype(f64), V.astype(f64)
    dot = (Qd @ Vd.T).astype(np.int64)
    nq = (Qd * Qd).sum(1).astype(np.int64)[:, None]
    nv = (Vd * Vd).sum(1).astype(np.int64)[None, :]
    if sim == "cosine":
        with np.errstate(divide="ignore", invalid="ignore"):
            c = (dot.astype(f64) / np.sqrt(nq.astype(f64) * nv.astype(f64))).astype(f32)
        s = (f32(1.0) + c) / f32(2.0)
        return np.where((nq == 0) | (nv == 0), f32(0.0), s).astype(f32)
    if sim == "dot_product":
        return (f32(0.5) + dot.astype(f32) / f32(dim * 32768)).astype(f32)
    if sim == "l2_norm":
        return (f32(1.0) / (f32(1.0) + (nq + nv - 2 * dot).astype(f32))).astype(f32)
    x = dot.astype(f32)
    with np.errstate(divide="ignore"):
        return np.where(x < 0, f32(1.0) / (f32(1.0) + f32(-1.0) * x), x + f32(1.0)).astype(f32)


def best(scores, docs, k):
    """The k best of one query's (score, doc) pairs by (score desc, doc asc)."""
    if len(scores) > 4 * k:
        thr = np.partition(scores, len(scores) - k)[len(scores) - k]
        keep = scores >= thr
        scores, docs = scores[keep], docs[keep]
    order = np.lexsort((docs, -scores.astype(f64)))[:k]
    return scores[order], docs[order]


def brute(sim, dim, Q, segs, k, boost=1.0, knn=False, min_score=0.0, masks=None, chunk=100_000):
    """[(scores, docs, matching)] per query.  segs: (base, rows, ord_to_doc, live, max_doc); masks: per segment bool[max_doc]."""
    per_q = [([], []) for _ in range(len(Q))]
    for si, (base, rows, o2d, live, max_doc) in enumerate(segs):
        for r0 in range(0, len(rows), chunk):
            V = rows[r0: r0 + chunk]
            local = (o2d[r0: r0 + chunk] if o2d is not None else np.arange(r0, r0 + len(V))).astype(np.int64)
            ok = np.ones(len(V), dtype=bool)
            if live is not None:
                ok &= live[local]
            if masks is not None:
                ok &= masks[si][local]
            s = unboosted(sim, dim, Q, V[ok])
            d = (base + local[ok]).astype(np.int64)
            for qi in range(len(Q)):
                sq, dq = s[qi], d
                if knn and min_score > 0:
                    keep = sq >= f32(min_score)
                    sq, dq = sq[keep], dq[keep]
                sq = (sq * f32(boost)).astype(f32)
                n = len(sq)
                bs, bd = best(sq, dq, k)
                per_q[qi][0].append((bs, bd, n))
    out = []
    for qi in range(len(Q)):
        parts = per_q[qi][0]
        s = np.concatenate([p[0] for p in parts]) if parts else np.zeros(0, f32)
        d = np.concatenate([p[1] for p in parts]) if parts else np.zeros(0, np.int64)
        bs, bd = best(s, d, k)
        out.append((bs, bd, sum(p[2] for p in parts)))
    return out


def check(got, exp, knn=False):
    """Bit for bit: docs in order, score bits, and the hit total (exact search: live docs with a vector; knn: the hits returned)."""
    s, d, n = exp
    assert got.docs.tolist() == d.tolist()
    assert got.scores.view(np.uint32).tolist() == s.view(np.uint32).tolist()
    assert got.total_hits == (len(d) if knn else n) and not got.relation_gte


def pack_bits(flags, max_doc):
    padded = np.zeros(((max_doc + 63) // 64) * 64, dtype=bool)
    padded[:max_doc] = flags
    return np.packbits(padded.reshape(-1, 64), axis=1, bitorder="little").view(np.uint64).reshape(-1)


def make_segments(rng, n_list, dim, sparse_ords=False, deletes=False, rows_of=None):
    segs, base = [], 0
    for si, n in enumerate(n_list):
        rows = rows_of(si, n) if rows_of else rng.integers(-128, 128, size=(n, dim), dtype=np.int8)
        max_doc = n if not (sparse_ords and si == 1) else 2 * n
        o2d = np.sort(rng.choice(max_doc, size=n, replace=False)).astype(np.int32) if (sparse_ords and si == 1) else None
        live = (rng.random(max_doc) > 0.1) if (deletes and si == 0) else None
        segs.append((base, rows, o2d, live, max_doc))
        base += max_doc
    return segs


def upload(ctx, segs):
    leaves = []
    for base, rows, o2d, live, max_doc in segs:
        g = api.GpuSegment(ctx, max_doc, base)
        g.add_byte_vectors(F, rows, o2d)
        g.seal()
        if live is not None:
            g.set_live_docs(pack_bits(live, max_doc))
        leaves.append(g)
    return leaves


def release(leaves):
    for g in leaves:
        g.release()


@pytest.mark.parametrize("sim", SIMS)
def test_exact_search_matches_bruteforce(ctx, sim):
    rng = np.random.default_rng(12345678)
    dim = 64
    segs = make_segments(rng, [3000, 1500, 700], dim, sparse_ords=True, deletes=True)
    leaves = upload(ctx, segs)
    sr = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics())
    Q = rng.integers(-128, 128, size=(5, dim), dtype=np.int8)
    live_vectors = int(segs[0][3][:3000].sum()) + 1500 + 700
    for k in (1, 10, 100):
        got = sr.knn_exact_bytes(F, sim, Q, k, boost=1.5)
        exp = brute(sim, dim, Q, segs, k, boost=1.5)
        for qi in range(len(Q)):
            check(got[qi], exp[qi])
            assert got[qi].total_hits == live_vectors
    release(leaves)


@pytest.mark.parametrize("sim", SIMS)
@pytest.mark.parametrize("dim", [3, 100, 768, 2048])
def test_dimensions_that_exercise_the_padding_and_the_range(ctx, sim, dim):
    rng = np.random.default_rng(dim)
    segs = make_segments(rng, [2500, 900], dim)
    leaves = upload(ctx, segs)
    sr = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics())
    Q = rng.integers(-128, 128, size=(4, dim), dtype=np.int8)
    if dim == 3:
        Q[0] = [-50, 5, 100]          # the reference's own query (VectorFieldDefTest.java:2028)
    for k in (10, 200):
        got = sr.knn_exact_bytes(F, sim, Q, k)
        exp = brute(sim, dim, Q, segs, k)
        for qi in range(len(Q)):
            check(got[qi], exp[qi])
    release(leaves)


@pytest.mark.parametrize("n_queries", [4, 64])
@pytest.mark.parametrize("dim,steps,depth", [(64, 1, 1), (100, 2, 2), (192, 3, 3), (256, 4, 4), (320, 5, 5), (384, 6, 6), (448, 7, 7),
                                             (512, 8, 8), (576, 10, 5), (832, 14, 7), (1100, 18, 6), (1400, 24, 8), (1700, 28, 7), (2048, 32, 8)])
def test_every_ring_depth_at_either_panel_width(ctx, dim, steps, depth, n_queries):
    """knn_bytes_kernel<P, D> is compiled once per panel width P (1: <= 16 queries, 4: more) and ring depth D (1 .. 8, a divisor of
    the resident steps): every one of the 16 instantiations is run here, the padded step counts (9 -> 10, 13 -> 14, 18, 22 -> 24,
    27 -> 28) among them, and 2048 dimensions with 64 queries -- the launch that takes the CU's whole LDS.  Two leaves, deletes,
    all four similarities."""
    rng = np.random.default_rng(1000 * dim + n_queries)
    segs = make_segments(rng, [2600, 1300], dim, sparse_ords=True, deletes=True)
    leaves = upload(ctx, segs)
    sr = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics())
    Q = rng.integers(-128, 128, size=(n_queries, dim), dtype=np.int8)
    for sim in SIMS:
        got = sr.knn_exact_bytes(F, sim, Q, 150, boost=1.5)
        exp = brute(sim, dim, Q, segs, 150, boost=1.5)
        for qi in range(n_queries):
            check(got[qi], exp[qi])
    release(leaves)


@pytest.mark.parametrize("sim", SIMS)
def test_the_largest_integers(ctx, sim):
    """Rows and queries of -128 / 127 only at 2048 dimensions: |dot| and the norms up to 2^25, squared distances to 2^27."""
    rng = np.random.default_rng(99)
    dim = 2048
    ext = np.array([-128, 127], dtype=np.int8)

    def rows_of(si, n):
        rows = ext[rng.integers(0, 2, size=(n, dim))]
        rows[0], rows[1] = -128, 127
        return rows
    segs = make_segments(rng, [1200, 500], dim, rows_of=rows_of)
    leaves = upload(ctx, segs)
    sr = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics())
    Q = ext[rng.integers(0, 2, size=(4, dim))]
    Q[0], Q[1] = -128, 127
    got = sr.knn_exact_bytes(F, sim, Q, 300)
    exp = brute(sim, dim, Q, segs, 300)
    for qi in range(len(Q)):
        check(got[qi], exp[qi])
    release(leaves)


def test_the_operand_map(ctx):
    """Data asymmetric in row, query and element, every (query, row) score in the answer: a transposed read of the result, swapped
    operands or a k-order that differs between the resident rows and the panel in LDS changes it."""
    dim, n, nq = 192, 1000, 64
    r, i, j = np.arange(n)[:, None], np.arange(dim)[None, :], np.arange(nq)[:, None]
    rows = (((r * 31 + i * 7) % 255) - 127).astype(np.int8)
    Q = (((j * 13 + i * i) % 251) - 125).astype(np.int8)
    segs = [(0, rows, None, None, n)]
    leaves = upload(ctx, segs)
    sr = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics())
    got = sr.knn_exact_bytes(F, "max_inner_product", Q, 1000)
    exp = brute("max_inner_product", dim, Q, segs, 1000)
    for qi in range(nq):
        assert len(got[qi].docs) == 1000
        check(got[qi], exp[qi])
    release(leaves)


@pytest.mark.parametrize("distinct", [1, 4])
def test_ties_come_out_in_docid_order(ctx, distinct):
    rng = np.random.default_rng(4)
    dim = 64
    protos = rng.integers(-128, 128, size=(distinct, dim), dtype=np.int8)

    def rows_of(si, n):
        return protos[rng.integers(0, distinct, size=n)]
    segs = make_segments(rng, [2500, 1500, 1000], dim, sparse_ords=True, rows_of=rows_of)     # 5 000 rows across three leaves
    leaves = upload(ctx, segs)
    sr = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics())
    Q = rng.integers(-128, 128, size=(3, dim), dtype=np.int8)
    for sim in ("cosine", "l2_norm"):
        for k in (1, 16, 1024):
            got = sr.knn_exact_bytes(F, sim, Q, k)
            exp = brute(sim, dim, Q, segs, k)
            for qi in range(len(Q)):
                check(got[qi], exp[qi])
                s, d = got[qi].scores, got[qi].docs
                assert all(d[i] < d[i + 1] for i in range(len(d) - 1) if s[i] == s[i + 1])
    release(leaves)


def test_panels_and_passes(ctx):
    """1 .. 130 queries against one corpus: each query's answer is its answer when searched alone."""
    rng = np.random.default_rng(8)
    dim, n = 128, 20_000
    segs = make_segments(rng, [n], dim)
    leaves = upload(ctx, segs)
    sr = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics())
    Q = rng.integers(-128, 128, size=(130, dim), dtype=np.int8)
    alone = [sr.knn_exact_bytes(F, "cosine", Q[qi: qi + 1], 50)[0] for qi in range(130)]
    exp = brute("cosine", dim, Q, segs, 50)
    for qi in range(130):
        check(alone[qi], exp[qi])
    for nq in (1, 16, 17, 64, 65, 130):
        got = sr.knn_exact_bytes(F, "cosine", Q[:nq], 50)
        assert len(got) == nq
        for qi in range(nq):
            assert got[qi].docs.tolist() == alone[qi].docs.tolist()
            assert got[qi].scores.view(np.uint32).tolist() == alone[qi].scores.view(np.uint32).tolist()
    release(leaves)


@pytest.mark.parametrize("sim", SIMS)
def test_the_knn_request_path(ctx, sim):
    """Filter mask (10 % of the docs) + deletes + min_score at the median unboosted score + boost 2."""
    rng = np.random.default_rng(31)
    dim = 64
    segs = make_segments(rng, [3000, 1500, 700], dim, sparse_ords=True, deletes=True)
    leaves = upload(ctx, segs)
    masks = []
    for leaf, (base, rows, o2d, live, max_doc) in zip(leaves, segs):
        m = rng.random(max_doc) < 0.1
        masks.append(m)
        leaf.set_mask(4, pack_bits(m, max_doc))
        leaf.set_mask(5, pack_bits(np.zeros(max_doc, dtype=bool), max_doc))
    sr = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics())
    Q = rng.integers(-128, 128, size=(5, dim), dtype=np.int8)
    for qi in range(len(Q)):
        everything = brute(sim, dim, Q[qi: qi + 1], segs, 10**6, masks=masks)[0]
        median = float(np.median(everything[0]))
        for k in (10, 100):
            got = sr.knn_search_bytes(F, sim, Q[qi: qi + 1], k, boost=2.0, filter=api.MaskFilter(4), min_score=median)[0]
            exp = brute(sim, dim, Q[qi: qi + 1], segs, k, boost=2.0, knn=True, min_score=median, masks=masks)[0]
            assert 0 < len(exp[1]) <= k
            check(got, exp, knn=True)
            assert got.total_hits == len(got.docs)
        got = sr.knn_search_bytes(F, sim, Q[qi: qi + 1], 500, filter=api.MaskFilter(4))[0]      # no threshold: fewer than k match the filter
        check(got, brute(sim, dim, Q[qi: qi + 1], segs, 500, knn=True, masks=masks)[0], knn=True)
    none = sr.knn_search_bytes(F, sim, Q, 10, filter=api.MaskFilter(5))     # a filter that accepts nothing
    assert all(len(t.docs) == 0 and t.total_hits == 0 for t in none)
    release(leaves)


def test_one_size_where_the_stream_matters(ctx):
    """2 M x 768 (1.5 GB): 64 queries, cosine, k = 100, against the brute force in row chunks; one pass, no second pass."""
    rng = np.random.default_rng(2_000_000)
    dim, n, chunk = 768, 2_000_000, 100_000
    rows = np.empty((n, dim), dtype=np.int8)
    for r0 in range(0, n, chunk):
        rows[r0: r0 + chunk] = rng.integers(-128, 128, size=(chunk, dim), dtype=np.int8)
    segs = [(0, rows, None, None, n)]
    leaves = upload(ctx, segs)
    sr = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics())
    Q = rng.integers(-128, 128, size=(64, dim), dtype=np.int8)
    before = ctx.stats()
    got = sr.knn_exact_bytes(F, "cosine", Q, 100)
    after = ctx.stats()
    assert after["knn_second_passes"] == before["knn_second_passes"]
    assert after["knn_panels"] == before["knn_panels"] + 1 and after["knn_rows"] == before["knn_rows"] + n
    exp = brute("cosine", dim, Q, segs, 100, chunk=chunk)
    for qi in range(64):
        check(got[qi], exp[qi])
    release(leaves)


def test_a_fork_answers_by_its_own_live_docs(ctx):
    rng = np.random.default_rng(12)
    dim, n = 64, 4000
    rows = rng.integers(-128, 128, size=(n, dim), dtype=np.int8)
    live_parent = rng.random(n) > 0.1
    live_fork = live_parent & (rng.random(n) > 0.3)        # a reader version's deletes only accumulate
    g = api.GpuSegment(ctx, n, 0)
    g.add_byte_vectors(F, rows)
    g.seal()
    g.set_live_docs(pack_bits(live_parent, n))
    parent_bytes = g.device_bytes
    assert parent_bytes >= n * dim
    fork = g.fork(pack_bits(live_fork, n))
    assert g.device_bytes == parent_bytes and fork.device_bytes < n * dim      # the rows are shared, not copied
    Q = rng.integers(-128, 128, size=(3, dim), dtype=np.int8)
    for handle, live in ((g, live_parent), (fork, live_fork), (g, live_parent)):
        sr = api.GpuIndexSearcher(ctx, [handle], api.IndexStatistics())
        got = sr.knn_exact_bytes(F, "l2_norm", Q, 50)
        exp = brute("l2_norm", dim, Q, [(0, rows, None, live, n)], 50)
        for qi in range(len(Q)):
            check(got[qi], exp[qi])
            assert got[qi].total_hits == int(live.sum())
    fork.release()
    g.release()


@pytest.mark.parametrize("sim", ["l2_norm", "max_inner_product"])
def test_the_byte_search_agrees_with_the_float_search(ctx, sim):
    """At 64 dimensions every partial sum of the float path is an integer below 2^24: the path the oracle certifies returns the same
    docids and score bits for the same values as fp32."""
    rng = np.random.default_rng(64)
    dim = 64
    segs = make_segments(rng, [3000, 1500], dim, sparse_ords=True, deletes=True)
    leaves = upload(ctx, segs)
    fleaves = []
    for base, rows, o2d, live, max_doc in segs:
        g = api.GpuSegment(ctx, max_doc, base)
        g.add_vectors(F, rows.astype(np.float32), o2d)
        g.seal()
        if live is not None:
            g.set_live_docs(pack_bits(live, max_doc))
        fleaves.append(g)
    Q = rng.integers(-128, 128, size=(6, dim), dtype=np.int8)
    a = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics()).knn_exact_bytes(F, sim, Q, 100, boost=1.5)
    b = api.GpuIndexSearcher(ctx, fleaves, api.IndexStatistics()).knn_exact(F, sim, Q.astype(np.float32), 100, boost=1.5)
    for x, y in zip(a, b):
        assert x.docs.tolist() == y.docs.tolist()
        assert x.scores.view(np.uint32).tolist() == y.scores.view(np.uint32).tolist()
        assert x.total_hits == y.total_hits
    release(leaves + fleaves)
