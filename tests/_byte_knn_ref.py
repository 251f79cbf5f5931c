"""The truth for knn requests over byte (int8) vector fields, in numpy: the brute force of tests/test_byte_vectors_gpu.py restated
for requests that carry a filter, k, boost and threshold EACH (tests/test_knn_byte_requests_gpu.py).  Imports nothing from the
library's search paths and takes no number from the device.

The score: dot, |q|^2 and |v|^2 as exact integers (float64 products of int8 values summed far below 2^53, cast to int64), then
include/nrtgpu.h's table in float32 with one rounding per operation; a member's threshold tests the UNBOOSTED score; then
* float32(boost); the list sorted by (score desc, doc asc).  Every comparison made with these lists is == on docids and on score
BITS: the matrix cores return the integers exactly, so there is no tolerance anywhere."""
import numpy as np

f32, f64 = np.float32, np.float64
SIMS = {"cosine": 0, "dot_product": 1, "l2_norm": 2, "max_inner_product": 3}
# mask ids per leaf: 25 %, 1 %, one that accepts 7 rows in total, an empty one, a second 25 %; None = no filter
M25, M1, M7, M0, M25B = 3, 4, 5, 6, 7
KINDS = (M25, M1, M7, M0, M25B, None)


def words(bits):
    """bool[n] -> the uint64 words of a liveDocs / mask bit set."""
    padded = np.zeros(((len(bits) + 63) // 64) * 64, dtype=bool)
    padded[: len(bits)] = bits
    return np.packbits(padded.reshape(-1, 64), axis=1, bitorder="little").view(np.uint64).reshape(-1)


def unboosted(sim, dim, Q, V):
    """float32[n_q, n_rows]: the header's table, vectorised (numpy's float32 array operations round once each)."""
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
    assert sim == "max_inner_product", sim
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


class Leaf:
    """One leaf on the host: int8 rows (None: the leaf lacks the field), ord -> doc, liveDocs, masks (all over docs)."""

    def __init__(self, base, max_doc, rows, o2d=None, live=None):
        self.base, self.max_doc, self.rows, self.o2d, self.live = base, max_doc, rows, o2d, live
        self.masks = {}

    def accept_rows(self, mask_id):
        """liveDocs & mask, per ROW."""
        acc = np.ones(self.max_doc, bool) if self.live is None else self.live.copy()
        if mask_id is not None:
            acc &= self.masks[mask_id]
        return acc[: len(self.rows)] if self.o2d is None else acc[self.o2d]

    def docs(self):
        """The global docid of every row."""
        local = np.arange(len(self.rows), dtype=np.int64) if self.o2d is None else self.o2d.astype(np.int64)
        return self.base + local

    def upload(self, ctx, field, api):
        g = api.GpuSegment(ctx, self.max_doc, self.base)
        if self.rows is None:   # the leaf lacks the field (it holds another one)
            g.add_byte_vectors(field + 6, np.ones((4, 16), np.int8), np.arange(4, dtype=np.int32))
        else:
            g.add_byte_vectors(field, self.rows, self.o2d)
        g.seal()
        if self.live is not None:
            g.set_live_docs(words(self.live))
        for mid, m in self.masks.items():
            g.set_mask(mid, words(m))
        return g


def reference_lists(sim, queries, leaves, kinds, depth=100, chunk=100_000):
    """Per query its top `depth` (unboosted float32 score, global doc) under its OWN filter kind (a mask id, or None), the leaves'
    lists merged by (score desc, doc asc).  The scores of a chunk of rows are computed once for all the queries."""
    dim = queries.shape[1]
    parts = [([], []) for _ in range(len(queries))]
    for lf in leaves:
        if lf.rows is None:
            continue
        docs = lf.docs()
        accept = {kind: lf.accept_rows(kind) for kind in set(kinds)}
        for r0 in range(0, len(lf.rows), chunk):
            S = unboosted(sim, dim, queries, lf.rows[r0: r0 + chunk])
            d = docs[r0: r0 + chunk]
            for q, kind in enumerate(kinds):
                ok = accept[kind][r0: r0 + chunk]
                bs, bd = best(S[q][ok], d[ok], depth)
                parts[q][0].append(bs)
                parts[q][1].append(bd)
    out = []
    for s_parts, d_parts in parts:
        s = np.concatenate(s_parts) if s_parts else np.zeros(0, f32)
        d = np.concatenate(d_parts) if d_parts else np.zeros(0, np.int64)
        bs, bd = best(s, d, depth)
        out.append([(f32(x), int(y)) for x, y in zip(bs, bd)])
    return out


def expected(full, k, boost, min_score):
    """What a request gets: the rows at or above its threshold (unboosted), the first k, boosted, (score desc, doc asc)."""
    hits = [(f32(s) * f32(boost), d) for s, d in full if s >= f32(min_score)][:k]
    return sorted(hits, key=lambda t: (-float(t[0]), t[1]))


def threshold_of(full, kind):
    """0: none; 1: the reference's 60th score (a shorter list: its middle); 2: above the best score -- an empty answer."""
    if kind == 0:
        return 0.0
    if kind == 2:
        return float(full[0][0]) * 2.0 + 1.0 if full else 1.0
    if not full:
        return 0.5
    return float(full[60][0]) if len(full) > 60 else float(full[len(full) // 2][0])


def check_hits(got, exp, what):
    assert got.docs.tolist() == [d for _, d in exp], what
    assert got.scores.view(np.uint32).tolist() == np.array([s for s, _ in exp], dtype=f32).view(np.uint32).tolist(), what
    assert got.total_hits == len(got.docs) and not got.relation_gte, what


def mixed_index(dim):
    """4000 / 2500 / 900 int8 rows -- the second leaf with a sparse ord -> doc map, the first and the last with 10 % deletes -- and a
    leaf that lacks the field; the five masks on each; 70 int8 queries.  Below 64 dimensions the values are drawn from -6 .. 6 only:
    scores tie by the dozen there, so the order among ties and thresholds that fall on a tie are part of every comparison; the
    larger dimensions use the whole int8 range."""
    rng = np.random.default_rng(2000 + dim)
    lo, hi = (-6, 7) if dim < 64 else (-128, 128)
    leaves, base = [], 0
    for si, n in enumerate((4000, 2500, 0, 900)):
        if n == 0:
            lf = Leaf(base, 500, None)
        else:
            max_doc = 2 * n if si == 1 else n
            o2d = np.sort(rng.choice(max_doc, size=n, replace=False)).astype(np.int32) if si == 1 else None
            live = rng.random(max_doc) > 0.1 if si in (0, 3) else None
            lf = Leaf(base, max_doc, rng.integers(lo, hi, size=(n, dim), dtype=np.int8), o2d, live)
        lf.masks = {M25: rng.random(lf.max_doc) < 0.25, M1: rng.random(lf.max_doc) < 0.01, M7: np.zeros(lf.max_doc, bool),
                    M0: np.zeros(lf.max_doc, bool), M25B: rng.random(lf.max_doc) < 0.25}
        leaves.append(lf)
        base += lf.max_doc
    for lf, n7 in zip((leaves[0], leaves[1], leaves[3]), (3, 3, 1)):   # 7 accepted rows in total: live docs that have a vector
        docs = np.arange(lf.max_doc) if lf.o2d is None else lf.o2d
        ok = docs[lf.live[docs]] if lf.live is not None else docs
        lf.masks[M7][rng.choice(ok, size=n7, replace=False)] = True
    assert sum(int(lf.accept_rows(M7).sum()) for lf in leaves if lf.rows is not None) == 7
    queries = rng.integers(lo, hi, size=(70, dim), dtype=np.int8)
    return leaves, queries


def mixed_requests(n):
    """(kinds, ks, boosts, threshold kinds) of n requests: inside EACH 16-query panel of the first 64 every filter kind, every k of
    {1, 10, 37, 100}, every boost of {0.5, 1, 2} and every threshold kind appears."""
    kinds = [KINDS[(q + q // 16) % 6] for q in range(n)]
    ks = [(1, 10, 37, 100)[(q + q // 4) % 4] for q in range(n)]
    boosts = [(0.5, 1.0, 2.0)[(q // 5) % 3] for q in range(n)]
    thr_kinds = [(q // 2) % 3 for q in range(n)]
    for p0 in range(0, min(n, 64) - 15, 16):
        panel = range(p0, p0 + 16)
        assert {kinds[q] for q in panel} == set(KINDS) and {ks[q] for q in panel} == {1, 10, 37, 100}
        assert {boosts[q] for q in panel} == {0.5, 1.0, 2.0} and {thr_kinds[q] for q in panel} == {0, 1, 2}
    return kinds, ks, boosts, thr_kinds
