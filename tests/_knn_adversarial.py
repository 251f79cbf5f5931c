"""Worst-case data for the exact float vector search's certification (vectors.cpp: knn_impl; host_math.h: knn_bound32 / knn_bound16;
plan.h: knn_result_upper / knn_estimate_lower), with a numpy emulation that PROVES it is worst-case.  No test in here:
tests/test_knn_adversarial_host.py holds the conditions against this module on the CPU, tests/test_knn_adversarial_gpu.py runs
the same cases through the library.

The search nominates rows from an ESTIMATE of the score (the fp16 sketch on the matrix cores), rescores the k + max(32, k / 2)
nominations in the oracle's order and certifies the answer with a bound E on |estimate - result|.  A case here is a (query,
winners, decoys) triple:
  * the k winners truly outscore every decoy under the oracle's fp32 left-to-right sum,
  * the sketch ranks every decoy above every winner, so all nominations are decoys,
  * the estimate's error on both groups is as close to E as data can make it.
A search whose E is too small, or that applies it wrongly, then certifies the decoys (or never finds the winners in the second
pass) and returns a wrong answer.

The lever is fp16's half-way values.  A = fp32(1 + 2^-11 - 2^-20) rounds DOWN to 1 after the sketch's power-of-two scaling: 2^-11
of the value is lost, in the rows and in the query alike, so a product of two such values loses 2^-10 -- the bound's leading term.
1 + j * 2^-10 is exact in fp16.  Winners carry ONE exact element with a bump of (m - 1) * 2^-10, decoys m exact elements with
2^-10 each: the estimate prefers the decoys by 2^-10, the truth the winners by about (m - 3) * 2^-11.

What "need" is: the smallest E for which the certification still refuses -- the k-th best nominated row's RESULT minus the last
nomination's ESTIMATE (for l2_norm: the other way round, in squared-distance units).  need / E is how much of the bound the case
uses up; the measured ratios are recorded in _TABLE below (from the emulation here, never from a device), and a bound cut in half
falls below need."""
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
A = np.float32(1.0 + 2.0 ** -11 - 2.0 ** -20)     # rounds down to 1 in fp16 after any power-of-two scaling
SIMS = {"cosine": 0, "dot_product": 1, "l2_norm": 2, "max_inner_product": 3}

Case = namedtuple("Case", "name sim_name dim k query winners decoys filler boost ratio")


def exact(j):
    """1 + j * 2^-10: exact in fp16."""
    return np.float32(1.0 + j * 2.0 ** -10)


def k_int_of(k):
    return min(1024, k + max(32, k // 2))


def resident_dim(dim):
    return (dim + 15) & ~15


# ---- the oracle's arithmetic, restated (nrt_oracle_vector_score: scalar, left to right, every op rounded to fp32) -------------
def seq_sums(sim, q, rows):
    """(dot or squared distance, |v|^2) per row, in the oracle's order."""
    q, rows = np.asarray(q, np.float32), np.asarray(rows, np.float32)
    acc, nv = np.zeros(len(rows), np.float32), np.zeros(len(rows), np.float32)
    for i in range(q.shape[0]):
        if sim == 2:
            d = (q[i] - rows[:, i]).astype(np.float32)
            acc = (acc + (d * d).astype(np.float32)).astype(np.float32)
        else:
            acc = (acc + (q[i] * rows[:, i]).astype(np.float32)).astype(np.float32)
            nv = (nv + (rows[:, i] * rows[:, i]).astype(np.float32)).astype(np.float32)
    return acc, nv


def seq_norm2(q):
    acc = np.float32(0)
    for x in np.asarray(q, np.float32):
        acc = np.float32(acc + np.float32(x * x))
    return acc


def score_of(sim, dot, nq, nv):
    """The oracle's map from the sums to a score (fp32 operations; cosine through double, as Lucene)."""
    one, two = np.float32(1), np.float32(2)
    dot = np.asarray(dot, np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        if sim == 0:
            c = (dot.astype(np.float64) / np.sqrt(np.float64(nq) * np.asarray(nv, np.float32).astype(np.float64))).astype(np.float32)
            s = ((one + c) / two).astype(np.float32)
            return np.where(s > 0, s, np.float32(0)).astype(np.float32)
        if sim == 1:
            s = ((one + dot) / two).astype(np.float32)
            return np.where(s > 0, s, np.float32(0)).astype(np.float32)
        if sim == 2:
            return (one / (one + dot)).astype(np.float32)
        return np.where(dot < 0, one / (one - dot), dot + one).astype(np.float32)


def results(sim, q, rows, boost=1.0):
    """What the search must return for each row: the oracle's score times the boost, in fp32."""
    acc, nv = seq_sums(sim, q, rows)
    return (score_of(sim, acc, seq_norm2(q), nv) * np.float32(boost)).astype(np.float32)


# ---- the sketch's arithmetic, emulated (knn.hip: knn_sketch_build_kernel, knn_panel_fp16_kernel, knn_sketch_kernel) -----------
def pow2_scale(absmax):
    """host_math.h: knn_sketch_scale."""
    if not absmax > 0:
        return 1.0
    _, e = np.frexp(np.float32(absmax))     # absmax < 2^e
    return float(np.ldexp(1.0, 14 - int(e)))


def sketch_dots(q, rows, rows_scale):
    """fp16 operands, exact products, fp32 accumulation, scaled back by the two powers of two (exact).  rows_scale: one scale, or
    one per row (rows of leaves with different scales)."""
    sq = pow2_scale(np.abs(q).max())
    sv = np.broadcast_to(np.asarray(rows_scale, np.float64), (len(rows),)).astype(np.float32)
    r16 = (rows * sv[:, None]).astype(np.float32).astype(np.float16).astype(np.float32)
    q16 = (q * np.float32(sq)).astype(np.float32).astype(np.float16).astype(np.float32)
    acc = (r16 * q16[None, :]).sum(axis=1, dtype=np.float32)
    return ((acc * np.float32(1.0 / sq)).astype(np.float32) * (np.float32(1) / sv)).astype(np.float32)


def estimates(sim, q, rows, rows_scale, boost=1.0):
    """(estimated score, estimated squared distance) per row, the way knn_sketch_kernel maps its dot products (fp32; the
    hardware's rsq / rcp are within an ulp of these, which the bound's 32 u covers).  |v|^2: the build's wave-order sum, here
    float64 rounded once (closer to the real value than any fp32 order: the fp32 part of the bound covers the difference)."""
    dot = sketch_dots(q, rows, rows_scale)
    one, half = np.float32(1), np.float32(0.5)
    nq = seq_norm2(q)
    nv = (rows.astype(np.float64) ** 2).sum(axis=1).astype(np.float32)
    d2 = np.maximum(((nq + nv).astype(np.float32) - (np.float32(2) * dot).astype(np.float32)).astype(np.float32), np.float32(0))
    with np.errstate(divide="ignore", invalid="ignore"):
        if sim == 0:
            c = ((dot * (one / np.sqrt(nq)).astype(np.float32)).astype(np.float32) * (one / np.sqrt(nv)).astype(np.float32)).astype(np.float32)
            est = np.maximum(((one + c) * half).astype(np.float32), np.float32(0))
        elif sim == 1:
            est = np.maximum(((one + dot) * half).astype(np.float32), np.float32(0))
        elif sim == 2:
            est = (one / (one + d2)).astype(np.float32)
        else:
            est = np.where(dot < 0, one / (one - dot), dot + one).astype(np.float32)
    return (est * np.float32(boost)).astype(np.float32), d2


# ---- the bound, restated from host_math.h (knn_bound32, knn_bound16) and plan.h -----------------------------------------------
E_REL = float(np.float32(32.0 * U))


def search_numbers(q, rows, rows_scales):
    """What knn_impl feeds the bounds: |q|^2 (fp32, in order), |q|_1, the query's unit, the rows' largest and smallest non-zero
    |v|^2, the largest 1 / scale of the leaves."""
    nv = (rows.astype(np.float64) ** 2).sum(axis=1).astype(np.float32)
    nz = nv[nv > 0]
    return dict(nq=float(seq_norm2(q)), q_l1=float(np.abs(q).astype(np.float64).sum()), q_absmax=float(np.abs(q).max()),
                q_unit=1.0 / pow2_scale(np.abs(q).max()), nv_max=float(nv.max()), nv_min=float(nz.min()) if len(nz) else float("inf"),
                rows_unit=max(1.0 / s for s in np.atleast_1d(rows_scales)))


def bound32(sim, dim, nq, nv_max, boost):
    gam = (dim + 4) * U
    e = {0: 2.0 * gam * boost, 1: 1.1 * gam * np.sqrt(nq * nv_max) * boost, 2: 4.5 * gam * (nq + nv_max),
         3: 2.2 * gam * np.sqrt(nq * nv_max) * boost}[sim]
    return float(np.nextafter(np.float32((e + 4.0 * U) * (1.0 + 1e-6)), np.float32(np.inf)))


def bound16(sim, dim, nq, q_l1, q_unit, nv_max, nv_min, rows_unit, boost):
    """dim: the resident dimension."""
    gam = (dim + 4) * U
    e16 = 2.0 ** -10 + 2.0 ** -22 + 4.0 * gam
    flush = q_l1 * 2.0 ** -14 * rows_unit + np.sqrt(dim * nv_max) * 2.0 ** -14 * q_unit
    e_dot = 1.01 * (e16 * np.sqrt(nq * nv_max) + flush)
    if sim == 0:
        e = 0.5 * 1.01 * (e16 + (flush / np.sqrt(nq * nv_min) if nq > 0 and np.isfinite(nv_min) else 0.0)) * boost
    elif sim == 1:
        e = 0.5 * e_dot * boost
    elif sim == 2:
        e = 2.0 * e_dot
    else:
        e = e_dot * boost
    e32 = bound32(sim, dim, nq, nv_max, boost)
    return float(np.nextafter(np.float32((e + e32 + 32.0 * U * (4.0 if sim == 2 else boost)) * (1.0 + 1e-6)), np.float32(np.inf)))


def result_upper(sim, m, e_abs, boost):
    if sim == 2:
        if not m > 0:
            return 0.0
        d2 = boost / m - 1.0
        lo = d2 - (e_abs + E_REL * (1.0 + d2))
        return boost / (1.0 + max(lo, 0.0)) * (1.0 + 1e-6)
    return (m + e_abs + E_REL * abs(m)) * (1.0 + 1e-6)


def estimate_lower(sim, s, e_abs, boost):
    if sim == 2:
        if not s > 0:
            return 0.0
        d2 = boost / s - 1.0
        return boost / (1.0 + max(d2, 0.0) + e_abs + E_REL * (1.0 + d2)) * (1.0 - 1e-6)
    return (s - (e_abs + E_REL * abs(s))) * (1.0 - 1e-6)


# ---- the constructions --------------------------------------------------------------------------------------------------------
def _spread(base, n, first, width, step):
    """n copies of `base`, copy i lowered by i * step in total, spread over `width` elements from `first` (each stays a value
    that rounds to 1 in fp16: the lowering per element is below 2^-11 + 2^-12)."""
    out = np.tile(base, (n, 1)).astype(np.float32)
    for i in range(n):
        for t in range(width):
            out[i, first + t] = np.float32(base[first + t] - np.float32(step * (i // width + (1 if t < i % width else 0))))
    assert step * ((n - 1) // width + 1) < 2.0 ** -11 + 2.0 ** -12 - 2.0 ** -19
    return out


def dot_triple(dim, k, n_decoys, m, width, step, used=None):
    """DOT_PRODUCT / MAXIMUM_INNER_PRODUCT (and the first `used` dimensions of the cosine cases).  q = A everywhere.  Winner i = A
    everywhere, element 0 = 1 + (m - 1) 2^-10, the `width` elements after it lowered by i * step in total.  Decoy j = A
    everywhere, elements 0 .. m-1 = 1 + 2^-10, element m = A - j 2^-22."""
    used = dim if used is None else used
    q = np.full(dim, A, np.float32)
    base = np.full(dim, A, np.float32)
    base[0] = exact(m - 1)
    winners = _spread(base, k, 1, width, step)
    decoys = np.tile(np.full(dim, A, np.float32), (n_decoys, 1))
    decoys[:, :m] = exact(1)
    decoys[:, m] = (A - np.arange(n_decoys) * 2.0 ** -22).astype(np.float32)
    assert 1 + width <= used and m + 1 <= used and float(decoys[:, m].min()) > 1.0 - 2.0 ** -12
    if used < dim:      # cosine: without these every cosine would collapse to 1 within an ulp
        q[used:] = 0.0
        winners[:, used:] = 1.0
        decoys[:, used:] = 1.0
    return q, winners, decoys


def l2_triple(dim, k, n_decoys, m, scale=32.0):
    """EUCLIDEAN, everything times S.  q = S A everywhere.  Winner i = q except the last element = S (A + (i + 1) 2^-13).  Decoy j =
    q except elements 0 .. m-1 = S (1 + 2^-10) and element m = S (A - (j + 1) 2^-15).  The estimated squared distances are all
    rounding (about 2 S^2 dim 2^-10); the true ones are below 0.002."""
    s = np.float32(scale)
    q = np.full(dim, s * A, np.float32)
    winners = np.tile(q, (k, 1))
    winners[:, -1] = (s * (A + (np.arange(k) + 1) * np.float32(2.0 ** -13))).astype(np.float32)
    decoys = np.tile(q, (n_decoys, 1))
    decoys[:, :m] = s * exact(1)
    decoys[:, m] = (s * (A - (np.arange(n_decoys) + 1) * np.float32(2.0 ** -15))).astype(np.float32)
    return q, winners, decoys


def filler_rows(dim, n, scale, seed):
    """Ordinary random rows, small next to the case's (they change neither the rows' largest |element| nor their largest norm):
    what the extra, ordinary query of the panel finds its answer among."""
    return (np.random.default_rng(seed).standard_normal((n, dim)) * 0.2 * scale).astype(np.float32)


def ordinary_query(dim, scale, seed):
    """A random query whose elements sum to something clearly negative: the case's near-identical rows then sit at the bottom of
    its ranking and its own answer (among the filler rows) certifies."""
    rng = np.random.default_rng(seed)
    while True:
        q = (rng.standard_normal(dim) * scale).astype(np.float32)
        if q.sum() < -0.5 * scale * np.sqrt(dim):
            return q


# name, similarity, dim, k, decoys, m, width, step -- and the need / E the emulation measures (measure() below; the host test
# asserts each at the recorded value - 0.02).  step: two fp32 ulps of the dot product, so the winners' results stay distinct.
_TABLE = [
    # name               sim                  dim    k  decoys   m  width  step        need / E
    ("dot_64",          "dot_product",         64,  10,    72,   4,     1, 2.0 ** -16,  0.933),
    ("dot_100",         "dot_product",        100,  10,    72,   4,     1, 2.0 ** -16,  0.928),
    ("dot_768",         "dot_product",        768,  10,    72,   8,     4, 2.0 ** -13,  0.762),
    ("mip_64",          "max_inner_product",   64,  10,    72,   4,     1, 2.0 ** -16,  0.933),
    ("mip_100",         "max_inner_product",  100,  10,    72,   4,     1, 2.0 ** -16,  0.928),
    ("mip_768",         "max_inner_product",  768,  10,    72,   8,     4, 2.0 ** -13,  0.762),
    ("l2_64",           "l2_norm",             64,  10,    72,   8,     0, 0.0,         0.888),
    ("l2_100",          "l2_norm",            100,  10,    72,   8,     0, 0.0,         0.891),
    ("l2_768",          "l2_norm",            768,  10,    72,  16,     0, 0.0,         0.699),
    ("cosine_64",       "cosine",              64,  10,    72,   8,     2, 2.0 ** -15,  0.589),
    ("cosine_100",      "cosine",             100,  10,    72,   8,     2, 2.0 ** -15,  0.606),
    ("cosine_768",      "cosine",             768,  10,    72,  32,     8, 2.0 ** -12,  0.486),
    ("dot_64_k1",       "dot_product",         64,   1,    40,   4,     1, 2.0 ** -16,  0.933),
    ("dot_64_k700",     "dot_product",         64, 700,  1724,  28,    24, 2.0 ** -16,  0.750),
]
N_FILLER = 40


def build(name, boost=1.0):
    row = next(r for r in _TABLE if r[0] == name)
    _, sim_name, dim, k, n_decoys, m, width, step, ratio = row
    if sim_name == "l2_norm":
        q, w, d = l2_triple(dim, k, n_decoys, m)
        fscale = 32.0
    else:
        q, w, d = dot_triple(dim, k, n_decoys, m, width, step, used=dim // 2 if sim_name == "cosine" else None)
        fscale = 1.0
    return Case(name, sim_name, dim, k, q, w, d, filler_rows(dim, N_FILLER, fscale, 100 + dim + k), float(boost), ratio)


CASE_NAMES = [r[0] for r in _TABLE]
K10_NAMES = CASE_NAMES[:12]


def layout(case, seed=7):
    """The case's rows in docid order -- winners, decoys and filler rows interleaved by a fixed permutation -- with what each row
    is (0 winner, 1 decoy, 2 filler) and its number within its group."""
    rows = np.concatenate([case.winners, case.decoys, case.filler]).astype(np.float32)
    kind = np.concatenate([np.zeros(len(case.winners), int), np.ones(len(case.decoys), int), np.full(len(case.filler), 2)])
    ident = np.concatenate([np.arange(len(case.winners)), np.arange(len(case.decoys)), np.arange(len(case.filler))])
    perm = np.random.default_rng(seed).permutation(len(rows))
    return np.ascontiguousarray(rows[perm]), kind[perm], ident[perm]


def panel(case):
    """The two queries of the case's panel: the adversarial one and an ordinary one."""
    return np.stack([case.query, ordinary_query(case.dim, 32.0 if case.sim_name == "l2_norm" else 1.0, 900 + case.dim)])


def two_leaf_extra(case):
    """The row that gives the winners' leaf a sketch scale 2^6 below the decoys': one large fp16-exact element, -1 elsewhere (far
    down every ranking)."""
    row = np.full((1, case.dim), -1.0, np.float32)
    row[0, 5] = 64.0
    return row, pow2_scale(64.0)


DEAD_DECOYS = (0, 1, 2, 30, 71)     # deleted in the "deleted decoys" case: the three the sketch likes best, one in the middle, the worst


def measure(case, extra_rows=None, extra_scale=None, e_of=None, dead_decoys=()):
    """Everything the host test asserts, from the emulation.  extra_rows / extra_scale: rows of ANOTHER leaf (their own sketch
    scale) that hold the winners' leaf-mates in the two-leaf case -- then the winners are scaled by extra_scale too.  e_of: a
    function (sim, resident dim, numbers, boost) -> E that replaces the restated bound (the library's, through its hook).
    dead_decoys: indices of deleted decoys."""
    sim, k, b = SIMS[case.sim_name], case.k, case.boost
    decoys = np.delete(case.decoys, list(dead_decoys), axis=0)
    groups = [case.winners, decoys, case.filler] + ([extra_rows] if extra_rows is not None else [])
    rows = np.concatenate(groups).astype(np.float32)
    main_scale = pow2_scale(np.abs(np.concatenate([decoys, case.filler])).max())
    w_scale = main_scale if extra_rows is None else extra_scale
    scales = np.concatenate([np.full(len(case.winners), w_scale), np.full(len(decoys) + len(case.filler), main_scale)]
                            + ([np.full(len(extra_rows), extra_scale)] if extra_rows is not None else []))
    res = results(sim, case.query, rows, b)
    est, d2_est = estimates(sim, case.query, rows, scales, b)
    nw, nd = len(case.winners), len(decoys)
    w_res, d_res, w_est, d_est = res[:nw], res[nw:nw + nd], est[:nw], est[nw:nw + nd]
    other_res, other_est = res[nw + nd:], est[nw + nd:]
    num = search_numbers(case.query, rows, sorted(set(scales.tolist())))
    rdim = resident_dim(case.dim)
    E = (e_of or (lambda s_, d_, n_, b_: bound16(s_, d_, n_["nq"], n_["q_l1"], n_["q_unit"], n_["nv_max"], n_["nv_min"], n_["rows_unit"], b_)))(sim, rdim, num, b)
    k_int = k_int_of(k)
    order = np.argsort(-d_est.astype(np.float64), kind="stable")[:k_int]       # the nominations: all decoys
    m_est = float(d_est[order[-1]])
    kth = float(np.sort(d_res[order])[::-1][k - 1])
    if sim == 2:
        d2_res, _ = seq_sums(2, case.query, rows)
        err = np.abs(d2_est.astype(np.float64) - d2_res.astype(np.float64))
        need = (b / m_est - 1.0) - (b / kth - 1.0)
        need2 = (b / float(w_est.min()) - 1.0) - (b / kth - 1.0)
    else:
        err = np.abs(est.astype(np.float64) - res.astype(np.float64))
        need = kth - m_est
        need2 = kth - float(w_est.min())
    gap_ulps = (float(w_res.min()) - float(d_res.max())) / float(np.spacing(np.float32(w_res.min())))
    return dict(sim=sim, E=E, numbers=num, rdim=rdim, need=need, need_second_pass=need2, ratio=need / E, max_err_ratio=float(err.max()) / E,
                gap_ulps=gap_ulps, winners_distinct=len(set(w_res.tolist())) == nw, w_res=w_res, d_res=d_res, w_est=w_est, d_est=d_est,
                other_res=other_res, other_est=other_est, k_int=k_int, kth=kth, m_est=m_est,
                certifies=kth > result_upper(sim, m_est, E, b),
                second_theta_keeps_winners=float(w_est.min()) >= estimate_lower(sim, kth, E, b))
