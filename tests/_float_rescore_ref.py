"""A restatement of the FLOAT vector rescorer (QueryRescore over an exact float vector query) in numpy float64, with a DERIVED
interval for what an fp32 kernel may return, the cases tests/test_float_rescore_gpu.py runs, and a float32 simulation of the
kernels' order of summation for tests/test_float_rescore_ref_host.py.  Imports nothing from the library and takes no number from
the device: rows, queries and the doc -> leaf -> row tables are the host's own.

The score.  second = map(sum) * boost, combined = (float)(qw * first + rw * second) in double; a doc without a vector keeps
(float)(qw * first).  map: cosine max((1 + c) / 2, 0) with c = (float)(q.v / sqrt(|q|^2 |v|^2)); dot_product max((1 + q.v) / 2, 0);
l2_norm 1 / (1 + |q - v|^2); max_inner_product 1 / (1 - q.v) below 0, q.v + 1 else.

The interval.  u = 2^-24, gamma(m) = m u / (1 - m u) (Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1: a
product of m factors (1 + d_i), |d_i| <= u, is 1 + t with |t| <= gamma(m)).  The kernels sum with one wave per row: lane l adds
the elements l, l + 64, ... of the RESIDENT row (the field's dimension rounded up to a multiple of 16, zero padded), then six
butterfly additions.  An element's term therefore passes at most ceil(dim_resident / 64) lane additions, 6 butterfly additions and
one rounding of its product (none when the compiler fuses multiply and add), so with m = ceil(dim_resident / 64) + 7:
  * dot-type sums lie in D +- gamma(m) sum|q_k v_k|, D the exact sum;
  * the squared distance sums (q_k - v_k)^2, whose difference is rounded once more and enters squared: S (1 +- gamma(m + 2));
  * cosine: |v|^2 is summed in the same wave order when the rows are uploaded, V (1 +- gamma(m)); |q|^2 is summed on the host
    left to right, every product rounded: Q (1 +- gamma(dim_resident + 1)).  c is cast to float once: its range is widened by
    2u |c| (that rounding, and the double division and square root before it).
The corners of these ranges go through the (monotone) map in float64.  What is left are single fp32 operations: 1 + x, one
division, the multiplication by the boost -- at most 3, a division taken as 2.5 ulp: the second-pass range is widened by 6u
relative; the combine is exact in double up to 2^-52 and cast once: 2u relative.  Both terms of the combine are >= 0, so the two
together stay within 8u relative of the result.  A doc without a vector has no range: (float)(qw * first), one IEEE operation.
`terms` replaces m for a summation in another order (a scalar left-to-right sum: dim_resident + 1)."""
import collections

import numpy as np

f32, f64 = np.float32, np.float64
U = 2.0 ** -24
SIMS = {"cosine": 0, "dot_product": 1, "l2_norm": 2, "max_inner_product": 3}
DIMS = [3, 64, 100, 200, 260, 768, 2048]   # resident: 16, 64, 112, 208, 272, 768, 2048
MARKS = (0, 63, 64, 191, 192, 255, 256)    # the ends of the lanes' first strides and of the four-element unrolled step
FEW = np.array([[3, 0.5, -3], [-3, 1, 3], [3, -2, 3], [-3, 0.25, -3]], dtype=f32)   # dimension 3: the only rows there are
# rows of a field by the similarity that reads it: "zeros" has a zero row every 97 (cosine and dot_product refuse them in Lucene,
# the oracle answers NaN); "unit": rows and queries of length 1 (dot_product clamps at q.v < -1: unnormalised sums would all score 0)
KIND_OF_SIM = {"cosine": "plain", "dot_product": "unit", "l2_norm": "zeros", "max_inner_product": "zeros"}
KINDS = ["plain", "zeros", "unit"]
TERM_SETS = [[1, 20, 300], [3, 8, 60, 2000], [2000], [1, 3, 8, 20, 60], [300, 2000], [777777]]   # the last: a term without postings
# (recall, window, queryWeight, rescoreWeight, boost) by dimension.  window < n: 3, 64, 260, 768; window == recall: 200, 2048;
# window > n: 100; recall = NRTGPU_MAX_K: 200; boost != 1: 100, 200, 768, 2048.  queryWeight = 0 at 3 (ties) and at 768 and 2048:
# l2_norm's score there is below 1e-3 and one element moves it by 1e-3 of that, less than the rounding of a combined score next
# to a first-pass score of a few units -- with queryWeight > 0 no tolerance could tell a dropped element there.
SHAPES = {3: (1000, 300, 0.0, 1.0, 1.0), 64: (64, 10, 1.0, 1.0, 1.0), 100: (200, 300, 0.5, 4.0, 2.0), 200: (1024, 1024, 1.0, 2.5, 0.37),
          260: (300, 100, 0.25, 3.0, 1.0), 768: (1000, 100, 0.0, 2.5, 0.37), 2048: (300, 300, 0.0, 3.0, 2.0)}


def resident(dim):
    return (dim + 15) & ~15


def gamma(m):
    return m * U / (1.0 - m * U)


def wave_terms(dim):
    return -(-resident(dim) // 64) + 7


def marker_positions(dim):
    return sorted({p for p in MARKS + (dim - 1,) if 0 <= p < dim})


def make_rows(rng, n, dim, kind):
    """float32[n, dim]: standard normal, +-3 at the marker positions; dimension 3: drawn from FEW."""
    if dim == 3:
        v = FEW[rng.integers(0, len(FEW), size=n)].copy()
    else:
        v = rng.standard_normal((n, dim), dtype=f32)
        pos = marker_positions(dim)
        v[:, pos] = 3.0 * rng.choice(np.array([-1.0, 1.0], dtype=f32), size=(n, len(pos)))
    if kind == "zeros":
        v[::97] = 0
    if kind == "unit":
        v = (v.astype(f64) / np.linalg.norm(v.astype(f64), axis=1, keepdims=True)).astype(f32)
    return np.ascontiguousarray(v)


def make_queries(rng, n, dim, kind):
    """float32[n, dim]: standard normal, +-1.5 at the marker positions (a marker pair adds 4.5 to a dot product in magnitude and
    at least 2.25 to a squared distance)."""
    q = rng.standard_normal((n, dim), dtype=f32)
    pos = marker_positions(dim)
    q[:, pos] = 1.5 * rng.choice(np.array([-1.0, 1.0], dtype=f32), size=(n, len(pos)))
    if kind == "unit":
        q = (q.astype(f64) / np.linalg.norm(q.astype(f64), axis=1, keepdims=True)).astype(f32)
    return np.ascontiguousarray(q)


class Table:
    """One field's rows by leaf: leaves[i] = (float32[n_vec, dim], ord_to_doc or None) or None; doc -> leaf -> row or none."""
    HAS, NO_FIELD, GAP, BEHIND = 0, 1, 2, 3

    def __init__(self, dim, bases, max_docs, leaves):
        self.dim, self.bases, self.max_docs, self.leaves = dim, list(bases), list(max_docs), leaves

    def lookup(self, docs):
        """-> (why: int[n] -- HAS or the reason there is no vector, rows: float32[n, dim], zeros where there is none)."""
        why = np.zeros(len(docs), dtype=np.int64)
        rows = np.zeros((len(docs), self.dim), dtype=f32)
        for i, doc in enumerate(docs):
            si = max(j for j, b in enumerate(self.bases) if b <= doc)
            local = int(doc) - self.bases[si]
            assert 0 <= local < self.max_docs[si]
            if self.leaves[si] is None:
                why[i] = self.NO_FIELD
                continue
            v, o2d = self.leaves[si]
            if o2d is None:
                if local >= len(v):
                    why[i] = self.BEHIND
                    continue
                r = local
            else:
                r = int(np.searchsorted(o2d, local))
                if r >= len(o2d) or o2d[r] != local:
                    why[i] = self.GAP
                    continue
            rows[i] = v[r]
        return why, rows


def second_pass(sim, q, rows, boost, dim, terms=None):
    """The second-pass score of every row in float64 and its range: (ref, lo, hi), float64[n].  q: float32[dim], rows: float32[n, dim]."""
    m = wave_terms(dim) if terms is None else terms
    q64, v64 = q.astype(f64), rows.astype(f64)
    if sim == 2:
        s = ((q64[None, :] - v64) ** 2).sum(axis=1)
        g = gamma(m + 2)
        ref, lo, hi = 1.0 / (1.0 + s), 1.0 / (1.0 + s * (1.0 + g)), 1.0 / (1.0 + s * (1.0 - g))
    else:
        d = v64 @ q64
        e = gamma(m) * (np.abs(v64) @ np.abs(q64))
        if sim == 0:
            qq, vv = q64 @ q64, (v64 * v64).sum(axis=1)
            assert qq > 0 and (vv > 0).all(), "a zero vector under cosine"
            gq, gv = gamma(resident(dim) + 1), gamma(m)
            den_lo, den_hi = np.sqrt(qq * (1 - gq) * vv * (1 - gv)), np.sqrt(qq * (1 + gq) * vv * (1 + gv))
            corners = np.stack([(d - e) / den_lo, (d - e) / den_hi, (d + e) / den_lo, (d + e) / den_hi])
            c_lo, c_hi = corners.min(axis=0), corners.max(axis=0)
            c_lo, c_hi = c_lo - 2 * U * np.abs(c_lo), c_hi + 2 * U * np.abs(c_hi)
            fn = lambda c: np.maximum((1.0 + c) / 2.0, 0.0)   # noqa: E731
            ref, lo, hi = fn(d / np.sqrt(qq * vv)), fn(c_lo), fn(c_hi)
        else:
            if sim == 1:
                fn = lambda x: np.maximum((1.0 + x) / 2.0, 0.0)   # noqa: E731
            else:
                fn = lambda x: np.where(x < 0, 1.0 / (1.0 - np.minimum(x, 0.0)), x + 1.0)   # noqa: E731
            ref, lo, hi = fn(d), fn(d - e), fn(d + e)
    b = float(f32(boost))
    return ref * b, lo * b * (1 - 6 * U), hi * b * (1 + 6 * U)


def combined(qw, rw, first, has, second):
    """QueryRescore.combine over every hit: (ref, lo, hi), float64[n].  first: float32[n]; has: bool[n]; second: second_pass's
    triple over all n rows (ignored where has is False)."""
    base = float(qw) * first.astype(f64)
    alone = f32(base).astype(f64)
    out = []
    for s, w in zip(second, (0.0, -2 * U, 2 * U)):
        out.append(np.where(has, (base + float(rw) * s) * (1 + w), alone))
    return tuple(out)


def check_answer(first_docs, ref, lo, hi, got_docs, got_scores, window, where=""):
    """(a) - (d) of the issue over one answer; returns max |got - ref| / half-width over the returned hits that have a range.
    A doc that the first pass lists twice may be returned twice: each return takes one of its entries, best first."""
    n = len(first_docs)
    got_docs, got_scores = [int(d) for d in got_docs], np.asarray(got_scores, dtype=f32)
    assert len(got_docs) == min(window, n), (where, "(a) length", len(got_docs), window, n)
    bits = got_scores.view(np.uint32).tolist()
    keys = [(-b, d) for b, d in zip(bits, got_docs)]
    assert keys == sorted(keys), (where, "(c) not sorted by (score bits descending, doc ascending)")
    by_doc = collections.defaultdict(list)
    for i, d in enumerate(first_docs):
        by_doc[int(d)].append(i)
    for d in by_doc:
        by_doc[d].sort(key=lambda i: -hi[i])
    worst = 0.0
    for d, s in zip(got_docs, got_scores.astype(f64).tolist()):
        assert by_doc.get(d), (where, "(a) not a first-pass doc, or returned more often than listed", d)
        i = by_doc[d].pop(0)
        assert lo[i] <= s <= hi[i], (where, "(b) score outside its range", d, s, lo[i], ref[i], hi[i])
        if hi[i] > lo[i]:
            worst = max(worst, abs(s - ref[i]) / ((hi[i] - lo[i]) / 2))
    if got_docs:
        last = float(got_scores[-1])
        for d, left in by_doc.items():
            for i in left:
                assert lo[i] <= last, (where, "(d) a doc left out scores above the last one returned", d, lo[i], last)
                # (a hit without a vector has one possible score: on an exact tie with the last one returned the docid decides)
                assert not (lo[i] == hi[i] == last and d < got_docs[-1]), (where, "(d) a tie left out although its docid is lower", d)
    else:
        assert n == 0
    return worst


# ---- the kernels' order of summation in float32, for the host tests of the interval ----------------------------------------
def _pad(a, width):
    out = np.zeros(a.shape[:-1] + (width,), dtype=f32)
    out[..., : a.shape[-1]] = a
    return out


def wave_sum(sim, q, rows, fused, skip=None):
    """One wave per row: lane l adds the elements l, l + 64, ..., then the xor butterfly; lane 0's value, float32[n].
    fused: acc = fma(x, y, acc) (the exact product added in double, rounded once to float) instead of two roundings.
    skip: an element the loop leaves out (a simulated mistake)."""
    width = -(-q.shape[0] // 64) * 64
    qp, vp = _pad(q, width), _pad(rows, width)
    if skip is not None:
        qp[skip] = 0
        vp[:, skip] = 0
    acc = np.zeros((rows.shape[0], 64), dtype=f32)
    for k in range(0, width, 64):
        x, y = vp[:, k:k + 64], qp[None, k:k + 64]
        if sim == 2:
            x = y - x
            y = x
        if fused:
            acc = (acc.astype(f64) + x.astype(f64) * y.astype(f64)).astype(f32)
        else:
            acc = acc + x * y
        assert acc.dtype == f32
    lanes = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ d]
    return acc[:, 0]


def host_query_norm(q):
    s = f32(0)
    for x in q:
        s = f32(s + f32(x * x))
    return s


def kernel_score(sim, acc, nq, nv, boost, qw, rw, first):
    """The kernels' float32 steps behind the sum: the map, the boost, the combine in double."""
    one, two = f32(1), f32(2)
    if sim == 0:
        c = (acc.astype(f64) / np.sqrt(f64(nq) * nv.astype(f64))).astype(f32)
        s = np.maximum((one + c) / two, f32(0))
    elif sim == 1:
        s = np.maximum((one + acc) / two, f32(0))
    elif sim == 2:
        s = one / (one + acc)
    else:
        s = np.where(acc < 0, one / (one - np.minimum(acc, f32(0))), acc + one)
    s = (s * f32(boost)).astype(f32)
    assert s.dtype == f32
    return (float(qw) * first.astype(f64) + float(rw) * s.astype(f64)).astype(f32)
