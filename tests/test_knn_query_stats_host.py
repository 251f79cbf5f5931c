"""The query statistics a pass of the exact float search stages (vectors.cpp: knn_query_stats -- |q|^2, the largest |element| and the
1-norm, eight queries side by side), without a device, through nrtgpu_debug_knn_query_stats of the development library.

|q|^2 must be bit-equal to the rescorers' chain (float_qnorm2: one query after the other, fp32, element order, every product
ROUNDED before it is added) -- the scores of the cosine similarity depend on it -- and the other two equal to numpy's.  The eight
chains side by side must not change any query's own order, whatever the position of the query in its group of eight (counts 1, 7,
8, 9, 17) and the dimension (1, 15, 16, 17, 100).

A compiler that fused x * x + s into one operation would give another sum.  The first test's values make that visible: elements
+-(1 + j / 4096) have 13 significant bits, so every product and every partial sum below 2^29 is exact in float64 and both chains
-- rounded and fused -- can be computed exactly with numpy.  For every dimension above 1 the two chains of the chosen values DIFFER
(asserted), and the library must return the rounded one.  At dimension 1 there is nothing to fuse into: 0 + x * x rounds once either
way, the two chains are equal for every x (asserted likewise)."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "nrtsearch_amd", "libnrtgpu.so")
DIMS, COUNTS = (1, 15, 16, 17, 100), (1, 7, 8, 9, 17)


@pytest.fixture(scope="module")
def stats():
    if not os.path.exists(LIB):
        pytest.skip("the library has not been built")
    from nrtsearch_amd import _lib, build
    build.build_dev()
    dev = _lib.load_dev()
    fn = dev.nrtgpu_debug_knn_query_stats
    fn.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    fn.restype = C.c_int32

    def call(q):
        q = np.ascontiguousarray(q, np.float32)
        nq, dim = q.shape
        n2, mx, ref = np.full(nq, -1, np.float32), np.full(nq, -1, np.float32), np.full(nq, -1, np.float32)
        l1 = np.full(nq, -1, np.float64)
        rc = fn(q.ctypes.data, nq, dim, n2.ctypes.data, mx.ctypes.data, l1.ctypes.data, ref.ctypes.data)
        assert rc == 0, dev.nrtgpu_last_error()
        return n2, mx, l1, ref
    return call


def chains(q):
    """(rounded, fused) |q|^2 per query in element order; exact for values whose products and sums float64 holds exactly."""
    rounded, fused = np.zeros(len(q), np.float32), np.zeros(len(q), np.float32)
    for d in range(q.shape[1]):
        x = q[:, d]
        rounded = rounded + x * x                                                          # fp32 product, fp32 sum: two roundings
        fused = (fused.astype(np.float64) + x.astype(np.float64) * x.astype(np.float64)).astype(np.float32)   # one rounding
    return rounded, fused


def short_mantissa_queries(nq, dim, seed):
    """+-(1 + j / 4096); the first seed from `seed` on whose values tell the two chains apart (any seed at dimension 1)."""
    while True:
        rng = np.random.default_rng(seed)
        q = ((1.0 + rng.integers(0, 4096, size=(nq, dim)) / 4096.0) * rng.choice([-1.0, 1.0], size=(nq, dim))).astype(np.float32)
        rounded, fused = chains(q)
        if dim == 1 or np.any(rounded != fused):
            return q
        seed += 1000


@pytest.mark.parametrize("nq", COUNTS)
@pytest.mark.parametrize("dim", DIMS)
def test_norm2_is_the_rounded_chain_where_a_fused_one_differs(stats, dim, nq):
    q = short_mantissa_queries(nq, dim, 100 * dim + nq)
    assert np.array_equal(q.astype(np.float64), 1.0 * q) and np.abs(q).max() < 2.0
    rounded, fused = chains(q)
    if dim == 1:
        assert np.array_equal(rounded, fused)     # (nothing to fuse into)
    else:
        assert np.any(rounded != fused), "the chosen values do not tell a fused chain from a rounded one"
    n2, mx, l1, ref = stats(q)
    assert n2.view(np.uint32).tolist() == ref.view(np.uint32).tolist()            # bit-equal to float_qnorm2
    assert n2.view(np.uint32).tolist() == rounded.view(np.uint32).tolist()        # which is the rounded chain
    assert mx.view(np.uint32).tolist() == np.abs(q).max(axis=1).view(np.uint32).tolist()
    assert l1.tolist() == np.abs(q.astype(np.float64)).sum(axis=1).tolist()       # (exact in float64: any order of summation)


@pytest.mark.parametrize("nq", COUNTS)
@pytest.mark.parametrize("dim", DIMS)
def test_the_three_statistics_of_ordinary_queries(stats, dim, nq):
    rng = np.random.default_rng(7 * dim + nq)
    q = (rng.standard_normal((nq, dim)) * np.exp2(rng.integers(-20, 20, size=(nq, 1)))).astype(np.float32)
    q[0, 0] = 0.0
    n2, mx, l1, ref = stats(q)
    assert n2.view(np.uint32).tolist() == ref.view(np.uint32).tolist()
    assert n2.view(np.uint32).tolist() == chains(q)[0].view(np.uint32).tolist()
    assert mx.view(np.uint32).tolist() == np.abs(q).max(axis=1).view(np.uint32).tolist()
    assert l1.tolist() == np.cumsum(np.abs(q.astype(np.float64)), axis=1)[:, -1].tolist()   # (cumsum: element order, as the search adds)
