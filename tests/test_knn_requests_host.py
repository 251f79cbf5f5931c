"""The knn request entries without a device: the header / ctypes pairing of nrtgpu_knn_search_requests and
nrtgpu_knn_search_coalesced, and how a panel that was searched with the largest k of its members is unpacked into each member's own k
and boost (vectors.cpp: knn_unpack_topdocs, through nrtgpu_debug_knn_unpack of the development library)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "nrtsearch_amd", "libnrtgpu.so")
CTYPE_OF = {"nrtgpu_ctx*": C.c_void_p, "const nrtgpu_seg* const*": C.c_void_p, "const int32_t*": C.c_void_p, "const float*": C.c_void_p,
            "int32_t": C.c_int32, "float": C.c_float}


@pytest.fixture(scope="module")
def dev():
    if not os.path.exists(LIB):
        pytest.skip("the library has not been built")
    from nrtsearch_amd import _lib, build
    build.build_dev()
    return _lib.load_dev()


def test_the_two_entries_are_bound_as_the_header_declares_them():
    from nrtsearch_amd import _lib
    if not os.path.exists(LIB):
        pytest.skip("the library has not been built")
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nrtgpu.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in ("nrtgpu_knn_search_requests", "nrtgpu_knn_search_coalesced"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/nrtgpu.h"
        want = []
        for p in (" ".join(p.split()) for p in m.group(1).split(",")):
            ctype = p.rsplit(" ", 1)[0]   # the declaration without the parameter's name
            want.append(C.POINTER(_lib.TopDocs) if ctype == "nrtgpu_topdocs*" else CTYPE_OF[ctype])
        fn = getattr(lib, name)
        assert list(fn.argtypes) == want, name
        assert fn.restype in (C.c_int, C.c_int32)
    assert len(lib.nrtgpu_knn_search_requests.argtypes) == 14 and len(lib.nrtgpu_knn_search_coalesced.argtypes) == 13


def _unpack(dev, scores, docs, counts, k_pass, ks, boosts, capacity=None):
    from nrtsearch_amd import _lib
    nq, k_stride = scores.shape
    outs = (_lib.TopDocs * nq)()
    cap = capacity or k_stride
    od, os_ = np.full((nq, cap), -1, np.int32), np.full((nq, cap), -1.0, np.float32)
    for q in range(nq):
        outs[q].capacity = cap
        outs[q].docs = C.cast(od.ctypes.data + q * cap * 4, C.POINTER(C.c_int32))
        outs[q].scores = C.cast(os_.ctypes.data + q * cap * 4, C.POINTER(C.c_float))
    ks_a = None if ks is None else np.ascontiguousarray(ks, np.int32)
    b_a = None if boosts is None else np.ascontiguousarray(boosts, np.float32)
    cnt = np.ascontiguousarray(counts, np.uint32)
    rc = dev.nrtgpu_debug_knn_unpack(scores.ctypes.data, docs.ctypes.data, cnt.ctypes.data, k_stride, nq, k_pass,
                                     None if ks_a is None else ks_a.ctypes.data, None if b_a is None else b_a.ctypes.data, outs)
    assert rc == 0, dev.nrtgpu_last_error()
    return [(od[q, : outs[q].n_hits].tolist(), os_[q, : outs[q].n_hits].copy(), int(outs[q].total_hits), int(outs[q].total_hits_is_lower_bound))
            for q in range(nq)]


def test_a_member_takes_the_first_k_of_its_own_and_its_own_boost(dev):
    rng = np.random.default_rng(3)
    nq, k_pass, k_stride = 5, 37, 48
    scores = np.sort(rng.random((nq, k_stride)).astype(np.float32), axis=1)[:, ::-1].copy()
    docs = rng.permutation(nq * k_stride).astype(np.int32).reshape(nq, k_stride)
    counts = [37, 37, 12, 0, 37]          # what the panel found per member: the third fewer than its k, the fourth nothing
    ks = [1, 37, 20, 10, 10]
    boosts = [0.5, 1.0, 2.0, 3.0, 1.5]
    got = _unpack(dev, scores, docs, counts, k_pass, ks, boosts)
    for q in range(nq):
        m = min(counts[q], ks[q])
        d, s, total, lower = got[q]
        assert d == docs[q, :m].tolist(), q
        assert s.view(np.uint32).tolist() == (scores[q, :m] * np.float32(boosts[q])).view(np.uint32).tolist(), q   # one fp32 product
        assert total == m and lower == 0
    # the caller's capacity bounds a member as it bounds a single request; without arrays every member takes k_pass and boost 1
    got = _unpack(dev, scores, docs, counts, k_pass, [37] * nq, None, capacity=8)
    assert [len(g[0]) for g in got] == [8, 8, 8, 0, 8]
    got = _unpack(dev, scores, docs, counts, k_pass, None, None)
    for q in range(nq):
        assert got[q][0] == docs[q, : counts[q]].tolist() and got[q][1].view(np.uint32).tolist() == scores[q, : counts[q]].view(np.uint32).tolist()


def test_scores_that_round_to_one_product_are_ordered_by_docid(dev):
    """Distinct scores can round to one product under a boost: among equal boosted scores the lower docid comes first, as in a list
    sorted by (score desc, doc asc)."""
    a = np.float32(1.0)
    b = np.nextafter(a, np.float32(0.0))                      # a > b, one ulp apart
    boost = np.float32(1.0 / 3.0)
    assert a * boost == b * boost or np.nextafter(b, np.float32(0.0)) * boost == b * boost
    lo = b if a * boost == b * boost else np.nextafter(b, np.float32(0.0))
    hi = a if a * boost == b * boost else b
    scores = np.array([[hi, lo, np.float32(0.25), 0.0]], np.float32)
    docs = np.array([[9, 4, 1, 0]], np.int32)                  # sorted by (score desc, doc asc) BEFORE the boost
    (d, s, total, _), = _unpack(dev, scores, docs, [3], 3, [3], [float(boost)])
    assert s[0] == s[1] and d == [4, 9, 1] and total == 3
