"""Run by tests/test_byte_vectors_host.py in a subprocess with tests/mockhip preloaded (kernels do nothing): the HOST paths of byte
(int8) vector fields -- upload, seal, liveDocs, fork, searches, every refusal of include/nrtgpu.h with its status code, the
segments' device bytes.  One `name value` line per case on stdout."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from nrtsearch_amd import _lib, api   # noqa: E402

L = _lib.load()
rng = np.random.default_rng(5)
dim, F = 100, 3
ctx = api.GpuContext(device_id=0, max_batch=64)


def say(name, value):
    print(name, value, flush=True)


def rc_of(fn):
    try:
        fn()
        return 0
    except api.NrtGpuError as e:
        return e.code


def message_of(fn):
    try:
        fn()
        return "no error"
    except api.NrtGpuError as e:
        return str(e)


# two segments, the second with a sparse ord -> doc map
n0, n1 = 3000, 1000
g0 = api.GpuSegment(ctx, n0, 0)
before = g0.device_bytes
g0.add_byte_vectors(F, rng.integers(-128, 128, size=(n0, dim), dtype=np.int8))
say("bytes_grew_by_at_least_rows", g0.device_bytes - before >= n0 * dim)
g1 = api.GpuSegment(ctx, 2 * n1, n0)
g1.add_byte_vectors(F, rng.integers(-128, 128, size=(n1, dim), dtype=np.int8), np.sort(rng.choice(2 * n1, size=n1, replace=False)).astype(np.int32))
say("float_rows_into_byte_field", rc_of(lambda: g1.add_vectors(F, np.zeros((4, dim), dtype=np.float32))))
g1.add_vectors(F + 1, rng.standard_normal((n1, 16)).astype(np.float32))
say("byte_rows_into_float_field", rc_of(lambda: g1.add_byte_vectors(F + 1, np.zeros((4, 16), dtype=np.int8))))
gx = api.GpuSegment(ctx, 16, 0)
say("upload_dim_2049", rc_of(lambda: gx.add_byte_vectors(F, np.zeros((4, 2049), dtype=np.int8))))
gx.release()
g0.seal()
g1.seal()
live = np.full((n0 + 63) // 64, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
live[0] = 0xFFFFFFFFFFFF0000
g0.set_live_docs(live)
parent_bytes = g0.device_bytes
live2 = live.copy()
live2[1] = 0          # (a reader version's deletes only accumulate)
fork = g0.fork(live2)
say("fork_holds_no_second_copy", g0.device_bytes == parent_bytes and fork.device_bytes < n0 * dim)

sr = api.GpuIndexSearcher(ctx, [g0, g1], api.IndexStatistics())
srf = api.GpuIndexSearcher(ctx, [fork, g1], api.IndexStatistics())
q1 = rng.integers(-128, 128, size=(1, dim), dtype=np.int8)
q130 = rng.integers(-128, 128, size=(130, dim), dtype=np.int8)


def searched(s, q, k, **kw):
    got = s.knn_search_bytes(F, "l2_norm", q, k, **kw) if kw else s.knn_exact_bytes(F, "cosine", q, k)
    assert len(got) == len(q) and all(len(t.docs) == len(t.scores) <= k for t in got)
    return got


say("search_1", rc_of(lambda: searched(sr, q1, 10)))
say("search_130", rc_of(lambda: searched(sr, q130, 1024)))
say("search_knn_130", rc_of(lambda: searched(sr, q130, 100, boost=2.0, min_score=0.25)))
say("search_fork", rc_of(lambda: searched(srf, q130, 16)))
got = sr.knn_exact_bytes(F, "dot_product", q1, 5)
assert got[0].total_hits == n0 - 16 + n1, got[0].total_hits      # live docs that have a vector: host knowledge, no kernel needed
assert srf.knn_exact_bytes(F, "dot_product", q1, 5)[0].total_hits == n0 - 16 - 64 + n1
say("relation", int(sr.knn_exact_relation(F, 10, 1000)))           # 3984 live vectors in one slice > max(1000, 10)

# refusals
qf = rng.standard_normal((2, dim)).astype(np.float32)
say("float_search_over_byte_field", rc_of(lambda: sr.knn_exact(F, "cosine", qf, 5)))
say("float_knn_search_over_byte_field", rc_of(lambda: sr.knn_search(F, "l2_norm", qf, 5)))
say("float_search_message", message_of(lambda: sr.knn_exact(F, "cosine", qf, 5)))
hstats = api.IndexStatistics()          # (a text field nobody uploaded: the hybrid entry must refuse the byte field before it plans)
hstats.fields[0] = api.CollectionStatistics(n0 + n1, 10 * (n0 + n1))
hstats.doc_freq[(0, 1)] = 100
srh = api.GpuIndexSearcher(ctx, [g0, g1], hstats)
first = api.TopDocs(np.array([1, 2], dtype=np.int32), np.array([1.0, 0.5], dtype=np.float32), 2, False)
say("rescore_over_byte_field", rc_of(lambda: sr.rescore_vectors(first, F, "cosine", qf[0], 2)))
say("hybrid_over_byte_field", rc_of(lambda: srh.search_hybrid_batch([api.TermQuery(0, 1)], [api.TopScoreDocCollectorManager(10)], F, "cosine", qf[:1], 5)))
say("hybrid_message", message_of(lambda: srh.search_hybrid_batch([api.TermQuery(0, 1)], [api.TopScoreDocCollectorManager(10)], F, "cosine", qf[:1], 5)))
say("byte_search_over_float_field", rc_of(lambda: sr.knn_exact_bytes(F + 1, "cosine", np.ones((1, 16), dtype=np.int8), 5)))
say("byte_search_message", message_of(lambda: sr.knn_exact_bytes(F + 1, "cosine", np.ones((1, 16), dtype=np.int8), 5)))
say("wrong_dim", rc_of(lambda: sr.knn_exact_bytes(F, "cosine", np.ones((1, dim + 1), dtype=np.int8), 5)))
say("search_dim_2049", rc_of(lambda: sr.knn_exact_bytes(F, "cosine", np.ones((1, 2049), dtype=np.int8), 5)))
say("k_1025", rc_of(lambda: sr.knn_exact_bytes(F, "cosine", q1, 1025)))
outs, docs, scores = api._topdocs_outputs(1, 5)
say("sim_4", L.nrtgpu_knn_exact_bytes(ctx._h, sr._segs, sr._bases, 2, F, 4, q1.ctypes.data, 1, dim, 5, C.c_float(1.0), outs))
say("negative_boost", rc_of(lambda: sr.knn_exact_bytes(F, "l2_norm", q1, 5, boost=-1.0)))
zero = np.zeros((1, dim), dtype=np.int8)
say("zero_query_cosine", rc_of(lambda: sr.knn_exact_bytes(F, "cosine", zero, 5)))
say("zero_query_dot_product", rc_of(lambda: sr.knn_exact_bytes(F, "dot_product", zero, 5)))
L.nrtgpu_set_thread_deadline_ns(L.nrtgpu_monotonic_ns() - 1)
say("expired_deadline", rc_of(lambda: sr.knn_exact_bytes(F, "cosine", q1, 5)))
L.nrtgpu_set_thread_deadline_ns(0)
try:
    sr.knn_exact_bytes(F, "cosine", q1.astype(np.float32), 5)
    say("float_array_is_a_type_error", False)
except TypeError:
    say("float_array_is_a_type_error", True)
try:
    sr.knn_exact_bytes(F, "normalized_cosine", q1, 5)
    say("normalized_cosine_refused", False)
except ValueError:
    say("normalized_cosine_refused", True)
for g in (fork, g0, g1):
    g.release()
ctx.close()
print("done", flush=True)
