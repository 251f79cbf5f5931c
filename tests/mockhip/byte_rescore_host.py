"""Run by tests/test_byte_rescore_host.py in a subprocess with tests/mockhip preloaded (kernels do nothing): the HOST paths of the
rescorers over a byte (int8) vector field -- nrtgpu_rescore_byte_vectors and nrtgpu_search_hybrid_bytes_batch: calls with 1 and
130 queries, every refusal of include/nrtgpu.h with its status code and message, the deadline.  One `name value` line per case."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from nrtsearch_amd import _lib, api, synth   # noqa: E402

L = _lib.load()
rng = np.random.default_rng(9)
dim, FB, FF = 100, 3, 4          # the byte field, a float field
ctx = api.GpuContext(device_id=0, max_batch=256)


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


# a text field to recall from; leaf 0: byte rows for every doc, leaf 1: a sparse ord -> doc map, leaf 2: no vectors at all
corpus = synth.build_corpus(6000, [2, 9, 70], n_segments=3)
leaves = []
for si, seg in enumerate(corpus.segments):
    g = api.GpuSegment(ctx, seg.max_doc, seg.doc_base)
    g.add_field_norms(0, seg.norms)
    g.add_terms(0, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
    if si == 0:
        g.add_byte_vectors(FB, rng.integers(-128, 128, size=(seg.max_doc, dim), dtype=np.int8))
    if si == 1:
        have = np.flatnonzero(rng.random(seg.max_doc) < 0.5).astype(np.int32)
        g.add_byte_vectors(FB, rng.integers(-128, 128, size=(len(have), dim), dtype=np.int8), have)
    if si < 2:
        g.add_vectors(FF, rng.standard_normal((seg.max_doc, 16)).astype(np.float32))
    g.seal()
    leaves.append(g)
sr = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics.from_corpus(corpus))
max_doc = sum(s.max_doc for s in corpus.segments)


def bq(terms):
    return api.BooleanQuery(tuple(api.TermQuery(0, int(t)) for t in terms))


def hybrid(nq, sim="cosine", qv=None, field=FB, window=50, qw=1.0, rw=2.0, boost=1.0):
    qs = [bq([2, 70]) if i % 2 else bq([9]) for i in range(nq)]
    mg = [api.TopScoreDocCollectorManager(300)] * nq
    if qv is None:
        qv = rng.integers(-128, 128, size=(nq, dim), dtype=np.int8)
    got = sr.search_hybrid_bytes_batch(qs, mg, field, sim, qv, window, qw, rw, boost)
    assert len(got) == nq and all(len(t.docs) == len(t.scores) <= window for t in got)
    return got


first = api.TopDocs(np.array([1, 2500, 5000, 7], dtype=np.int32), np.array([1.0, 0.5, 0.25, 0.125], dtype=np.float32), 4, False)
q1 = rng.integers(-128, 128, size=dim, dtype=np.int8)


def rescore(sim="cosine", q=q1, field=FB, hits=first, window=3, qw=1.0, rw=2.0, boost=1.0):
    got = sr.rescore_byte_vectors(hits, field, sim, q, window, qw, rw, boost)
    assert len(got.docs) == len(got.scores) <= window
    return got


say("hybrid_1", rc_of(lambda: hybrid(1)))
say("hybrid_130", rc_of(lambda: hybrid(130)))
say("hybrid_window_above_max_k", rc_of(lambda: hybrid(2, window=5000)))
say("rescore_4_hits", rc_of(lambda: rescore()))
say("rescore_keeps_window", len(rescore(window=3).docs) == 3 and len(rescore(window=10).docs) == 4)
say("rescore_no_hits", rc_of(lambda: rescore(hits=api.TopDocs(np.zeros(0, np.int32), np.zeros(0, np.float32), 0, False))))
say("rescore_negative_weight", rc_of(lambda: rescore(qw=-1.0, rw=-2.0)))          # sorted on the host: any finite weights

# refusals: the hybrid entry, then the rescore entry
zero = np.zeros(dim, dtype=np.int8)
outs, docs, scores = api._topdocs_outputs(1, 5)
m = sr._marshal([bq([9])], [api.TopScoreDocCollectorManager(10)])
say("hybrid_sim_4", L.nrtgpu_search_hybrid_bytes_batch(ctx._h, sr._segs, sr._bases, 3, m.queries, 1, FB, 4, q1.ctypes.data, dim, C.c_float(1.0),
                                                       1.0, 1.0, 5, outs))
say("hybrid_zero_query_cosine", rc_of(lambda: hybrid(2, qv=np.stack([q1, zero]))))
say("hybrid_zero_query_l2_norm", rc_of(lambda: hybrid(2, sim="l2_norm", qv=np.stack([q1, zero]))))
say("hybrid_wrong_dim", rc_of(lambda: hybrid(1, qv=np.ones((1, dim + 1), dtype=np.int8))))
say("hybrid_float_field", rc_of(lambda: hybrid(1, field=FF, qv=np.ones((1, 16), dtype=np.int8))))
say("hybrid_float_field_message", message_of(lambda: hybrid(1, field=FF, qv=np.ones((1, 16), dtype=np.int8))))
say("hybrid_negative_boost", rc_of(lambda: hybrid(1, boost=-1.0)))
say("hybrid_infinite_boost", rc_of(lambda: hybrid(1, boost=float("inf"))))
say("hybrid_nan_boost", rc_of(lambda: hybrid(1, boost=float("nan"))))
say("hybrid_dim_2049", rc_of(lambda: hybrid(1, qv=np.ones((1, 2049), dtype=np.int8))))
say("hybrid_negative_query_weight", rc_of(lambda: hybrid(1, qw=-1.0)))
say("hybrid_negative_rescore_weight", rc_of(lambda: hybrid(1, rw=-0.5)))
say("hybrid_negative_weight_message", message_of(lambda: hybrid(1, rw=-0.5)))
say("hybrid_window_0", rc_of(lambda: hybrid(1, window=0)))

od, os_ = np.zeros(4, np.int32), np.zeros(4, np.float32)
out = _lib.TopDocs()
out.capacity = 4
out.docs = od.ctypes.data_as(C.POINTER(C.c_int32))
out.scores = os_.ctypes.data_as(C.POINTER(C.c_float))
say("rescore_sim_4", L.nrtgpu_rescore_byte_vectors(ctx._h, sr._segs, sr._bases, 3, FB, 4, q1.ctypes.data, dim, C.c_float(1.0), first.docs.ctypes.data,
                                                   first.scores.ctypes.data, 4, 1.0, 1.0, 4, C.byref(out)))
say("rescore_zero_query_cosine", rc_of(lambda: rescore(q=zero)))
say("rescore_zero_query_dot_product", rc_of(lambda: rescore(sim="dot_product", q=zero)))
say("rescore_wrong_dim", rc_of(lambda: rescore(q=np.ones(dim - 1, dtype=np.int8))))
say("rescore_float_field", rc_of(lambda: rescore(field=FF, q=np.ones(16, dtype=np.int8))))
say("rescore_float_field_message", message_of(lambda: rescore(field=FF, q=np.ones(16, dtype=np.int8))))
say("rescore_negative_boost", rc_of(lambda: rescore(boost=-0.5)))
say("rescore_nan_boost", rc_of(lambda: rescore(boost=float("nan"))))
say("rescore_infinite_weight", rc_of(lambda: rescore(rw=float("inf"))))
say("rescore_dim_2049", rc_of(lambda: rescore(q=np.ones(2049, dtype=np.int8))))
outside = api.TopDocs(np.array([1, max_doc], dtype=np.int32), np.array([1.0, 0.5], dtype=np.float32), 2, False)
say("rescore_hit_outside_every_segment", rc_of(lambda: rescore(hits=outside)))
say("rescore_outside_message", message_of(lambda: rescore(hits=outside)))

# the float entries over the byte field, and the reverse (above): both refuse
qf = rng.standard_normal((1, dim)).astype(np.float32)
say("float_rescore_over_byte_field", rc_of(lambda: sr.rescore_vectors(first, FB, "cosine", qf[0], 2)))
say("float_hybrid_over_byte_field", rc_of(lambda: sr.search_hybrid_batch([bq([9])], [api.TopScoreDocCollectorManager(10)], FB, "cosine", qf, 5)))
say("float_hybrid_over_float_field", rc_of(lambda: sr.search_hybrid_batch([bq([9])], [api.TopScoreDocCollectorManager(10)], FF, "cosine",
                                                                          rng.standard_normal((1, 16)).astype(np.float32), 5)))

L.nrtgpu_set_thread_deadline_ns(L.nrtgpu_monotonic_ns() - 1)
say("hybrid_expired_deadline", rc_of(lambda: hybrid(3)))
L.nrtgpu_set_thread_deadline_ns(0)
say("hybrid_after_the_deadline_was_cleared", rc_of(lambda: hybrid(3)))

for name, fn in (("hybrid_float_array_is_a_type_error", lambda: hybrid(1, qv=np.ones((1, dim), dtype=np.float32))),
                 ("rescore_float_array_is_a_type_error", lambda: rescore(q=q1.astype(np.float32))),
                 ("rescore_int32_array_is_a_type_error", lambda: rescore(q=q1.astype(np.int32)))):
    try:
        fn()
        say(name, False)
    except TypeError:
        say(name, True)
for name, fn in (("hybrid_normalized_cosine_refused", lambda: hybrid(1, sim="normalized_cosine")),
                 ("rescore_normalized_cosine_refused", lambda: rescore(sim="normalized_cosine"))):
    try:
        fn()
        say(name, False)
    except ValueError:
        say(name, True)
for g in leaves:
    g.release()
ctx.close()
print("done", flush=True)
