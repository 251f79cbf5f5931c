"""Run by tests/test_float_rescore_host.py in a subprocess with tests/mockhip preloaded (kernels do nothing): the HOST paths of the
rescorers over a float vector field -- nrtgpu_rescore_vectors and nrtgpu_search_hybrid_batch, the twins of
tests/mockhip/byte_rescore_host.py's entries: calls with 1 and 130 queries, the refusals with their status codes and messages, the
deadline.  One `name value` line per case; MOCKHIP_TRACE must be set (the gather launches of a rescore call are counted).  `--null-segment` adds the call with a NULL pointer in the middle of `segs` (a library
from before the rescorers shared one host path dereferenced it)."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from nrtsearch_amd import _lib, api, synth   # noqa: E402

L = _lib.load()
rng = np.random.default_rng(9)
dim, FF, FB = 100, 4, 3          # the float field (resident padded to 112), a byte field
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


# a text field to recall from; leaf 0: float rows for every doc, leaf 1: a sparse ord -> doc map, leaf 2: no vectors at all
corpus = synth.build_corpus(6000, [2, 9, 70], n_segments=3)
leaves = []
for si, seg in enumerate(corpus.segments):
    g = api.GpuSegment(ctx, seg.max_doc, seg.doc_base)
    g.add_field_norms(0, seg.norms)
    g.add_terms(0, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
    if si == 0:
        g.add_vectors(FF, rng.standard_normal((seg.max_doc, dim)).astype(np.float32))
    if si == 1:
        have = np.flatnonzero(rng.random(seg.max_doc) < 0.5).astype(np.int32)
        g.add_vectors(FF, rng.standard_normal((len(have), dim)).astype(np.float32), have)
    if si < 2:
        g.add_byte_vectors(FB, rng.integers(-128, 128, size=(seg.max_doc, 16), dtype=np.int8))
    g.seal()
    leaves.append(g)
sr = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics.from_corpus(corpus))
max_doc = sum(s.max_doc for s in corpus.segments)


def bq(terms):
    return api.BooleanQuery(tuple(api.TermQuery(0, int(t)) for t in terms))


def hybrid(nq, sim="cosine", qv=None, field=FF, window=50, qw=1.0, rw=2.0, boost=1.0):
    qs = [bq([2, 70]) if i % 2 else bq([9]) for i in range(nq)]
    mg = [api.TopScoreDocCollectorManager(300)] * nq
    if qv is None:
        qv = rng.standard_normal((nq, dim)).astype(np.float32)
    got = sr.search_hybrid_batch(qs, mg, field, sim, qv, window, qw, rw, boost)
    assert len(got) == nq and all(len(t.docs) == len(t.scores) <= window for t in got)
    return got


# hits in all three leaves: 1 and 7 in leaf 0 (row == doc); in leaf 1 a doc whose row the sparse map holds and one it does not;
# 5000 in leaf 2 (no vectors)
base1, base2 = corpus.segments[1].doc_base, corpus.segments[2].doc_base
assert base1 <= 3100 < base2 <= 5000
mapped = base1 + int(have[5])
unmapped = base1 + int(np.setdiff1d(np.arange(corpus.segments[1].max_doc), have)[3])
first = api.TopDocs(np.array([1, mapped, 5000, 7, unmapped], dtype=np.int32), np.array([1.0, 0.5, 0.25, 0.125, 0.0625], dtype=np.float32), 5, False)
q1 = rng.standard_normal(dim).astype(np.float32)


def rescore(sim="cosine", q=q1, field=FF, hits=first, window=3, qw=1.0, rw=2.0, boost=1.0):
    got = sr.rescore_vectors(hits, field, sim, q, window, qw, rw, boost)
    assert len(got.docs) == len(got.scores) <= window
    return got


def raw_rescore(segs, sim=0):
    od, os_ = np.zeros(5, np.int32), np.zeros(5, np.float32)
    out = _lib.TopDocs()
    out.capacity = 5
    out.docs = od.ctypes.data_as(C.POINTER(C.c_int32))
    out.scores = os_.ctypes.data_as(C.POINTER(C.c_float))
    return L.nrtgpu_rescore_vectors(ctx._h, segs, sr._bases, 3, FF, sim, q1.ctypes.data, dim, C.c_float(1.0), first.docs.ctypes.data,
                                    first.scores.ctypes.data, 5, 1.0, 1.0, 5, C.byref(out))


say("hybrid_1", rc_of(lambda: hybrid(1)))
say("hybrid_130", rc_of(lambda: hybrid(130)))
say("hybrid_window_above_max_k", rc_of(lambda: hybrid(2, window=5000)))
say("rescore_hit_docs", first.docs.tolist())
launched = len(open(os.environ["MOCKHIP_TRACE"]).readlines())
say("rescore_5_hits", rc_of(lambda: rescore()))
# one gather launch per leaf that has rows and hits (leaves 0 and 1), none for the leaf without vectors
say("rescore_launches", [l.strip() for l in open(os.environ["MOCKHIP_TRACE"]).readlines()[launched:]])
# the kernels do nothing there, so a hit in a leaf with rows scores 0 and the hit in the leaf without rows keeps query_weight x its
# first score: doc 5000 leads, the others -- the leaf-1 doc without a row among them -- follow in docid order
say("rescore_window_below_the_hits", rescore(window=3).docs.tolist())
say("rescore_window_above_the_hits", rescore(window=10).docs.tolist())
say("rescore_no_vectors_leaf_score", rescore(window=10, qw=3.0).scores.tolist())
say("rescore_no_hits", rc_of(lambda: rescore(hits=api.TopDocs(np.zeros(0, np.int32), np.zeros(0, np.float32), 0, False))))
say("rescore_no_hits_window", len(rescore(hits=api.TopDocs(np.zeros(0, np.int32), np.zeros(0, np.float32), 0, False)).docs))
# the float entry checks neither the boost nor the weights (the byte entry refuses these: tests/mockhip/byte_rescore_host.py)
say("rescore_negative_weight", rc_of(lambda: rescore(qw=-1.0, rw=-2.0)))
say("rescore_negative_boost", rc_of(lambda: rescore(boost=-0.5)))
say("rescore_nan_boost", rc_of(lambda: rescore(boost=float("nan"))))
say("rescore_infinite_weight", rc_of(lambda: rescore(rw=float("inf"))))

# refusals: the hybrid entry, then the rescore entry
outs, docs, scores = api._topdocs_outputs(1, 5)
m = sr._marshal([bq([9])], [api.TopScoreDocCollectorManager(10)])
say("hybrid_sim_4", L.nrtgpu_search_hybrid_batch(ctx._h, sr._segs, sr._bases, 3, m.queries, 1, FF, 4, q1.ctypes.data, dim, C.c_float(1.0), 1.0, 1.0,
                                                 5, outs))
say("hybrid_sim_4_message", L.nrtgpu_last_error().decode())
say("hybrid_wrong_dim", rc_of(lambda: hybrid(1, qv=np.ones((1, dim + 1), dtype=np.float32))))
say("hybrid_wrong_dim_message", message_of(lambda: hybrid(1, qv=np.ones((1, dim + 1), dtype=np.float32))))
say("hybrid_byte_field", rc_of(lambda: hybrid(1, field=FB, qv=np.ones((1, 16), dtype=np.float32))))
say("hybrid_byte_field_message", message_of(lambda: hybrid(1, field=FB, qv=np.ones((1, 16), dtype=np.float32))))
say("hybrid_negative_query_weight", rc_of(lambda: hybrid(1, qw=-1.0)))
say("hybrid_negative_weight_message", message_of(lambda: hybrid(1, rw=-0.5)))
say("hybrid_window_0", rc_of(lambda: hybrid(1, window=0)))

say("rescore_sim_4", raw_rescore(sr._segs, sim=4))
say("rescore_sim_4_message", L.nrtgpu_last_error().decode())
say("rescore_wrong_dim", rc_of(lambda: rescore(q=np.ones(dim - 1, dtype=np.float32))))
say("rescore_wrong_dim_message", message_of(lambda: rescore(q=np.ones(dim - 1, dtype=np.float32))))
say("rescore_byte_field", rc_of(lambda: rescore(field=FB, q=np.ones(16, dtype=np.float32))))
say("rescore_byte_field_message", message_of(lambda: rescore(field=FB, q=np.ones(16, dtype=np.float32))))
outside = api.TopDocs(np.array([1, max_doc], dtype=np.int32), np.array([1.0, 0.5], dtype=np.float32), 2, False)
say("rescore_hit_outside_every_segment", rc_of(lambda: rescore(hits=outside)))
say("rescore_outside_message", message_of(lambda: rescore(hits=outside)))

L.nrtgpu_set_thread_deadline_ns(L.nrtgpu_monotonic_ns() - 1)
say("hybrid_expired_deadline", rc_of(lambda: hybrid(3)))
say("hybrid_expired_deadline_message", message_of(lambda: hybrid(3)))
L.nrtgpu_set_thread_deadline_ns(0)
say("hybrid_after_the_deadline_was_cleared", rc_of(lambda: hybrid(3)))

if "--null-segment" in sys.argv:
    holed = (C.c_void_p * 3)(*[l._h for l in leaves])
    holed[1] = None
    say("rescore_null_segment", raw_rescore(holed))
    say("rescore_null_segment_message", L.nrtgpu_last_error().decode())
    say("rescore_after_the_null_segment", raw_rescore(sr._segs))
for g in leaves:
    g.release()
ctx.close()
print("done", flush=True)
