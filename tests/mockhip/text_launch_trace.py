"""Run by tests/test_text_launch_schedule_host.py in a subprocess with tests/mockhip preloaded, MOCKHIP_TRACE and MOCKHIP_TRACE_OPS
set: what the TEXT paths' host code (search.cpp, finalscore.cpp) puts on a stream -- the batch entry at three sizes, a batch with
both scorers, speculation off, collect_timing on and off, the two-pass paths (mockhip_poke_arg makes merge_topk_kernel leave
kHitsSpecInvalid in a hit total), the hybrid entries, the device-resident entries (synchronous, through the launcher thread, one
shard of several), the merge of gathered lists, the final-score routes, the coalescer, and every entry's refusals in the order
its prologue makes them.  Prints, per step, the deltas of the context's counters and every kernel launch (name, grid.x, block.x,
dynamic shared bytes), copy, memset, event record, stream wait and synchronisation of the step.  The kernels do nothing there, so
every answer is empty; "device" buffers of the caller are numpy arrays (`ext` in the trace)."""
import ctypes as C
import faulthandler
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from nrtsearch_amd import _lib, api, synth, workload   # noqa: E402

faulthandler.dump_traceback_later(300, exit=True)
TRACE = os.environ["MOCKHIP_TRACE"]
COUNTERS = ("batches", "queries", "scan_launches", "fixed_point_launches", "maxscore_launches", "scan_items", "maxscore_items",
            "scan_postings", "maxscore_postings", "spec_queries", "spec_reruns")
SPEC_INVALID = 1 << 47   # plan.h: kHitsSpecInvalid
MERGE_OUT_HITS = 10      # merge_topk_kernel's out_hits argument
mock = C.CDLL(None)
mock.mockhip_poke_arg.argtypes = [C.c_char_p, C.c_int, C.c_long, C.c_uint64, C.c_int]
mock.mockhip_poke_arg.restype = None
L = _lib.load()
seen = 0


def step(name, ctx, fn, lines=True, diag=False):
    global seen
    before = ctx.stats()
    fn()
    after = ctx.stats()
    print("==", name, " ".join(f"{c}=+{after[c] - before[c]}" for c in COUNTERS))
    if diag:
        d = api.GpuContext.last_diagnostics()
        print("diagnostics", " ".join(f"{n}={d[n]}" for n in ("queries", "postings", "items_maxscore", "items_scan")), f"device_ms={d['device_ms']:.4f}")
    got = open(TRACE).read().split("\n")[:-1]
    print("\n".join(got[seen:]) if lines else f"({len(got) - seen} lines)")
    seen = len(got)


def tag(elems, value=SPEC_INVALID):
    """the next merge_topk_kernel launch leaves `value` in these queries' hit totals"""
    for q in elems:
        mock.mockhip_poke_arg(b"merge_topk_kernel", MERGE_OUT_HITS, q, value, 1)


def refusal(name, call):
    rc = call()
    try:
        _lib.check(rc)
        print("refusal", name, 0)
    except api.NrtGpuError as e:
        print("refusal", name, e.code, str(e))


w = workload.Workload("t", 120_000, 3, 50, 16, 3)
qr = synth.make_queries(300, w.n_terms, w.max_rank)
corpus = workload.build_shard_corpus(w, qr)
rng = np.random.default_rng(7)
FF, FB, DIM = 1, 2, 20
queries = workload.boolean_queries(qr)
top = api.TopScoreDocCollectorManager(w.k)
floor = api.TopScoreDocCollectorManager(w.k, None, api.TOTAL_HITS_THRESHOLD, 0.5)   # min_competitive_score: the exhaustive scan


def make(collect_timing, max_batch=512, flags=0):
    ctx = api.GpuContext(device_id=0, max_batch=max_batch, collect_timing=collect_timing, flags=flags)
    leaves = []
    for seg in corpus.segments:
        g = api.GpuSegment(ctx, seg.max_doc, seg.doc_base)
        g.add_field_norms(0, seg.norms)
        g.add_terms(0, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
        g.add_vectors(FF, np.zeros((seg.max_doc, DIM), dtype=np.float32))
        g.add_byte_vectors(FB, np.ones((seg.max_doc, DIM), dtype=np.int8))
        g.seal()
        leaves.append(g)
    return ctx, leaves, api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics.from_corpus(corpus))


def close(ctx, leaves):
    for g in leaves:
        g.release()
    ctx.close()


ctx, leaves, sr = make(True)
step("build", ctx, lambda: None, lines=False)
# 1. the batch entry: one query, a few, enough for the parallel unpack
for n in (1, 16, 300):
    step(f"search_batch_{n}", ctx, lambda: sr.search_batch(queries[:n], [top] * n), diag=True)
    print("spec_counters", ctx.spec_counters())
# 2. both scorers in one call, 3. the same without speculation
mixed = [top if i % 3 else floor for i in range(24)]
step("search_batch_mixed", ctx, lambda: sr.search_batch(queries[:24], mixed), diag=True)
ctx.set_speculation(0)
step("search_batch_mixed_no_speculation", ctx, lambda: sr.search_batch(queries[:24], mixed), diag=True)
step("search_batch_16_no_speculation", ctx, lambda: sr.search_batch(queries[:16], [top] * 16), diag=True)
ctx.set_speculation(5.0)
# 5. one tagged query: the second pass is a follow-up launch; 6. more than 32: a batch of its own
tag([3])
step("search_batch_16_one_tagged", ctx, lambda: sr.search_batch(queries[:16], [top] * 16), diag=True)
print("spec_counters", ctx.spec_counters())
tag([3], 0)
step("search_batch_16_untagged_again", ctx, lambda: sr.search_batch(queries[:16], [top] * 16), diag=True)
tag(range(5, 45))
step("search_batch_64_forty_tagged", ctx, lambda: sr.search_batch(queries[:64], [top] * 64), diag=True)
print("spec_counters", ctx.spec_counters())
tag(range(5, 45), 0)
step("search_batch_64_untagged_again", ctx, lambda: sr.search_batch(queries[:64], [top] * 64), diag=True)
# 7. the hybrid entries, clean and with one tagged query
qf = rng.standard_normal((40, DIM)).astype(np.float32)
qb = rng.integers(-100, 100, size=(40, DIM), dtype=np.int8)
for name, fn, field, qv in (("hybrid", sr.search_hybrid_batch, FF, qf), ("hybrid_bytes", sr.search_hybrid_bytes_batch, FB, qb)):
    step(f"search_{name}_batch", ctx, lambda: fn(queries[:40], [top] * 40, field, "cosine", qv, 20, 1.0, 2.0), diag=True)
    tag([7])
    step(f"search_{name}_batch_one_tagged", ctx, lambda: fn(queries[:40], [top] * 40, field, "cosine", qv, 20, 1.0, 2.0), diag=True)
    print("spec_counters", ctx.spec_counters())
    tag([7], 0)
    step(f"search_{name}_batch_untagged_again", ctx, lambda: fn(queries[:40], [top] * 40, field, "cosine", qv, 20, 1.0, 2.0))
# 8. - 10. device-resident results
B, ks = 32, 64
pb = api.PreparedBatch(sr, queries[:B], [top] * B)
d_keys, d_cnt, d_hits, d_guess = np.zeros((B, ks), np.uint64), np.zeros(B, np.uint32), np.zeros(B, np.uint64), np.zeros(B, np.uint64)
ptrs = (d_keys.ctypes.data, d_cnt.ctypes.data, d_hits.ctypes.data)
step("run_device", ctx, lambda: pb.run_device(ks, *ptrs), diag=True)
step("begin_wait_device", ctx, lambda: api.PreparedBatch.wait_device(pb.begin_device(ks, *ptrs)), diag=True)
d_hits[3] = SPEC_INVALID   # (the caller's own array: nothing overwrites it, nrtgpu_pending_wait runs the whole batch again)
step("begin_wait_device_pre_tagged", ctx, lambda: api.PreparedBatch.wait_device(pb.begin_device(ks, *ptrs)), diag=True)
print("spec_counters", ctx.spec_counters())
d_hits[:] = 0
step("begin_shard_device_world_2", ctx, lambda: api.PreparedBatch.wait_device(pb.begin_shard_device(ks, *ptrs, 2, d_guess.ctypes.data)), diag=True)
step("begin_shard_device_world_0", ctx, lambda: api.PreparedBatch.wait_device(pb.begin_shard_device(ks, *ptrs, 0, d_guess.ctypes.data)), diag=True)
# 11. the merge of gathered lists
for nl, nq in ((2, 8), (8, 70)):
    gk, gc, gh = np.zeros((nl * nq, ks), np.uint64), np.zeros(nl * nq, np.uint32), np.zeros(nl * nq, np.uint64)
    step(f"merge_topk_device_{nl}x{nq}", ctx,
         lambda: api.merge_topk_device(ctx, nl, nq, ks, gk.ctypes.data, gc.ctypes.data, gh.ctypes.data, [w.k] * nq, [api.TOTAL_HITS_THRESHOLD] * nq))
# 12. the final-score routes
fsq = [api.FunctionScoreQuery(q, (api.WeightFunction(2.5, 0),), "multiply", "multiply") for q in queries[:9]]
step("search_function_score_batch", ctx, lambda: sr.search_function_score_batch(fsq, [top] * 9), diag=True)
mmq = [api.MultiMatchQuery("cross_fields", tuple((api.TermQuery(0, int(t)),) for t in row)) for row in qr[:9]]
step("search_multi_match_batch", ctx, lambda: sr.search_multi_match_batch(mmq, [top] * 9), diag=True)
# 13. the coalescer
step("search_coalesced", ctx, lambda: sr.search_coalesced(queries[0], top), diag=True)
close(ctx, leaves)

# 4. collect_timing off
ctx, leaves, sr = make(False)
step("build_no_timing", ctx, lambda: None, lines=False)
step("search_batch_16_no_timing", ctx, lambda: sr.search_batch(queries[:16], [top] * 16), diag=True)
step("search_batch_mixed_no_timing", ctx, lambda: sr.search_batch(queries[:24], mixed), diag=True)
tag([3])
step("search_batch_16_one_tagged_no_timing", ctx, lambda: sr.search_batch(queries[:16], [top] * 16), diag=True)
step("search_hybrid_batch_no_timing", ctx, lambda: sr.search_hybrid_batch(queries[:40], [top] * 40, FF, "cosine", qf, 20, 1.0, 2.0), diag=True)
pb = api.PreparedBatch(sr, queries[:B], [top] * B)
d_hits[:] = 0
step("begin_wait_device_no_timing", ctx, lambda: api.PreparedBatch.wait_device(pb.begin_device(ks, *ptrs)), diag=True)
step("search_function_score_batch_no_timing", ctx, lambda: sr.search_function_score_batch(fsq, [top] * 9), diag=True)
close(ctx, leaves)

# the caller sleeps on an event (NRTGPU_FLAG_BLOCKING_WAIT); TEXT_TRACE_PROFILE=1 (by hand, with the development library: the
# product has no instrumented variant, and the recorded schedule is the product's): that variant zeroes its profile buffers itself
for name, flags in (("blocking_wait", _lib.NRTGPU_FLAG_BLOCKING_WAIT),) + ((("profile", _lib.NRTGPU_FLAG_PROFILE),) if os.environ.get("TEXT_TRACE_PROFILE") else ()):
    ctx, leaves, sr = make(True, flags=flags)
    step(f"build_{name}", ctx, lambda: None, lines=False)
    step(f"search_batch_mixed_{name}", ctx, lambda: sr.search_batch(queries[:24], mixed), diag=True)
    tag([3])
    step(f"search_batch_16_one_tagged_{name}", ctx, lambda: sr.search_batch(queries[:16], [top] * 16), diag=True)
    pb = api.PreparedBatch(sr, queries[:B], [top] * B)
    d_hits[:] = 0
    d_hits[3] = SPEC_INVALID
    step(f"begin_wait_device_pre_tagged_{name}", ctx, lambda: api.PreparedBatch.wait_device(pb.begin_device(ks, *ptrs)), diag=True)
    step(f"search_multi_match_batch_{name}", ctx, lambda: sr.search_multi_match_batch(mmq, [top] * 9), diag=True)
    step(f"merge_topk_device_{name}", ctx,
         lambda: api.merge_topk_device(ctx, 2, 8, ks, d_keys.ctypes.data, d_cnt.ctypes.data, d_hits.ctypes.data, [w.k] * 8, [api.TOTAL_HITS_THRESHOLD] * 8))
    close(ctx, leaves)

# 14. what every entry answers to a bad call, check by check
ctx, leaves, sr = make(False, max_batch=8)
step("build_refusals", ctx, lambda: None, lines=False)
n_seg = len(leaves)
m = sr._marshal(queries[:9], [top] * 9)
fs = sr._marshal_function_scores(fsq, m)
mm, gs = sr._marshal_multi_match(mmq, [top] * 9)
outs = (_lib.TopDocs * 9)()
holes = (C.c_void_p * n_seg)(*[None if i == 1 else g._h for i, g in enumerate(leaves)])
h = C.c_void_p()
vec, bvec = qf.ctypes.data, qb.ctypes.data
entries = {
    "batch": lambda q, n, segs: L.nrtgpu_search_bm25_batch(ctx._h, segs, sr._bases, n_seg, q, n, outs),
    "hybrid": lambda q, n, segs: L.nrtgpu_search_hybrid_batch(ctx._h, segs, sr._bases, n_seg, q, n, FF, 0, vec, DIM, 1.0, 1.0, 2.0, 20, outs),
    "hybrid_bytes": lambda q, n, segs: L.nrtgpu_search_hybrid_bytes_batch(ctx._h, segs, sr._bases, n_seg, q, n, FB, 0, bvec, DIM, 1.0, 1.0, 2.0, 20, outs),
    "device": lambda q, n, segs: L.nrtgpu_search_bm25_batch_device_epoch(ctx._h, segs, sr._bases, n_seg, q, n, ks, *ptrs, -1),
    "device_begin": lambda q, n, segs: L.nrtgpu_search_bm25_batch_device_begin(ctx._h, segs, sr._bases, n_seg, q, n, ks, *ptrs, -1, C.byref(h)),
    "shard_begin": lambda q, n, segs: L.nrtgpu_search_bm25_shard_device_begin(ctx._h, segs, sr._bases, n_seg, q, n, ks, *ptrs, 2, d_guess.ctypes.data, C.byref(h)),
    "function_score": lambda q, n, segs: L.nrtgpu_search_function_score_batch(ctx._h, segs, sr._bases, n_seg, q, fs, n, outs),
    "multi_match": lambda q, n, segs: L.nrtgpu_search_multi_match_batch(ctx._h, segs, sr._bases, n_seg, q if q is None else mm.queries, gs, n, outs),
}
for name, call in entries.items():
    refusal(f"{name} null_queries", lambda: call(None, 4, sr._segs))
    refusal(f"{name} no_queries", lambda: call(m.queries, 0, sr._segs))
    refusal(f"{name} above_max_batch", lambda: call(m.queries, 9, sr._segs))
    refusal(f"{name} null_leaf", lambda: call(m.queries, 4, holes))
    api.GpuContext.set_thread_deadline(-1.0)
    refusal(f"{name} deadline", lambda: call(m.queries, 4, sr._segs))
    # where the checks meet: which of two faults of one call an entry names
    refusal(f"{name} deadline_and_no_queries", lambda: call(m.queries, 0, sr._segs))
    refusal(f"{name} deadline_and_above_max_batch", lambda: call(m.queries, 9, sr._segs))
    refusal(f"{name} deadline_and_null_leaf", lambda: call(m.queries, 4, holes))
    api.GpuContext.set_thread_deadline(None)
    refusal(f"{name} above_max_batch_and_null_leaf", lambda: call(m.queries, 9, holes))
for name in ("hybrid", "hybrid_bytes"):
    fn = getattr(L, f"nrtgpu_search_{name}_batch")
    field, v = (FF, vec) if name == "hybrid" else (FB, bvec)
    refusal(f"{name} negative_weight", lambda: fn(ctx._h, sr._segs, sr._bases, n_seg, m.queries, 4, field, 0, v, DIM, 1.0, -1.0, 2.0, 20, outs))
    refusal(f"{name} negative_weight_above_max_batch", lambda: fn(ctx._h, sr._segs, sr._bases, n_seg, m.queries, 9, field, 0, v, DIM, 1.0, -1.0, 2.0, 20, outs))
    refusal(f"{name} bad_window_null_leaf", lambda: fn(ctx._h, holes, sr._bases, n_seg, m.queries, 4, field, 0, v, DIM, 1.0, 1.0, 2.0, 0, outs))
    refusal(f"{name} other_dimension", lambda: fn(ctx._h, sr._segs, sr._bases, n_seg, m.queries, 4, field, 0, v, DIM + 1, 1.0, 1.0, 2.0, 20, outs))
    refusal(f"{name} other_element_type", lambda: fn(ctx._h, sr._segs, sr._bases, n_seg, m.queries, 4, FF + FB - field, 0, v, DIM, 1.0, 1.0, 2.0, 20, outs))
for name in ("device", "device_begin", "shard_begin"):
    short = {"device": lambda: L.nrtgpu_search_bm25_batch_device_epoch(ctx._h, sr._segs, sr._bases, n_seg, m.queries, 4, 16, *ptrs, -1),
             "device_begin": lambda: L.nrtgpu_search_bm25_batch_device_begin(ctx._h, sr._segs, sr._bases, n_seg, m.queries, 4, 16, *ptrs, -1, C.byref(h)),
             "shard_begin": lambda: L.nrtgpu_search_bm25_shard_device_begin(ctx._h, sr._segs, sr._bases, n_seg, m.queries, 4, 16, *ptrs, 2, d_guess.ctypes.data, C.byref(h))}[name]
    refusal(f"{name} k_stride_below_k", short)
refusal("shard_begin no_guess_buffer", lambda: L.nrtgpu_search_bm25_shard_device_begin(ctx._h, sr._segs, sr._bases, n_seg, m.queries, 4, ks, *ptrs, 2, None, C.byref(h)))
step("refusals", ctx, lambda: None)
step("search_batch_after_refusals", ctx, lambda: sr.search_batch(queries[:4], [top] * 4), diag=True)
close(ctx, leaves)
print("done", flush=True)
