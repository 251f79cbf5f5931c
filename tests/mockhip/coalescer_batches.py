"""Run by tests/test_coalescer_host.py in a subprocess with tests/mockhip preloaded (MOCKHIP_SYNC_US: what a stream synchronisation
"takes") and the development library: which requests nrtgpu_search_bm25_coalesced and nrtgpu_knn_exact_coalesced send to the device
together, and what every caller is told, for batches formed BY CONSTRUCTION -- the callers of a scenario are parked behind
nrtgpu_debug_hold_coalescers until nrtgpu_debug_coalescer_pending reports them all, then released -- not by thread timing.
Prints, per scenario, the deltas of the context's counters and the sorted multiset of (rc, first 80 characters of the error) over
the callers.  Nothing printed depends on the order the callers arrived in.  A HIP failure's text ends with the source position of
the call that saw it, "(<path>:<line>)": printed as "(FILE:LINE)", so that neither the checkout's directory nor an edit above that
line changes the output."""
import ctypes as C
import faulthandler
import os
import re
import sys
import threading
import time
from collections import Counter

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from nrtsearch_amd import _lib, api, synth, workload   # noqa: E402

faulthandler.dump_traceback_later(120, exit=True)
mock = C.CDLL(os.environ["LD_PRELOAD"])
COUNTERS = ("batches", "queries", "knn_panels", "knn_second_passes", "spec_reruns")
BM25, KNN = 0, 1
FV, DIM = 1, 16

w = workload.Workload("coalescer batches", 150_000, 3, 50, 64, 2)
qr = synth.make_queries(64, w.n_terms, w.max_rank)
corpus = workload.build_shard_corpus(w, qr)
rng = np.random.default_rng(7)
ctx = api.GpuContext(0, max_batch=64)
leaves = []
for seg in corpus.segments:
    g = api.GpuSegment(ctx, seg.max_doc, seg.doc_base)
    g.add_field_norms(0, seg.norms)
    g.add_terms(0, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
    g.add_vectors(FV, rng.standard_normal((seg.max_doc, DIM)).astype(np.float32))
    g.seal()
    leaves.append(g)
sr = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics.from_corpus(corpus))
queries = workload.boolean_queries(qr)
mgr = api.TopScoreDocCollectorManager(w.k)
vq = rng.standard_normal((80, DIM)).astype(np.float32)
KS = (1, 10, 37, 100)


def bm25(i, slices=None, deadline=None, query=None):
    def call():
        api.GpuContext.set_thread_slices(slices)
        api.GpuContext.set_thread_deadline(deadline)
        try:
            return sr.search_coalesced(query if query is not None else queries[i % len(queries)], mgr)
        finally:
            api.GpuContext.set_thread_deadline(None)
            api.GpuContext.set_thread_slices(None)
    return call


def knn(i, sim="cosine", deadline=None, dim=DIM):
    def call():
        api.GpuContext.set_thread_deadline(deadline)
        try:
            return sr.knn_exact_coalesced(FV, sim, vq[i % len(vq), :dim] if dim <= DIM else np.ones(dim, np.float32), KS[i % 4])
        finally:
            api.GpuContext.set_thread_deadline(None)
    return call


class Callers:
    """threads that make one call each; what each was told, as (rc, text)"""

    def __init__(self):
        self.threads, self.told, self.mu = [], [], threading.Lock()

    def start(self, calls):
        def run(call):
            try:
                r = call()
                assert len(r.scores) == 0      # the kernels did nothing
                told = (0, "")
            except _lib.NrtGpuError as e:
                text = str(e).split(": ", 1)[1]
                told = (e.code, re.sub(r"\(\S+:\d+\)", "(FILE:LINE)", text)[:80])
            except Exception as e:   # noqa: BLE001
                told = (1, repr(e)[:80])
            with self.mu:
                self.told.append(told)
        for call in calls:
            t = threading.Thread(target=run, args=(call,))
            t.start()
            self.threads.append(t)

    def returned(self):
        with self.mu:
            return len(self.told)

    def join(self):
        for t in self.threads:
            t.join()


def wait_for(what, cond):
    t_end = time.monotonic() + 60.0
    while not cond():
        assert time.monotonic() < t_end, f"waited a minute for {what}"
        time.sleep(0.001)


def scenario(name, which, steps, before_release=None):
    """steps: (calls, pending_after, returned_after) -- start the calls, then wait until the coalescer holds `pending_after` requests
    and `returned_after` callers have come back; then before_release() and the release."""
    before = ctx.stats()
    ctx.debug_hold_coalescers(True)
    cs = Callers()
    try:
        for calls, pending, returned in steps:
            cs.start(calls)
            wait_for(f"{name}: {pending} pending, {returned} back",
                     lambda: ctx.debug_coalescer_pending(which) == pending and cs.returned() == returned)
        if before_release:
            before_release()
    finally:
        ctx.debug_hold_coalescers(False)
    cs.join()
    after = ctx.stats()
    print("==", name, " ".join(f"{c}=+{after[c] - before[c]}" for c in COUNTERS))
    for (rc, text), n in sorted(Counter(cs.told).items()):
        print(f"{n} x rc {rc} `{text}`")
    print("pending", ctx.debug_coalescer_pending(BM25), ctx.debug_coalescer_pending(KNN), flush=True)


# ---- nrtgpu_search_bm25_coalesced
scenario("bm25_32_same_leaves", BM25, [([bm25(i) for i in range(32)], 32, 0)])
scenario("bm25_8_and_8_by_slices", BM25, [([bm25(i, slices=[0, 0] if i % 2 else [0, 1]) for i in range(16)], 16, 0)])
# (the leader leaves with max_batch = 64 while held; the sixteen left behind have a leader of their own, which is held)
scenario("bm25_80_is_64_then_16", BM25, [([bm25(i) for i in range(80)], 16, 64)])
# a mask no leaf holds passes validate_query and is refused by the planner: the batch is re-run member by member
no_such_mask = api.BooleanQuery(queries[0].should, 1, filter=(api.MaskFilter(9),))
scenario("bm25_12_one_refused_by_the_planner", BM25, [([bm25(i, query=no_such_mask if i == 5 else None) for i in range(12)], 12, 0)])
# the first caller (no deadline) leads; one of the eleven behind it has 30 ms, and the batch is held for 100 ms after all have queued
scenario("bm25_deadline_expires_in_the_queue", BM25,
         [([bm25(0)], 1, 0), ([bm25(i, deadline=0.030 if i == 4 else None) for i in range(1, 12)], 12, 0)],
         before_release=lambda: time.sleep(0.100))
scenario("bm25_8_first_launch_fails", BM25, [([bm25(i) for i in range(8)], 8, 0)], before_release=lambda: mock.mockhip_fail_next_launches(1))
print("lone",len(bm25(3)().scores), ctx.debug_coalescer_pending(BM25))

# ---- nrtgpu_knn_exact_coalesced
scenario("knn_32_cosine_16_l2", KNN, [([knn(i, "cosine" if i % 3 else "l2_norm") for i in range(48)], 48, 0)])
scenario("knn_80_is_64_then_16", KNN, [([knn(i) for i in range(80)], 16, 64)])
scenario("knn_deadline_expires_in_the_queue", KNN,
         [([knn(0)], 1, 0), ([knn(i, deadline=0.030 if i == 4 else None) for i in range(1, 12)], 12, 0)],
         before_release=lambda: time.sleep(0.100))
scenario("knn_8_first_launch_fails", KNN, [([knn(i) for i in range(8)], 8, 0)], before_release=lambda: mock.mockhip_fail_next_launches(1))
# a dimension the field does not have: refused before it is queued (nothing is held, nothing was pending)
scenario("knn_wrong_dimension_fails_alone", KNN, [([knn(0, dim=24)], 0, 1)])
print("lone", len(knn(3)().scores), ctx.debug_coalescer_pending(KNN))

for g in leaves:
    g.release()
ctx.close()
print("done", flush=True)
