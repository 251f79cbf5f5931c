"""Run by tests/test_knn_byte_requests_host.py in a subprocess with tests/mockhip preloaded, MOCKHIP_TRACE set and the development
library: what the knn request entries over a byte field launch, and which panels their coalesced callers form, without a GPU.

Part 1 prints, per step, "== <step> knn_panels=+N" and the knn_bytes* kernels the step launched (name, grid.x, block.x, dynamic
shared bytes): nrtgpu_knn_search_bytes with one filter and threshold, the same requests through nrtgpu_knn_search_bytes_requests,
70 mixed requests (a pass of 64 and a pass of 6), 10 mixed requests, and the old entry once more.  The kernels do nothing there, so
every answer is empty and no list overflows.

Part 2 parks callers of nrtgpu_knn_search_bytes_coalesced / nrtgpu_knn_exact_bytes_coalesced behind nrtgpu_debug_hold_coalescers
(tests/mockhip/coalescer_batches.py does the same for the float entries) and prints, per scenario, the panels formed and the sorted
multiset of (rc, first 60 characters of the error) over the callers."""
import faulthandler
import os
import sys
import threading
import time
from collections import Counter

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from nrtsearch_amd import _lib, api   # noqa: E402

faulthandler.dump_traceback_later(120, exit=True)
TRACE = os.environ["MOCKHIP_TRACE"]
FB, FF, DIM = 2, 1, 100
BREQ, BEXACT = 3, 4   # nrtgpu_debug_coalescer_pending's `which`
rng = np.random.default_rng(11)
seen = 0

ctx = api.GpuContext(device_id=0, max_batch=64, collect_timing=True)
leaves, base = [], 0
for n in (40_000, 30_000, 100):
    g = api.GpuSegment(ctx, n, base)
    g.add_byte_vectors(FB, rng.integers(-128, 128, size=(n, DIM), dtype=np.int8))
    g.add_vectors(FF, rng.standard_normal((n, 16)).astype(np.float32))
    g.set_mask(1, np.full((n + 63) // 64, 0x5555555555555555, dtype=np.uint64))
    g.set_mask(2, np.full((n + 63) // 64, 0x3333333333333333, dtype=np.uint64))
    g.seal()
    leaves.append(g)
    base += n
sr = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics())
qb = rng.integers(-128, 128, size=(80, DIM), dtype=np.int8)
F1, F2 = api.MaskFilter(1), api.MaskFilter(2)


def step(name, fn):
    global seen
    before = ctx.stats()["knn_panels"]
    fn()
    print("==", name, f"knn_panels=+{ctx.stats()['knn_panels'] - before}")
    lines = open(TRACE).read().split("\n")[:-1]
    print("\n".join(l for l in lines[seen:] if "knn_bytes" in l))
    seen = len(lines)


step("build", lambda: None)
step("search_bytes_5", lambda: sr.knn_search_bytes(FB, "l2_norm", qb[:5], 10, 2.0, F1, 0.25))
step("requests_equal_5", lambda: sr.knn_search_bytes_requests(FB, "l2_norm", qb[:5], [10] * 5, [2.0] * 5, [F1] * 5, [0.25] * 5))
step("search_bytes_70", lambda: sr.knn_search_bytes(FB, "l2_norm", qb[:70], 10, 2.0, F1, 0.25))
step("requests_equal_70", lambda: sr.knn_search_bytes_requests(FB, "l2_norm", qb[:70], [10] * 70, [2.0] * 70, [F1] * 70, [0.25] * 70))
mixed = lambda n: sr.knn_search_bytes_requests(FB, "l2_norm", qb[:n], [(1, 10, 37, 100)[q % 4] for q in range(n)],   # noqa: E731
                                               [(0.5, 1.0, 2.0)[q % 3] for q in range(n)], [(F1, F2, None)[q % 3] for q in range(n)],
                                               [(0.0, 0.25)[q % 2] for q in range(n)])
step("requests_mixed_70", lambda: mixed(70))
step("requests_mixed_17", lambda: mixed(17))
step("requests_mixed_16", lambda: mixed(16))
step("search_bytes_5_again", lambda: sr.knn_search_bytes(FB, "l2_norm", qb[:5], 10, 2.0, F1, 0.25))

# ---- part 2: the cohorts of the coalesced entries
KS = (1, 10, 37, 100)


def breq(i, sim="cosine", deadline=None, query=None, mask=None):
    def call():
        api.GpuContext.set_thread_deadline(deadline)
        try:
            return sr.knn_search_bytes_coalesced(FB, sim, qb[i % len(qb)] if query is None else query, KS[i % 4], boost=(0.5, 1.0, 2.0)[i % 3],
                                                 filter=(F1, F2, None)[i % 3] if mask is None else api.MaskFilter(mask), min_score=(0.0, 0.25)[i % 2])
        finally:
            api.GpuContext.set_thread_deadline(None)
    return call


def bexact(i, sim="cosine", boost=1.0):
    return lambda: sr.knn_exact_bytes_coalesced(FB, sim, qb[i % len(qb)], KS[i % 4], boost=boost)


def freq(i):
    return lambda: sr.knn_search_coalesced(FF, "cosine", np.ones(16, np.float32), KS[i % 4])


class Callers:
    def __init__(self):
        self.threads, self.told, self.mu = [], [], threading.Lock()

    def start(self, calls):
        def run(call):
            try:
                r = call()
                assert len(r.scores) == 0      # the kernels did nothing
                told = (0, "")
            except _lib.NrtGpuError as e:
                told = (e.code, str(e).split(": ", 1)[1][:60])
            except Exception as e:   # noqa: BLE001
                told = (1, repr(e)[:60])
            with self.mu:
                self.told.append(told)
        for call in calls:
            t = threading.Thread(target=run, args=(call,))
            t.start()
            self.threads.append(t)

    def returned(self):
        with self.mu:
            return len(self.told)


def wait_for(what, cond):
    t_end = time.monotonic() + 60.0
    while not cond():
        assert time.monotonic() < t_end, f"waited a minute for {what}"
        time.sleep(0.001)


def pending():
    return [ctx.debug_coalescer_pending(w) for w in range(5)]


def scenario(name, steps, before_release=None):
    """steps: (calls, pending_after (all five coalescers), returned_after)."""
    before = ctx.stats()["knn_panels"]
    ctx.debug_hold_coalescers(True)
    cs = Callers()
    try:
        for calls, want, returned in steps:
            cs.start(calls)
            wait_for(f"{name}: {want} pending, {returned} back", lambda: pending() == want and cs.returned() == returned)
        if before_release:
            before_release()
    finally:
        ctx.debug_hold_coalescers(False)
    for t in cs.threads:
        t.join()
    print("==", name, f"knn_panels=+{ctx.stats()['knn_panels'] - before}")
    for (rc, text), n in sorted(Counter(cs.told).items()):
        print(f"{n} x rc {rc} `{text}`")
    print("pending", *pending(), flush=True)


scenario("breq_32_cosine_16_l2", [([breq(i, "cosine" if i % 3 else "l2_norm") for i in range(48)], [0, 0, 0, 48, 0], 0)])
# (the leader leaves with a whole panel of 64 while held; the sixteen left behind have a leader of their own, which is held)
scenario("breq_80_is_64_then_16", [([breq(i) for i in range(80)], [0, 0, 0, 16, 0], 64)])
scenario("breq_deadline_expires_in_the_queue",
         [([breq(0)], [0, 0, 0, 1, 0], 0), ([breq(i, deadline=0.030 if i == 4 else None) for i in range(1, 12)], [0, 0, 0, 12, 0], 0)],
         before_release=lambda: time.sleep(0.100))
# requests that cannot be answered fail alone before they are queued: nothing is held, nothing was pending
scenario("breq_bad_requests_fail_alone",
         [([breq(0, query=np.ones(24, np.int8)), breq(1, query=np.zeros(DIM, np.int8)), breq(2, mask=77)], [0, 0, 0, 0, 0], 3)])
scenario("bexact_two_boosts", [([bexact(i, boost=1.0 if i % 3 else 2.0) for i in range(48)], [0, 0, 0, 0, 48], 0)])
scenario("bexact_80_is_64_then_16", [([bexact(i) for i in range(80)], [0, 0, 0, 0, 16], 64)])
scenario("float_and_byte_callers_never_share", [([freq(i) for i in range(8)] + [breq(i) for i in range(8)] + [bexact(i) for i in range(8)],
                                                 [0, 0, 8, 8, 8], 0)])
print("lone", len(breq(3)().scores), len(bexact(3)().scores), *pending())

for g in leaves:
    g.release()
ctx.close()
print("done", flush=True)
