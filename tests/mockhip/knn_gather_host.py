"""Run by tests/test_knn_gather_host.py in a subprocess with tests/mockhip preloaded and MOCKHIP_TRACE set: the HOST side of the
gather route of the filtered knn requests (nrtgpu_set_knn_gather; vectors_gather.cpp) -- the setter's argument check, the route
decision per knob and filter (which kernels a request enqueues), the default context's launches (raw trace lines, for the
comparison with tests/golden/vector_host_launch_trace.txt) and the fp16 sketch that a float field searched only on the gather
route never builds.  The kernels do nothing there: every answer is empty and the listing kernel counts no row.
One `name value` line per case on stdout."""
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from nrtsearch_amd import _lib, api   # noqa: E402

TRACE = os.environ["MOCKHIP_TRACE"]
L = _lib.load()
rng = np.random.default_rng(5)
ROWS, FF, FB = (40_000, 30_000, 100), 1, 2          # tests/mockhip/vector_launch_trace.py's leaves
M_HALF, M_HALF_PCT, M_5PCT, M_ALL = 1, 2, 3, 4
seen = 0


def say(name, value):
    print(name, value, flush=True)


def rc_of(fn):
    try:
        fn()
        return 0
    except api.NrtGpuError as e:
        return e.code


def launched(fn):
    """The trace lines of the launches fn() enqueued."""
    global seen
    fn()
    lines = open(TRACE).read().split("\n")[:-1]
    new, seen = lines[seen:], len(lines)
    return new


def kernel_names(lines):
    out = []
    for line in lines:
        m = re.match(r"_ZN6nrtgpu(\d+)", line)
        out.append(line[m.end(): m.end() + int(m.group(1))] if m else line.split()[0])
    return out


def every(n, step):
    return np.packbits((np.arange(((n + 63) // 64) * 64) % step == 0).reshape(-1, 64), axis=1, bitorder="little").view(np.uint64).reshape(-1)


def vector_leaves(ctx):
    leaves, base = [], 0
    for n in ROWS:
        g = api.GpuSegment(ctx, n, base)
        g.add_vectors(FF, rng.standard_normal((n, 64)).astype(np.float32))
        g.add_byte_vectors(FB, rng.integers(-128, 128, size=(n, 100), dtype=np.int8))
        g.set_mask(M_HALF, np.full((n + 63) // 64, 0x5555555555555555, dtype=np.uint64))
        g.set_mask(M_HALF_PCT, every(n, 200))
        g.set_mask(M_5PCT, every(n, 20))
        g.set_mask(M_ALL, every(n, 1))
        g.seal()
        leaves.append(g)
        base += n
    return leaves


# ---- the setter ----
ctx = api.GpuContext(device_id=0, max_batch=256, collect_timing=True)
say("set_minus_1", rc_of(lambda: ctx.set_knn_gather(-1)))
say("set_1001", rc_of(lambda: ctx.set_knn_gather(1001)))
say("set_null_ctx", L.nrtgpu_set_knn_gather(None, 10))
say("set_1000", rc_of(lambda: ctx.set_knn_gather(1000)))
say("set_0", rc_of(lambda: ctx.set_knn_gather(0)))

# ---- the default context: the knn requests of the recorded schedule, raw ----
leaves = vector_leaves(ctx)
sr = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics())
qf = rng.standard_normal((70, 64)).astype(np.float32)
qb = rng.integers(-128, 128, size=(70, 100), dtype=np.int8)
launched(lambda: sr.knn_exact(FF, "cosine", qf, 10))            # (the field's first exact search builds the sketch, as in the recording)


def float_request(mask=M_HALF, n=5):
    return sr.knn_search(FF, "dot_product", qf[:n], 10, 2.0, api.MaskFilter(mask), 0.25)


def byte_request(mask=M_HALF, n=5):
    return sr.knn_search_bytes(FB, "l2_norm", qb[:n], 10, 2.0, api.MaskFilter(mask), 0.25)


say("default_float", "|".join(launched(float_request)))
say("default_bytes", "|".join(launched(byte_request)))

# ---- the route per knob and filter ----
for kind, request in (("float", float_request), ("bytes", byte_request)):
    for knob in (0, 10, 1000):
        ctx.set_knn_gather(knob)
        for mname, mask in (("half_pct", M_HALF_PCT), ("5pct", M_5PCT), ("all", M_ALL)):
            before = ctx.stats()
            lines = launched(lambda: request(mask))
            after = ctx.stats()
            say(f"route_{kind}_{knob}_{mname}", ",".join(kernel_names(lines)))
            say(f"stats_{kind}_{knob}_{mname}", " ".join(f"{c}=+{after[c] - before[c]}" for c in ("knn_panels", "knn_score_launches", "knn_rows",
                                                                                                 "knn_sketch_launches", "knn_second_passes")))
ctx.set_knn_gather(1000)
say("route_float_1000_all_130_queries", ",".join(kernel_names(launched(lambda: sr.knn_search(FF, "cosine", np.tile(qf, (2, 1))[:130], 10, 1.0, api.MaskFilter(M_ALL))))))
L.nrtgpu_set_thread_deadline_ns(L.nrtgpu_monotonic_ns() - 1)
say("expired_deadline_float", rc_of(lambda: float_request(M_HALF_PCT)))
say("expired_deadline_bytes", rc_of(lambda: byte_request(M_HALF_PCT)))
L.nrtgpu_set_thread_deadline_ns(0)
say("wrong_dim", rc_of(lambda: sr.knn_search(FF, "cosine", qf[:1, :48], 10, 1.0, api.MaskFilter(M_HALF_PCT))))
say("float_entry_on_byte_field", rc_of(lambda: sr.knn_search(FB, "cosine", qf[:1], 10, 1.0, api.MaskFilter(M_HALF_PCT))))
say("byte_entry_on_float_field", rc_of(lambda: sr.knn_search_bytes(FF, "cosine", qb[:1, :64], 10, 1.0, api.MaskFilter(M_HALF_PCT))))
say("unknown_mask", rc_of(lambda: float_request(7)))
say("k_1025", rc_of(lambda: sr.knn_search(FF, "cosine", qf[:1], 1025, 1.0, api.MaskFilter(M_HALF_PCT))))
for g in leaves:
    g.release()
ctx.close()

# ---- a float field that is only ever searched on the gather route builds no sketch ----
ctx = api.GpuContext(device_id=0, max_batch=256)
n, dim = 50_000, 64
g = api.GpuSegment(ctx, n, 0)
g.add_vectors(FF, rng.standard_normal((n, dim)).astype(np.float32))
g.set_mask(M_HALF_PCT, every(n, 200))
g.seal()
sr = api.GpuIndexSearcher(ctx, [g], api.IndexStatistics())
sketch_bytes = n * dim * 2
bytes0 = g.device_bytes
launched(lambda: None)      # (the upload's own kernels)
ctx.set_knn_gather(1000)
names = kernel_names(launched(lambda: sr.knn_search(FF, "l2_norm", qf[:3], 10, 1.0, api.MaskFilter(M_HALF_PCT))))
say("gather_only_kernels", ",".join(names))
say("gather_only_growth_below_sketch", g.device_bytes - bytes0 < sketch_bytes // 8)
bytes1 = g.device_bytes
ctx.set_knn_gather(0)
names = kernel_names(launched(lambda: sr.knn_search(FF, "l2_norm", qf[:3], 10, 1.0, api.MaskFilter(M_HALF_PCT))))
say("full_pass_builds_sketch", "knn_sketch_build_kernel" in names and g.device_bytes - bytes1 >= sketch_bytes)
g.release()
ctx.close()
print("done", flush=True)
