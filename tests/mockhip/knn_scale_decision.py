"""Run by tests/test_knn_adversarial_host.py in a subprocess with tests/mockhip preloaded (kernels do nothing): WHERE a panel of the
exact float vector search nominates from -- the fp16 sketch or the fp32 rows -- as knn_impl decides it from the queries' largest
|element| (host_math.h: knn_sketch_scale).  The field's side of the decision needs the rows' largest |element|, which a kernel
computes: the test pins that through nrtgpu_debug_knn_bounds.  One JSON line per panel: the deltas of the context's counters."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from nrtsearch_amd import api   # noqa: E402

rng = np.random.default_rng(3)
dim, n = 64, 100
ctx = api.GpuContext(device_id=0, max_batch=64, collect_timing=True)   # (timing on: the launches are counted)
g = api.GpuSegment(ctx, n, 0)
g.add_vectors(0, rng.standard_normal((n, dim)).astype(np.float32))
g.seal()
sr = api.GpuIndexSearcher(ctx, [g], api.IndexStatistics())
ordinary = rng.standard_normal((2, dim)).astype(np.float32)
peak = np.abs(ordinary).max(axis=1, keepdims=True)
tiny = (ordinary * np.float32(2.0 ** -120) / peak).astype(np.float32)      # every query's largest |element| is 2^-120
edge = (ordinary * np.float32(2.0 ** -113) / peak).astype(np.float32)      # 2^-113: the smallest that still scales
assert np.abs(tiny).max(axis=1).tolist() == [2.0 ** -120] * 2 and np.abs(edge).max(axis=1).tolist() == [2.0 ** -113] * 2
inf = ordinary.copy()
inf[0, 5] = np.inf
for name, q in (("ordinary", ordinary), ("tiny", tiny), ("tiny_next_to_ordinary", np.stack([ordinary[0], tiny[1]])), ("edge", edge),
                ("zero", np.zeros((1, dim), np.float32)), ("inf", inf)):
    for sim in ("cosine", "dot_product", "l2_norm", "max_inner_product"):
        before = ctx.stats()
        sr.knn_exact(0, sim, q, 10)
        after = ctx.stats()
        print("PANEL " + json.dumps({"name": name, "sim": sim, "sketch": after["knn_sketch_launches"] - before["knn_sketch_launches"],
                                     "launches": after["knn_score_launches"] - before["knn_score_launches"]}), flush=True)
g.release()
ctx.close()
print("done", flush=True)
