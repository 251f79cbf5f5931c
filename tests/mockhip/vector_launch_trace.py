"""Run by tests/test_vector_launch_schedule_host.py in a subprocess with tests/mockhip preloaded and MOCKHIP_TRACE set: the launch
SCHEDULE of the vector paths' host code -- the exact searches over float and byte rows (with the sketch and without, the knn request
with a filter and a score threshold), the two-call rescorers and the fused hybrid tails -- with collect_timing on.  Prints, per
step, the deltas of the context's knn counters and the kernels the step launched (name, grid.x, block.x, dynamic shared bytes).
The kernels do nothing there, so every answer is empty, no list overflows (the `safe` schedule is the GPU suites' business) and
no float answer certifies: every float panel runs its second pass too."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from nrtsearch_amd import _lib, api, synth   # noqa: E402

TRACE = os.environ["MOCKHIP_TRACE"]
COUNTERS = ("knn_panels", "knn_score_launches", "knn_rows", "knn_sketch_launches", "knn_second_passes")
rng = np.random.default_rng(5)
ROWS, FF, FB = (40_000, 30_000, 100), 1, 2
seen = 0


def step(name, ctx, fn):
    global seen
    before = ctx.stats()
    fn()
    after = ctx.stats()
    print("==", name, " ".join(f"{c}=+{after[c] - before[c]}" for c in COUNTERS))
    lines = open(TRACE).read().split("\n")[:-1]
    print("\n".join(lines[seen:]))
    seen = len(lines)


def vector_leaves(ctx):
    leaves, base = [], 0
    for n in ROWS:
        g = api.GpuSegment(ctx, n, base)
        g.add_vectors(FF, rng.standard_normal((n, 64)).astype(np.float32))
        g.add_byte_vectors(FB, rng.integers(-128, 128, size=(n, 100), dtype=np.int8))
        g.set_mask(1, np.full((n + 63) // 64, 0x5555555555555555, dtype=np.uint64))
        g.seal()
        leaves.append(g)
        base += n
    return leaves


qf = rng.standard_normal((70, 64)).astype(np.float32)
qb = rng.integers(-128, 128, size=(70, 100), dtype=np.int8)
for name, flags in (("sketch", 0), ("no_sketch", _lib.NRTGPU_FLAG_NO_VECTOR_SKETCH)):
    ctx = api.GpuContext(device_id=0, max_batch=256, collect_timing=True, flags=flags)
    leaves = vector_leaves(ctx)
    sr = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics())
    step(f"build_{name}", ctx, lambda: None)
    step(f"knn_exact_{name}", ctx, lambda: sr.knn_exact(FF, "cosine", qf, 10))
    step(f"knn_search_{name}", ctx, lambda: sr.knn_search(FF, "dot_product", qf[:5], 10, 2.0, api.MaskFilter(1), 0.25))
    if not flags:
        step("knn_exact_bytes", ctx, lambda: sr.knn_exact_bytes(FB, "cosine", qb, 10))
        step("knn_search_bytes", ctx, lambda: sr.knn_search_bytes(FB, "l2_norm", qb[:5], 10, 2.0, api.MaskFilter(1), 0.25))
    for g in leaves:
        g.release()
    ctx.close()

# past two selections (65 536 + 15 x 65 536 rows) the nominating launches run back to back, append-only, with ONE selection behind them
ctx = api.GpuContext(device_id=0, max_batch=256, collect_timing=True)
big = api.GpuSegment(ctx, 1_100_000, 0)
big.add_vectors(FF, np.zeros((1_100_000, 16), dtype=np.float32))
big.add_byte_vectors(FB, np.zeros((1_100_000, 16), dtype=np.int8))
big.seal()
sr = api.GpuIndexSearcher(ctx, [big], api.IndexStatistics())
step("build_deferred", ctx, lambda: None)
step("knn_exact_deferred", ctx, lambda: sr.knn_exact(FF, "dot_product", qf[:3, :16], 10))
step("knn_exact_bytes_deferred", ctx, lambda: sr.knn_exact_bytes(FB, "dot_product", qb[:3, :16], 10))
big.release()
ctx.close()

# the rescorers: a text field to recall from; leaf 0: rows for every doc, leaf 1: a sparse ord -> doc map, leaf 2: no vectors
ctx = api.GpuContext(device_id=0, max_batch=256, collect_timing=True)
corpus = synth.build_corpus(6000, [2, 9, 70], n_segments=3)
leaves, maps = [], []
for si, seg in enumerate(corpus.segments):
    g = api.GpuSegment(ctx, seg.max_doc, seg.doc_base)
    g.add_field_norms(0, seg.norms)
    g.add_terms(0, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
    have = None if si == 0 else np.flatnonzero(rng.random(seg.max_doc) < 0.5).astype(np.int32)
    maps.append(have)
    n = seg.max_doc if have is None else len(have)
    if si < 2:
        g.add_vectors(FF, rng.standard_normal((n, 100)).astype(np.float32), have)
        g.add_byte_vectors(FB, rng.integers(-128, 128, size=(n, 100), dtype=np.int8), have)
    g.seal()
    leaves.append(g)
sr = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics.from_corpus(corpus))
step("build_rescorers", ctx, lambda: None)
# hits in all three leaves: two dense rows of leaf 0; of leaf 1 four docs the sparse map holds and one it does not; two docs of leaf 2
b1, b2 = corpus.segments[1].doc_base, corpus.segments[2].doc_base
no_row = int(np.setdiff1d(np.arange(corpus.segments[1].max_doc), maps[1])[2])
docs = np.array([1, b1 + maps[1][0], b2 + 10, 7, b1 + maps[1][3], b1 + maps[1][40], b1 + no_row, b1 + maps[1][-1], b2 + 11], dtype=np.int32)
assert sorted(int(np.searchsorted([b1, b2], d, side="right")) for d in docs) == [0, 0, 1, 1, 1, 1, 1, 2, 2]
first = api.TopDocs(docs, np.linspace(1.0, 0.1, len(docs)).astype(np.float32), len(docs), False)
step("rescore_vectors", ctx, lambda: sr.rescore_vectors(first, FF, "cosine", rng.standard_normal(100).astype(np.float32), 5, 1.0, 2.0))
step("rescore_byte_vectors", ctx, lambda: sr.rescore_byte_vectors(first, FB, "cosine", rng.integers(-128, 128, size=100, dtype=np.int8), 5, 1.0, 2.0))
qs = [api.BooleanQuery(tuple(api.TermQuery(0, t) for t in ((2, 70) if i % 2 else (9,)))) for i in range(130)]
mg = [api.TopScoreDocCollectorManager(300)] * 130
step("search_hybrid_batch", ctx, lambda: sr.search_hybrid_batch(qs, mg, FF, "cosine", rng.standard_normal((130, 100)).astype(np.float32), 50, 1.0, 2.0))
step("search_hybrid_bytes_batch", ctx,
     lambda: sr.search_hybrid_bytes_batch(qs, mg, FB, "cosine", rng.integers(-128, 128, size=(130, 100), dtype=np.int8), 50, 1.0, 2.0))
for g in leaves:
    g.release()
ctx.close()
print("done", flush=True)
