#!/usr/bin/env python3
"""Exact search over a byte (int8) vector field against the float search over the same values, config C4's shape: N x 768 rows
(default 10 M), 64 queries per call, cosine, k = 100, 5 warm-up + 20 timed calls each, one process, collect_timing on.

    python scripts/gpu_knn_bytes.py [--rows N] [--out profiles/knn_bytes_10M.json]

The byte rows are rng.integers(-128, 128) in segments of 2.5 M; the float field holds the same values as fp32 (with its fp16
sketch: 46 GB resident at 10 M).  If the float field does not fit (host or device memory), both are measured over the first
4 M rows instead and the record says so.  Acceptance (the bar is bytes alone: the byte pass streams half of what the fp16 sketch
pass streams and has no rescoring stage behind it): a byte call takes no longer than the float call of the same rows."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np   # noqa: E402

from nrtsearch_amd import api, build   # noqa: E402

DIM, NQ, K, WARM, TIMED, SEG = 768, 64, 100, 5, 20, 2_500_000


def segments(n, seed=777):
    rng = np.random.default_rng(seed)
    base = 0
    while base < n:
        rows = min(SEG, n - base)
        yield base, rng.integers(-128, 128, size=(rows, DIM), dtype=np.int8)
        base += rows


def upload(ctx, n, as_float):
    leaves = []
    try:
        for base, rows in segments(n):
            g = api.GpuSegment(ctx, len(rows), base)
            leaves.append(g)
            if as_float:
                g.add_vectors(0, rows.astype(np.float32))
            else:
                g.add_byte_vectors(0, rows)
            g.seal()
    except (MemoryError, api.NrtGpuError):
        for g in leaves:
            g.release()
        raise
    return leaves


def timed(ctx, call):
    for _ in range(WARM):
        call()
    before = ctx.stats()
    t0 = time.perf_counter()
    for _ in range(TIMED):
        got = call()
    ms = (time.perf_counter() - t0) / TIMED * 1e3
    after = ctx.stats()
    d = {k: after[k] - before[k] for k in ("knn_panels", "knn_score_launches", "knn_score_ms", "knn_rows", "knn_second_passes", "knn_sketch_launches")}
    return ms, d, got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_bytes_10M.json"))
    a = ap.parse_args()
    ctx = api.GpuContext(0, 64, collect_timing=True)
    queries = np.random.default_rng(778).integers(-128, 128, size=(NQ, DIM), dtype=np.int8)
    n, float_note, fleaves = a.rows, "the float field holds the same rows", None
    t0 = time.time()
    try:
        fleaves = upload(ctx, n, True)
    except (MemoryError, api.NrtGpuError) as e:
        n = min(n, 4_000_000)
        float_note = f"the float field did not fit at {a.rows} rows ({type(e).__name__}): both fields hold the first {n} rows"
        fleaves = upload(ctx, n, True)
    fsr = api.GpuIndexSearcher(ctx, fleaves, api.IndexStatistics())
    qf = queries.astype(np.float32)
    f_ms, f_d, f_got = timed(ctx, lambda: fsr.knn_exact(0, "cosine", qf, K))
    print(json.dumps({"event": "float", "rows": n, "ms_per_call": round(f_ms, 3), "upload_s": round(time.time() - t0, 1)}), flush=True)
    t0 = time.time()
    bleaves = upload(ctx, n, False)
    bsr = api.GpuIndexSearcher(ctx, bleaves, api.IndexStatistics())
    b_ms, b_d, b_got = timed(ctx, lambda: bsr.knn_exact_bytes(0, "cosine", queries, K))
    print(json.dumps({"event": "bytes", "rows": n, "ms_per_call": round(b_ms, 3), "upload_s": round(time.time() - t0, 1)}), flush=True)
    steps = (DIM + 63) // 64
    streamed = n * steps * 64 + 4 * n
    b_kernel = b_d["knn_score_ms"] / TIMED
    f_kernel = f_d["knn_score_ms"] / TIMED
    # the float search returns the oracle's bits for fp32 sums in ITS order: at 768 dimensions those are not integers below 2^24
    # any more, so the two answers may differ in the last bit of a score; what is recorded is how many docids they share
    same_docs = sum(len(set(x.docs.tolist()) & set(y.docs.tolist())) for x, y in zip(b_got, f_got))
    rec = {
        "what": "nrtgpu_knn_exact_bytes against nrtgpu_knn_exact over the same values, one process, one GPU",
        "rows": n, "dim": DIM, "queries_per_call": NQ, "k": K, "similarity": "cosine", "warmup_calls": WARM, "timed_calls": TIMED,
        "segments": len(bleaves), "note": float_note, "build_id": build.build_id(),
        "bytes": {"ms_per_call": round(b_ms, 3), "pass_kernel_ms_per_call": round(b_kernel, 3),
                  "launches_per_call": b_d["knn_score_launches"] / TIMED, "bytes_streamed_per_call": streamed,
                  "TBps_kernel": round(streamed / (b_kernel * 1e-3) / 1e12, 3) if b_kernel > 0 else None,
                  "TBps_call": round(streamed / (b_ms * 1e-3) / 1e12, 3), "second_passes": b_d["knn_second_passes"]},
        "float": {"ms_per_call": round(f_ms, 3), "nomination_kernel_ms_per_call": round(f_kernel, 3),
                  "sketch_launches_per_call": f_d["knn_sketch_launches"] / TIMED, "second_passes": f_d["knn_second_passes"],
                  "TBps_kernel": round(n * DIM * 2 / (f_kernel * 1e-3) / 1e12, 3) if f_kernel > 0 else None},
        "bytes_over_float": round(b_ms / f_ms, 3), "accepted": bool(b_ms <= f_ms),
        "top_docs_shared_with_float_search": f"{same_docs} of {NQ * K}",
        "stream_ceiling_TBps": 6.3,
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec), flush=True)
    for g in bleaves + fleaves:
        g.release()
    ctx.close()
    return 0 if rec["accepted"] else 1


if __name__ == "__main__":
    sys.exit(main())
