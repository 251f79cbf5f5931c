#!/usr/bin/env python3
"""What a filter mask built on the device from doc value columns costs (nrtgpu_segment_set_mask_from_values: valuemask.hip)
beside what it replaces: NumPy building the same words from the host copy of the column, then nrtgpu_segment_set_mask.

One process.  The leaves are bench.py's C3 index (10 M docs, ten tiered segments) with columns only -- the builder reads no
posting: `rating` a dense int column in 0..99, `price` a float column on 90 % of the docs, `tags` a multi-valued int column
(0..3 values per doc out of 1000).  A measurement is ONE mask for the whole index: the call on each of the ten leaves, summed.

  range_dense     rating in [40, 99]                     exists_sparse   price has a value
  in_set_dense    rating in a set of 64 values           in_set_multi    some tag in a set of 64 values
  range_multi     some tag in [100, 299]                 in_set_4096     rating in a set of 4096 values (100 of them occur)

Before anything is timed the device's words are compared with NumPy's on every leaf.  Then `--warmup` calls, then `--steps` timed
ones per line and side, the sides alternating; the median.  device_ms: the call's wall time; kernel_ms: the kernel's own time by
HIP events (nrtgpu_config.collect_timing -> nrtgpu_last_diagnostics); host_build_ms / host_set_ms: NumPy's words and their
registration.  Every step runs under a time limit of its own.  Prints one JSON line."""
import argparse
import json
import os
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from nrtsearch_amd import api, workload  # noqa: E402

RATING, PRICE, TAGS = 7, 8, 9
MASK = 40


class step:
    """a time limit for one step of the script"""

    def __init__(self, name, seconds):
        self.name, self.seconds = name, seconds

    def __enter__(self):
        def late(signum, frame):
            raise TimeoutError(f"step {self.name!r} ran longer than {self.seconds} s")
        signal.signal(signal.SIGALRM, late)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        return False


def pack(ok: np.ndarray) -> np.ndarray:
    padded = np.zeros(((len(ok) + 63) // 64) * 64, dtype=bool)
    padded[: len(ok)] = ok
    return np.packbits(padded.reshape(-1, 64), axis=1, bitorder="little").view(np.uint64).reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=0, help="0: C3's 10 M")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    w = workload.C3
    if args.docs:
        w = workload.Workload(f"C3 shape at {args.docs} docs", args.docs, w.n_terms, w.k, w.n_queries, w.segments_per_shard, w.max_rank)
    _, _, sizes = workload.shard_leaves(w, 1, 0)

    with step("upload", 240):
        ctx = api.GpuContext(0, max_batch=16, collect_timing=True)
        rng = np.random.default_rng(77)
        leaves, host = [], []
        base = 0
        for n in sizes:
            rating = rng.integers(0, 100, size=n).astype(np.int32)
            price_docs = np.nonzero(rng.random(n) < 0.9)[0].astype(np.int32)
            price = rng.random(len(price_docs)).astype(np.float32)
            tag_docs = np.repeat(np.arange(n, dtype=np.int32), rng.integers(0, 4, size=n))
            tags = rng.integers(0, 1000, size=len(tag_docs)).astype(np.int32)
            g = api.GpuSegment(ctx, n, base)
            g.add_doc_values(RATING, "int", rating)
            g.add_doc_values(PRICE, "float", price, price_docs)
            g.add_doc_values_multi(TAGS, "int", tags, tag_docs)
            g.seal()
            leaves.append(g)
            host.append(dict(n=n, rating=rating, price_docs=price_docs, tag_docs=tag_docs, tags=tags))
            base += n

    set64 = np.arange(3, 3 + 64 * 15, 15, dtype=np.int32)            # 64 values out of 0..999 (7 of them below 100)
    set4096 = np.arange(-1998, 2098, dtype=np.int32)                  # 4096 values; 0..99 occur
    VC = api.ValueClause

    def any_value(h, keep_value):
        keep = np.zeros(h["n"], dtype=bool)
        keep[h["tag_docs"][keep_value]] = True
        return keep

    lines = {
        "range_dense": ([VC.range_(RATING, "int", 40, 99)], lambda h: (h["rating"] >= 40) & (h["rating"] <= 99)),
        "exists_sparse": ([VC.exists(PRICE)], lambda h: any_docs(h["n"], h["price_docs"])),
        "in_set_dense": ([VC.in_set(RATING, "int", set64)], lambda h: np.isin(h["rating"], set64)),
        "in_set_multi": ([VC.in_set(TAGS, "int", set64)], lambda h: any_value(h, np.isin(h["tags"], set64))),
        "range_multi": ([VC.range_(TAGS, "int", 100, 299)], lambda h: any_value(h, (h["tags"] >= 100) & (h["tags"] <= 299))),
        "in_set_4096": ([VC.in_set(RATING, "int", set4096)], lambda h: np.isin(h["rating"], set4096)),
    }

    def any_docs(n, docs):
        keep = np.zeros(n, dtype=bool)
        keep[docs] = True
        return keep

    def device(clauses):
        t0, kernel, count = time.perf_counter(), 0.0, 0
        for g in leaves:
            count += g.set_mask_from_values(MASK, clauses)
            kernel += api.GpuContext.last_diagnostics()["device_ms"]
        return (time.perf_counter() - t0) * 1e3, kernel, count

    def on_host(build):
        t0 = time.perf_counter()
        words = [pack(build(h)) for h in host]
        t1 = time.perf_counter()
        for g, wds in zip(leaves, words):
            g.set_mask(MASK + 1, wds)
        return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3

    out = dict(docs=int(sum(sizes)), leaves=len(sizes), warmup=args.warmup, steps=args.steps, lines={})
    with step("compare", 240):
        counts = {}
        for name, (clauses, build) in lines.items():
            _, _, counts[name] = device(clauses)
            for g, h in zip(leaves, host):
                assert np.array_equal(g.get_mask(MASK), pack(build(h))), name
    for name, (clauses, build) in lines.items():
        with step(name, 300):
            for _ in range(args.warmup):
                device(clauses)
                on_host(build)
            dev, ker, hb, hs = [], [], [], []
            for _ in range(args.steps):
                d, k, _ = device(clauses)
                b, s = on_host(build)
                dev.append(d)
                ker.append(k)
                hb.append(b)
                hs.append(s)
            med = lambda v: round(float(np.median(v)), 4)   # noqa: E731
            out["lines"][name] = dict(mask_docs=int(counts[name]), device_ms=med(dev), kernel_ms=med(ker), host_build_ms=med(hb), host_set_ms=med(hs),
                                      host_ms=med(np.array(hb) + np.array(hs)), device_min_ms=round(min(dev), 4), device_max_ms=round(max(dev), 4),
                                      ratio=round(float(np.median(dev)) / float(np.median(np.array(hb) + np.array(hs))), 4))
    print(json.dumps(out), flush=True)
    for g in leaves:
        g.release()
    ctx.close()


if __name__ == "__main__":
    main()
