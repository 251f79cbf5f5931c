#!/usr/bin/env python3
"""What sorting by a 64-bit column costs beside sorting by a 32-bit one, and what a mask from a 64-bit column costs beside one from
a 32-bit column: scripts/gpu_field_sort.py's corpus, batch and method -- one process, bench.py's C3 corpus (10 M docs, ten tiered
segments; the postings of one 1024-query batch of its five-term disjunctions), HIP events (nrtgpu_config.collect_timing ->
nrtgpu_stats.scan_ms / nrtgpu_last_diagnostics.device_ms).

  baseline  bm25_field_sort_kernel through nrtgpu_search_sorted_batch, ascending over a random int32 column
  sorted64  bm25_field_sort64_kernel through nrtgpu_search_sorted64_batch, descending ("newest first") over a random epoch-millis
            column spanning ten years (39 value bits beside 24 docid bits)
  ties      both routes again over a column of 100 distinct values (days, not milliseconds): ties decide every rank, many keys of a
            compaction share a high word, the select leaves its buckets for the byte radix -- the same column bytes as above, so
            the difference to the random columns is the select's share
  mask      value_mask_kernel: one range clause over the int32 column on every leaf, the kernels' times summed;
  mask64    value_mask64_kernel: "in the last 30 days" over the epoch-millis column, the same

Same build, same plan, same postings; the 64-bit route reads 8 bytes per doc where the baseline reads 4, and its packed keys
share high words where the baseline's do not (the select's radix fallback).  Counts must agree before anything is timed.  Warm-up
calls first; then the baseline is measured three times (its own spread) with the 64-bit route in between.  Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from nrtsearch_amd import api, synth, workload  # noqa: E402

COL32, COL64, TIES32, TIES64 = 7, 8, 9, 10
NOW, DAY = 1_700_000_000_000, 86_400_000
TEN_YEARS = 3653 * DAY


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=0, help="0: C3's 10 M")
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--k", type=int, default=0, help="0: C3's 1000")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    args = ap.parse_args()

    w = workload.C3
    if args.docs:
        w = workload.Workload(f"C3 shape at {args.docs} docs", args.docs, w.n_terms, w.k, w.n_queries, w.segments_per_shard, w.max_rank)
    k = args.k or w.k
    qr = synth.make_queries(w.n_queries, w.n_terms, w.max_rank)[: args.queries]
    corpus = workload.build_shard_corpus(w, qr, 1, 0)
    ctx = api.GpuContext(0, max_batch=args.queries, collect_timing=True)
    rng = np.random.default_rng(77)
    leaves = []
    for seg in corpus.segments:
        g = api.GpuSegment(ctx, seg.max_doc, seg.doc_base)
        g.add_field_norms(0, seg.norms)
        g.add_terms(0, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
        g.add_doc_values(COL32, "int", rng.integers(-2**31, 2**31, size=seg.max_doc, dtype=np.int64).astype(np.int32))
        g.add_doc_values64(COL64, "long", NOW - rng.integers(0, TEN_YEARS, size=seg.max_doc, dtype=np.int64))
        days = rng.integers(0, 100, size=seg.max_doc, dtype=np.int64)
        g.add_doc_values(TIES32, "int", days.astype(np.int32))
        g.add_doc_values64(TIES64, "long", NOW - days * DAY)
        g.seal()
        leaves.append(g)
    sr = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics.from_corpus(corpus))
    inner = workload.boolean_queries(qr)
    mgrs = [api.TopScoreDocCollectorManager(k)] * len(inner)
    sorts32 = [api.SortField(COL32, "int")] * len(inner)
    sorts64 = [api.SortField64(COL64, "long", True)] * len(inner)

    base = api.search_sorted_batch(sr, inner, mgrs, sorts32)
    new = api.search_sorted64_batch(sr, inner, mgrs, sorts64)
    for a, b in zip(base, new):
        assert (a.total_hits, a.relation_gte, len(a.docs)) == (b.total_hits, b.relation_gte, len(b.docs))
        assert np.all(np.diff(b.values) <= 0) and np.all(np.diff(a.values.astype(np.int64)) >= 0)

    def timed(call):
        ctx.reset_stats()
        call()
        st = ctx.stats()
        assert st["scan_launches"] == 1 and st["maxscore_launches"] == 0, st
        return st["scan_ms"], st["scan_items"], st["scan_postings"]

    def run_base():
        return timed(lambda: api.search_sorted_batch(sr, inner, mgrs, sorts32))

    def run_new():
        return timed(lambda: api.search_sorted64_batch(sr, inner, mgrs, sorts64))

    ties32 = [api.SortField(TIES32, "int")] * len(inner)
    ties64 = [api.SortField64(TIES64, "long", True)] * len(inner)

    def run_ties32():
        return timed(lambda: api.search_sorted_batch(sr, inner, mgrs, ties32))[0]

    def run_ties64():
        return timed(lambda: api.search_sorted64_batch(sr, inner, mgrs, ties64))[0]

    def mask32():
        return sum((leaf.set_mask_from_values(40, [api.ValueClause.range_(COL32, "int", 0, 2**30)]), api.GpuContext.last_diagnostics()["device_ms"])[1]
                   for leaf in leaves)

    def mask64():
        return sum((leaf.set_mask_from_values64(41, [api.ValueClause64.range_(COL64, "long", NOW - 30 * DAY, NOW)]),
                    api.GpuContext.last_diagnostics()["device_ms"])[1] for leaf in leaves)

    for _ in range(args.warmup):
        run_base()
        run_new()
        mask32()
        mask64()
        run_ties32()
        run_ties64()
    rounds = [[], [], []]
    new_ms, m32, m64, t32, t64 = [], [[], [], []], [], [], []
    for r in range(3):
        for _ in range(args.steps):
            rounds[r].append(run_base())
            new_ms.append(run_new()[0])
            m32[r].append(mask32())
            m64.append(mask64())
            t32.append(run_ties32())
            t64.append(run_ties64())
    base_ms = [float(np.median([s[0] for s in rd])) for rd in rounds]
    mid = float(np.median(base_ms))
    n_ms = float(np.median(new_ms))
    m32_ms = [float(np.median(x)) for x in m32]
    m32_mid, m64_ms = float(np.median(m32_ms)), float(np.median(m64))
    print(json.dumps(dict(docs=w.n_docs, queries=args.queries, terms=w.n_terms, k=k, steps=args.steps, items=int(rounds[0][0][1]),
                          postings=int(rounds[0][0][2]), sorted32_kernel_ms=[round(m, 4) for m in base_ms],
                          sorted32_spread=round((max(base_ms) - min(base_ms)) / mid, 4), sorted64_kernel_ms=round(n_ms, 4),
                          ratio=round(n_ms / mid, 4), sorted64_ms_all=[round(m, 4) for m in new_ms],
                          ties32_kernel_ms=round(float(np.median(t32)), 4), ties64_kernel_ms=round(float(np.median(t64)), 4),
                          mask32_kernel_ms=[round(m, 4) for m in m32_ms], mask32_spread=round((max(m32_ms) - min(m32_ms)) / m32_mid, 4),
                          mask64_kernel_ms=round(m64_ms, 4), mask_ratio=round(m64_ms / m32_mid, 4), mask64_ms_all=[round(m, 4) for m in m64])), flush=True)
    for leaf in leaves:
        leaf.release()
    ctx.close()


if __name__ == "__main__":
    main()
