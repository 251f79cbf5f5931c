#!/usr/bin/env python3
"""What the sorted-search route costs beside the final-score route it is modelled on: one process, bench.py's C3 corpus (10 M
docs, ten tiered segments; the postings of one 1024-query batch of its five-term disjunctions), a random int column on every
leaf, and the same batch through both kernels, timed by HIP events (nrtgpu_config.collect_timing -> nrtgpu_stats.scan_ms).

  baseline  bm25_function_score_kernel through nrtgpu_search_function_score_batch with zero functions
  sorted    bm25_field_sort_kernel through nrtgpu_search_sorted_batch, ascending over the column

Same build, same plan (the exhaustive plan of the same disjunctions), same postings; the sorted route adds one 4-byte code per
doc and drops the BM25 arithmetic.  The counts of the two must agree (checked before anything is timed).  Warm-up calls first;
then the baseline is measured three times (its own spread) with the sorted route in between.  Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from nrtsearch_amd import api, synth, workload  # noqa: E402

COL = 7


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
        g.add_doc_values(COL, "int", rng.integers(-2**31, 2**31, size=seg.max_doc, dtype=np.int64).astype(np.int32))
        g.seal()
        leaves.append(g)
    sr = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics.from_corpus(corpus))
    inner = workload.boolean_queries(qr)
    mgrs = [api.TopScoreDocCollectorManager(k)] * len(inner)
    bare = [api.FunctionScoreQuery(q) for q in inner]
    sorts = [api.SortField(COL, "int")] * len(inner)

    base = sr.search_function_score_batch(bare, mgrs)
    srt = api.search_sorted_batch(sr, inner, mgrs, sorts)
    for a, b in zip(base, srt):
        assert (a.total_hits, a.relation_gte, len(a.docs)) == (b.total_hits, b.relation_gte, len(b.docs))
        assert np.all(np.diff(b.values.astype(np.int64)) >= 0)

    def timed(call):
        ctx.reset_stats()
        call()
        st = ctx.stats()
        assert st["scan_launches"] == 1 and st["maxscore_launches"] == 0, st
        return st["scan_ms"], st["scan_items"], st["scan_postings"]

    def run_base():
        return timed(lambda: sr.search_function_score_batch(bare, mgrs))

    def run_sorted():
        return timed(lambda: api.search_sorted_batch(sr, inner, mgrs, sorts))

    for _ in range(args.warmup):
        run_base()
        run_sorted()
    rounds = [[], [], []]
    sorted_ms = []
    for r in range(3):
        for _ in range(args.steps):
            rounds[r].append(run_base())
            sorted_ms.append(run_sorted()[0])
    base_ms = [float(np.median([s[0] for s in rd])) for rd in rounds]
    mid = float(np.median(base_ms))
    srt_ms = float(np.median(sorted_ms))
    print(json.dumps(dict(docs=w.n_docs, queries=args.queries, terms=w.n_terms, k=k, steps=args.steps, items=int(rounds[0][0][1]),
                          postings=int(rounds[0][0][2]), function_score_kernel_ms=[round(m, 4) for m in base_ms],
                          function_score_spread=round((max(base_ms) - min(base_ms)) / mid, 4), sorted_kernel_ms=round(srt_ms, 4),
                          ratio=round(srt_ms / mid, 4), sorted_ms_all=[round(m, 4) for m in sorted_ms])), flush=True)
    for leaf in leaves:
        leaf.release()
    ctx.close()


if __name__ == "__main__":
    main()
