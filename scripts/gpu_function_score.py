#!/usr/bin/env python3
"""What the function-score route costs beside the exhaustive scan it is modelled on: one process, one corpus, the same
five-term queries through both kernels, timed by HIP events (nrtgpu_config.collect_timing -> nrtgpu_stats.scan_ms).

  scan            bm25_scan_kernel through nrtgpu_search_bm25_batch in a context with NRTGPU_FLAG_NO_PRUNE, ScoreMode.COMPLETE
  function score  bm25_function_score_kernel through nrtgpu_search_function_score_batch with 4 weight functions (masks of
                  density 0.30, 0.05, 0.0005 and one without a filter)

Both stream the same posting bytes; the function-score kernel adds up to 8 mask words per 64 docs and gives up the scan's
accumulator-space pruning of candidates.  Warm-up calls first, then the two are timed in alternation.  With no functions the
new route must return the scan's answers (checked before anything is timed).  Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from nrtsearch_amd import _lib, api, synth  # noqa: E402

INT_MAX = 2**31 - 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--terms", type=int, default=5)
    ap.add_argument("--segments", type=int, default=4)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()

    qr = synth.make_queries(args.queries, args.terms)
    corpus = synth.build_corpus(args.docs, sorted(set(int(r) for r in qr.reshape(-1))), n_segments=args.segments, delete_fraction=0.01)
    ctx = api.GpuContext(0, max_batch=args.queries, collect_timing=True, flags=_lib.NRTGPU_FLAG_NO_PRUNE)
    leaves = [api.GpuSegment.from_data(ctx, s) for s in corpus.segments]
    for si, (seg, leaf) in enumerate(zip(corpus.segments, leaves)):
        for mid, density in ((7, 0.30), (9, 0.05), (11, 0.0005)):
            leaf.set_mask(mid, synth.random_mask(seg.max_doc, density, 100 * mid + si))
    sr = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics.from_corpus(corpus))
    inner = [api.BooleanQuery(tuple(api.TermQuery(0, int(t)) for t in row)) for row in qr]
    mgrs = [api.TopScoreDocCollectorManager(args.k, None, INT_MAX)] * len(inner)
    funcs = (api.WeightFunction(2.5, 7), api.WeightFunction(1.25, 0), api.WeightFunction(0.5, 9), api.WeightFunction(3.0, 11))
    fsq = [api.FunctionScoreQuery(q, funcs, "multiply", "multiply") for q in inner]
    bare = [api.FunctionScoreQuery(q) for q in inner]

    plain = sr.search_batch(inner, mgrs)
    same = sr.search_function_score_batch(bare, mgrs)
    for a, b in zip(plain, same):
        assert a.docs.tolist() == b.docs.tolist() and a.scores.view(np.uint32).tolist() == b.scores.view(np.uint32).tolist()
        assert a.total_hits == b.total_hits and not b.relation_gte

    def timed(call):
        ctx.reset_stats()
        call()
        st = ctx.stats()
        assert st["scan_launches"] == 1 and st["maxscore_launches"] == 0, st
        return st["scan_ms"], st["scan_items"], st["scan_postings"]

    for _ in range(args.warmup):
        timed(lambda: sr.search_batch(inner, mgrs))
        timed(lambda: sr.search_function_score_batch(fsq, mgrs))
    scan, func = [], []
    for _ in range(args.steps):
        scan.append(timed(lambda: sr.search_batch(inner, mgrs)))
        func.append(timed(lambda: sr.search_function_score_batch(fsq, mgrs)))
    scan_ms = float(np.median([s[0] for s in scan]))
    func_ms = float(np.median([f[0] for f in func]))
    print(json.dumps(dict(docs=args.docs, queries=args.queries, terms=args.terms, k=args.k, steps=args.steps, items=int(scan[0][1]),
                          postings=int(scan[0][2]), scan_kernel_ms=round(scan_ms, 4), function_score_kernel_ms=round(func_ms, 4),
                          ratio=round(func_ms / scan_ms, 3), scan_ms_all=[round(s[0], 4) for s in scan],
                          function_score_ms_all=[round(f[0], 4) for f in func])), flush=True)
    for leaf in leaves:
        leaf.release()
    ctx.close()


if __name__ == "__main__":
    main()
