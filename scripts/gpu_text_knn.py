#!/usr/bin/env python3
"""What knn clauses beside a text query cost: one process, the corpus and the five-term queries of scripts/gpu_function_score.py,
timed by HIP events (nrtgpu_config.collect_timing -> nrtgpu_stats.scan_ms).

  yardstick   bm25_function_score_kernel through nrtgpu_search_function_score_batch with zero functions
  no lists    bm25_text_knn_kernel through nrtgpu_search_text_knn_batch with n_lists = 0
  one list    the same with one list of --list-docs docs per query (docs drawn over the whole index, scores in (0, 1])

The three stream the same posting bytes; the new kernel adds, per sub-tile of a part that has entries, one 256-byte load of the
next 64 listed docids (issued beside the clause-range lookup) and, per listed doc, one LDS read-modify-write.  Warm-up calls first,
then the three are timed in alternation.  With no lists the new entry must return the yardstick's answers (checked before anything
is timed).  Prints one JSON line and, with --out, writes it to a file."""
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
    ap.add_argument("--list-docs", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    qr = synth.make_queries(args.queries, args.terms)
    corpus = synth.build_corpus(args.docs, sorted(set(int(r) for r in qr.reshape(-1))), n_segments=args.segments, delete_fraction=0.01)
    ctx = api.GpuContext(0, max_batch=args.queries, collect_timing=True, flags=_lib.NRTGPU_FLAG_NO_PRUNE)
    leaves = [api.GpuSegment.from_data(ctx, s) for s in corpus.segments]
    sr = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics.from_corpus(corpus))
    inner = [api.BooleanQuery(tuple(api.TermQuery(0, int(t)) for t in row)) for row in qr]
    mgrs = [api.TopScoreDocCollectorManager(args.k, None, INT_MAX)] * len(inner)
    bare = [api.FunctionScoreQuery(q) for q in inner]
    rng = np.random.Generator(np.random.PCG64(2024))
    none = [[] for _ in inner]
    one = [[api.KnnClause(np.sort(rng.choice(args.docs, size=args.list_docs, replace=False)).astype(np.int32),
                          (1.0 - rng.random(args.list_docs)).astype(np.float32), 1.0)] for _ in inner]

    a = sr.search_function_score_batch(bare, mgrs)
    b = sr.search_text_knn_batch(inner, none, mgrs)
    for x, y in zip(a, b):
        assert x.docs.tolist() == y.docs.tolist() and x.scores.view(np.uint32).tolist() == y.scores.view(np.uint32).tolist()
        assert x.total_hits == y.total_hits and x.relation_gte == y.relation_gte

    def timed(call):
        ctx.reset_stats()
        call()
        st = ctx.stats()
        assert st["scan_launches"] == 1 and st["maxscore_launches"] == 0, st
        return st["scan_ms"], st["scan_items"], st["scan_postings"]

    runs = {"yardstick": lambda: sr.search_function_score_batch(bare, mgrs), "no_lists": lambda: sr.search_text_knn_batch(inner, none, mgrs),
            "one_list": lambda: sr.search_text_knn_batch(inner, one, mgrs)}
    for _ in range(args.warmup):
        for call in runs.values():
            timed(call)
    ms = {name: [] for name in runs}
    items = postings = 0
    for _ in range(args.steps):
        for name, call in runs.items():
            t, items, postings = timed(call)
            ms[name].append(t)
    med = {name: float(np.median(v)) for name, v in ms.items()}
    res = dict(docs=args.docs, queries=args.queries, terms=args.terms, k=args.k, list_docs=args.list_docs, steps=args.steps, items=int(items),
               postings=int(postings), yardstick_kernel_ms=round(med["yardstick"], 4), no_lists_kernel_ms=round(med["no_lists"], 4),
               one_list_kernel_ms=round(med["one_list"], 4),
               yardstick_spread_ms=[round(float(min(ms["yardstick"])), 4), round(float(max(ms["yardstick"])), 4)],
               no_lists_ratio=round(med["no_lists"] / med["yardstick"], 4), one_list_ratio=round(med["one_list"] / med["yardstick"], 4),
               yardstick_ms_all=[round(v, 4) for v in ms["yardstick"]], no_lists_ms_all=[round(v, 4) for v in ms["no_lists"]],
               one_list_ms_all=[round(v, 4) for v in ms["one_list"]])
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    for leaf in leaves:
        leaf.release()
    ctx.close()


if __name__ == "__main__":
    main()
