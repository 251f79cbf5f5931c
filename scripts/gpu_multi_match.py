#!/usr/bin/env python3
"""What the multi-match route costs beside the two exhaustive kernels it is modelled on: one process, one two-field corpus, the
same six clauses per query (3 tokens x 2 fields) through four calls, timed by HIP events (nrtgpu_config.collect_timing ->
nrtgpu_stats.scan_ms).

  scan            the clauses as ONE flat disjunction: bm25_scan_kernel through nrtgpu_search_bm25_batch (NRTGPU_FLAG_NO_PRUNE)
  function score  the same flat disjunction: bm25_function_score_kernel through nrtgpu_search_function_score_batch, no functions
  cross_fields    3 groups (tokens) x 2 fields, SHOULD groups, tie breaker 0.3: bm25_multi_match_kernel
  best_fields     2 groups (fields) x 3 tokens, SHOULD clauses, tie breaker 0.3: bm25_multi_match_kernel

All four stream the same posting bytes under ScoreMode.COMPLETE.  Warm-up calls first, then the four are timed in alternation.
Before anything is timed: one clause per group must return the flat disjunction's answers.  Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from nrtsearch_amd import _lib, api, synth  # noqa: E402

INT_MAX = 2**31 - 1
FIELD_SEEDS = (1234, 777)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--tokens", type=int, default=3)
    ap.add_argument("--segments", type=int, default=4)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()

    qr = synth.make_queries(args.queries, args.tokens)
    ranks = sorted(set(int(r) for r in qr.reshape(-1)))
    fields = [synth.build_corpus(args.docs, ranks, n_segments=args.segments, delete_fraction=0.01, seed=s) for s in FIELD_SEEDS]
    ctx = api.GpuContext(0, max_batch=args.queries, collect_timing=True, flags=_lib.NRTGPU_FLAG_NO_PRUNE)
    leaves = []
    for si, seg0 in enumerate(fields[0].segments):
        leaf = api.GpuSegment(ctx, seg0.max_doc, seg0.doc_base)
        for fi, corpus in enumerate(fields):
            s = corpus.segments[si]
            leaf.add_field_norms(fi, s.norms)
            leaf.add_terms(fi, s.term_ids, s.offsets, s.docids, s.freqs)
        leaf.seal()
        leaf.set_live_docs(seg0.live_bits)
        leaves.append(leaf)
    stats = api.IndexStatistics()
    for fi, corpus in enumerate(fields):
        stats.fields[fi] = api.CollectionStatistics(corpus.doc_count, corpus.sum_total_term_freq)
        for t, df in corpus.doc_freq.items():
            stats.doc_freq[(fi, int(t))] = int(df)
    sr = api.GpuIndexSearcher(ctx, leaves, stats)
    nf = len(fields)
    tq = lambda f, t: api.TermQuery(f, int(t))   # noqa: E731
    flat = [api.BooleanQuery(tuple(tq(f, t) for t in row for f in range(nf))) for row in qr]
    bare = [api.FunctionScoreQuery(q) for q in flat]
    cross = [api.MultiMatchQuery("cross_fields", tuple(tuple(tq(f, t) for f in range(nf)) for t in row), "should", 0, 0.3) for row in qr]
    best = [api.MultiMatchQuery("best_fields", tuple(tuple(tq(f, t) for t in row) for f in range(nf)), "should", 0, 0.3) for row in qr]
    singles = [api.MultiMatchQuery("cross_fields", tuple((tq(f, t),) for t in row[:2] for f in range(nf)), "should", 0, 0.3) for row in qr]
    mgrs = [api.TopScoreDocCollectorManager(args.k, None, INT_MAX)] * len(flat)

    plain = sr.search_batch([api.BooleanQuery(tuple(tq(f, t) for t in row[:2] for f in range(nf))) for row in qr], mgrs)
    same = sr.search_multi_match_batch(singles, mgrs)
    for a, b in zip(plain, same):
        assert a.docs.tolist() == b.docs.tolist() and a.scores.view(np.uint32).tolist() == b.scores.view(np.uint32).tolist()
        assert a.total_hits == b.total_hits and not b.relation_gte

    def timed(call):
        ctx.reset_stats()
        call()
        st = ctx.stats()
        assert st["scan_launches"] == 1 and st["maxscore_launches"] == 0, st
        return st["scan_ms"], st["scan_items"], st["scan_postings"]

    calls = {"scan": lambda: sr.search_batch(flat, mgrs), "function_score": lambda: sr.search_function_score_batch(bare, mgrs),
             "cross_fields": lambda: sr.search_multi_match_batch(cross, mgrs), "best_fields": lambda: sr.search_multi_match_batch(best, mgrs)}
    for _ in range(args.warmup):
        for call in calls.values():
            timed(call)
    runs = {name: [] for name in calls}
    for _ in range(args.steps):
        for name, call in calls.items():
            runs[name].append(timed(call))
    med = {name: float(np.median([r[0] for r in rs])) for name, rs in runs.items()}
    out = dict(docs=args.docs, queries=args.queries, tokens=args.tokens, fields=nf, k=args.k, steps=args.steps,
               items=int(runs["cross_fields"][0][1]), postings=int(runs["cross_fields"][0][2]))
    for name in calls:
        out[name + "_kernel_ms"] = round(med[name], 4)
    for name in ("cross_fields", "best_fields"):
        out[name + "_over_scan"] = round(med[name] / med["scan"], 3)
        out[name + "_over_function_score"] = round(med[name] / med["function_score"], 3)
    for name, rs in runs.items():
        out[name + "_ms_all"] = [round(r[0], 4) for r in rs]
    print(json.dumps(out), flush=True)
    for leaf in leaves:
        leaf.release()
    ctx.close()


if __name__ == "__main__":
    main()
