#!/usr/bin/env python3
"""What a function score over a multi-match query costs beside the multi-match kernel it shares its body with: one process, one
two-field corpus, the same six clauses per query (3 tokens x 2 fields), both shapes (cross_fields: 3 groups x 2 fields, best_fields:
2 groups x 3 tokens; SHOULD, tie breaker 0.3), timed by HIP events (nrtgpu_config.collect_timing -> nrtgpu_stats.scan_ms).

  multi_match     bm25_multi_match_kernel through nrtgpu_search_multi_match_batch: THE YARDSTICK
  functions_0     bm25_multi_match_function_score_kernel through nrtgpu_search_function_score_multi_match_batch, no functions:
                  the same work as the yardstick
  functions_3     ... with 3 weight functions (two resident masks, 40 % and 10 % of the docs, and one without a filter)
  functions_8     ... with 8

All stream the same posting bytes under ScoreMode.COMPLETE.  Warm-up calls first, then the versions are timed in alternation.
The bar: the median of functions_0 may exceed the yardstick's median by no more than the spread (max - min) of the yardstick's
own runs in this process.  The times with functions get no bar; they are recorded with their ratio to functions_0.
Before anything is timed: without functions the new entry must return the multi-match entry's answers.
Prints one JSON line; --out writes it to a file as well."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from nrtsearch_amd import api, build, synth  # noqa: E402

INT_MAX = 2**31 - 1
FIELD_SEEDS = (1234, 777)
MASKS = ((7, 0.4), (9, 0.1))
THREE = ((7, 1.5), (9, 3.0), (0, 0.5))
EIGHT = ((7, 1.5), (9, 3.0), (0, 0.5), (7, 2.0), (9, 0.75), (0, 1.25), (7, 0.3), (9, 7.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--tokens", type=int, default=3)
    ap.add_argument("--segments", type=int, default=4)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    qr = synth.make_queries(args.queries, args.tokens)
    ranks = sorted(set(int(r) for r in qr.reshape(-1)))
    fields = [synth.build_corpus(args.docs, ranks, n_segments=args.segments, delete_fraction=0.01, seed=s) for s in FIELD_SEEDS]
    ctx = api.GpuContext(0, max_batch=args.queries, collect_timing=True)
    leaves = []
    for si, seg0 in enumerate(fields[0].segments):
        leaf = api.GpuSegment(ctx, seg0.max_doc, seg0.doc_base)
        for fi, corpus in enumerate(fields):
            s = corpus.segments[si]
            leaf.add_field_norms(fi, s.norms)
            leaf.add_terms(fi, s.term_ids, s.offsets, s.docids, s.freqs)
        leaf.seal()
        leaf.set_live_docs(seg0.live_bits)
        for mid, dens in MASKS:
            leaf.set_mask(mid, synth.random_mask(seg0.max_doc, dens, 10 * mid + si))
        leaves.append(leaf)
    stats = api.IndexStatistics()
    for fi, corpus in enumerate(fields):
        stats.fields[fi] = api.CollectionStatistics(corpus.doc_count, corpus.sum_total_term_freq)
        for t, df in corpus.doc_freq.items():
            stats.doc_freq[(fi, int(t))] = int(df)
    sr = api.GpuIndexSearcher(ctx, leaves, stats)
    nf = len(fields)
    tq = lambda f, t: api.TermQuery(f, int(t))   # noqa: E731
    inner = {"cross_fields": [api.MultiMatchQuery("cross_fields", tuple(tuple(tq(f, t) for f in range(nf)) for t in row), "should", 0, 0.3) for row in qr],
             "best_fields": [api.MultiMatchQuery("best_fields", tuple(tuple(tq(f, t) for t in row) for f in range(nf)), "should", 0, 0.3) for row in qr]}
    mgrs = [api.TopScoreDocCollectorManager(args.k, None, INT_MAX)] * len(qr)

    def wrapped(shape, functions):
        return [api.FunctionScoreQuery(q, tuple(api.WeightFunction(w, m) for m, w in functions)) for q in inner[shape]]

    calls = {}
    for shape in inner:
        plain = sr.search_multi_match_batch(inner[shape], mgrs)
        bare = sr.search_function_score_multi_match_batch(wrapped(shape, ()), mgrs)
        for a, b in zip(plain, bare):
            assert a.docs.tolist() == b.docs.tolist() and a.scores.view(np.uint32).tolist() == b.scores.view(np.uint32).tolist()
            assert a.total_hits == b.total_hits and a.relation_gte == b.relation_gte
        calls[shape + "/multi_match"] = (lambda qs: lambda: sr.search_multi_match_batch(qs, mgrs))(inner[shape])
        for name, functions in (("functions_0", ()), ("functions_3", THREE), ("functions_8", EIGHT)):
            calls[shape + "/" + name] = (lambda qs: lambda: sr.search_function_score_multi_match_batch(qs, mgrs))(wrapped(shape, functions))

    def timed(call):
        ctx.reset_stats()
        call()
        st = ctx.stats()
        assert st["scan_launches"] == 1 and st["maxscore_launches"] == 0, st
        return st["scan_ms"], st["scan_items"], st["scan_postings"]

    for _ in range(args.warmup):
        for call in calls.values():
            timed(call)
    runs = {name: [] for name in calls}
    for _ in range(args.steps):
        for name, call in calls.items():
            runs[name].append(timed(call))
    out = dict(docs=args.docs, queries=args.queries, tokens=args.tokens, fields=nf, k=args.k, warmup=args.warmup, steps=args.steps,
               build_id=build.build_id(), profiler_run=False, shapes={})
    for shape in inner:
        ms = {name.split("/")[1]: [r[0] for r in rs] for name, rs in runs.items() if name.startswith(shape + "/")}
        med = {name: float(np.median(v)) for name, v in ms.items()}
        spread = max(ms["multi_match"]) - min(ms["multi_match"])
        rec = dict(items=int(runs[shape + "/multi_match"][0][1]), postings=int(runs[shape + "/multi_match"][0][2]))
        for name in ms:
            rec[name + "_kernel_ms"] = round(med[name], 4)
        rec["multi_match_spread_ms"] = round(spread, 4)
        rec["functions_0_minus_multi_match_ms"] = round(med["functions_0"] - med["multi_match"], 4)
        rec["functions_0_within_the_bar"] = bool(med["functions_0"] - med["multi_match"] <= spread)
        for name in ("functions_3", "functions_8"):
            rec[name + "_over_functions_0"] = round(med[name] / med["functions_0"], 3)
        for name, v in ms.items():
            rec[name + "_ms_all"] = [round(x, 4) for x in v]
        out["shapes"][shape] = rec
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    for leaf in leaves:
        leaf.release()
    ctx.close()


if __name__ == "__main__":
    main()
