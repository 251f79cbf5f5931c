#!/usr/bin/env python3
"""What the terms aggregation costs beside the sorted-search route it shares its traversal with: one process, bench.py's C3 corpus
(10 M docs, ten tiered segments; the postings of one 1024-query batch of its five-term disjunctions), and the same batch through
both kernels, timed by HIP events (nrtgpu_config.collect_timing -> nrtgpu_stats.scan_ms; for the terms route the interval holds
bm25_terms_count_kernel AND terms_compact_kernel).

  baseline  bm25_field_sort_kernel through nrtgpu_search_sorted_batch (k = 1000), ascending over a random int column
  five      nrtgpu_count_terms_batch over a column of 5 distinct values            (max_buckets 16)
  thousand  ... over a column of 1000 distinct values                              (max_buckets 2048)
  random    ... over the random int column: every query overflows max_buckets 4096 -- the time still counts

Same build, same plan (the exhaustive plan of the same disjunctions), same postings, one 4-byte code per doc on either route.
total_hits of the two routes must agree, and the first two columns must count every hit (checked before anything is timed).
Warm-up calls first; then three rounds of `--steps` runs, the baseline and the three columns alternating; every column's median
is reported as a ratio to the median of the baseline's three round medians, beside the baseline's own spread.  Prints one JSON
line; `--label` names the build (the in-wave combining rounds it was compiled with)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from nrtsearch_amd import api, synth, workload  # noqa: E402

COLUMNS = {"five": (8, 16), "thousand": (9, 2048), "random": (7, 4096)}   # field id, max_buckets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=0, help="0: C3's 10 M")
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--k", type=int, default=0, help="0: C3's 1000")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--label", default="")
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
        g.add_doc_values(7, "int", rng.integers(-2**31, 2**31, size=seg.max_doc, dtype=np.int64).astype(np.int32))
        g.add_doc_values(8, "int", rng.integers(0, 5, size=seg.max_doc).astype(np.int32))
        g.add_doc_values(9, "int", rng.integers(0, 1000, size=seg.max_doc).astype(np.int32))
        g.seal()
        leaves.append(g)
    sr = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics.from_corpus(corpus))
    inner = workload.boolean_queries(qr)
    mgrs = [api.TopScoreDocCollectorManager(k)] * len(inner)
    sorts = [api.SortField(7, "int")] * len(inner)

    def count(name):
        field, bound = COLUMNS[name]
        return api.count_terms_batch(sr, inner, [api.TermsCollector(field, 10)] * len(inner), bound, mgrs)

    base = api.search_sorted_batch(sr, inner, mgrs, sorts)
    buckets = {}
    for name in COLUMNS:
        got = count(name)
        for a, b in zip(base, got):
            assert a.total_hits == b.total_hits, (name, a.total_hits, b.total_hits)
            if name == "random":
                assert b.overflowed or b.total_hits <= COLUMNS[name][1]
            else:
                assert not b.overflowed and b.hits_with_value == b.total_hits == int(b.counts.sum()), name
        buckets[name] = int(np.median([len(b.counts) for b in got]))
    overflowed = sum(int(b.overflowed) for b in got)

    def timed(call):
        ctx.reset_stats()
        call()
        st = ctx.stats()
        assert st["scan_launches"] == 1 and st["maxscore_launches"] == 0, st
        return st["scan_ms"], st["scan_items"], st["scan_postings"]

    def run_base():
        return timed(lambda: api.search_sorted_batch(sr, inner, mgrs, sorts))

    for _ in range(args.warmup):
        run_base()
        for name in COLUMNS:
            timed(lambda: count(name))
    rounds = [[], [], []]
    ms = {name: [] for name in COLUMNS}
    for r in range(3):
        for _ in range(args.steps):
            rounds[r].append(run_base())
            for name in COLUMNS:
                ms[name].append(timed(lambda: count(name))[0])
    base_ms = [float(np.median([s[0] for s in rd])) for rd in rounds]
    mid = float(np.median(base_ms))
    out = dict(label=args.label, docs=w.n_docs, queries=args.queries, terms=w.n_terms, k=k, steps=args.steps, items=int(rounds[0][0][1]),
               postings=int(rounds[0][0][2]), sorted_kernel_ms=[round(m, 4) for m in base_ms],
               sorted_spread=round((max(base_ms) - min(base_ms)) / mid, 4), median_buckets=buckets, random_overflowed=overflowed)
    for name in COLUMNS:
        med = float(np.median(ms[name]))
        out[name] = dict(kernel_ms=round(med, 4), ratio=round(med / mid, 4), min_ms=round(min(ms[name]), 4), max_ms=round(max(ms[name]), 4))
    print(json.dumps(out), flush=True)
    for leaf in leaves:
        leaf.release()
    ctx.close()


if __name__ == "__main__":
    main()
