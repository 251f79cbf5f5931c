#!/usr/bin/env python3
"""What a doc-set request costs on its own route (docset.hip) beside the only way the parent commit's library answers the same
question: the text route over a one-clause query whose term is indexed in EVERY doc, under the same masks
(nrtgpu_search_sorted_batch / nrtgpu_count_terms_batch: 8 B of postings and one LDS atomic per doc on top of the column).

One process, bench.py's C3 corpus (10 M docs, ten tiered segments) with one more term in every doc, a random int column (the
sort) and a column of 1000 distinct values (the count); batches of 1024 queries, k = 1000; kernel time by HIP events
(nrtgpu_config.collect_timing -> nrtgpu_stats.scan_ms; for the counting routes the interval holds the compaction too).

  all        no mask: every doc is a hit
  tenth      a random mask that accepts 10 % of the docs (query i takes mask i mod `--masks`: a segment keeps at most 64
             combined accept sets resident)
  permille   ... 0.1 %
  half_range no mask, ONE range clause on the sort column that keeps the negative half (doc-set route only: the text route has no
             range clause; its ratio is to the baseline of `all`, which answers another question)

Before anything is timed the two routes' outputs are compared on the timed inputs (docs, value bits, total_hits, relation;
buckets).  Warm-up calls first; then three rounds of `--steps` runs, the routes and lines alternating; per line the median of
each route, the baseline's spread over its three round medians, and the ratio.  Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from nrtsearch_amd import api, synth, workload  # noqa: E402

EVERY = 1 << 40        # the term indexed in every doc
SORT_COL, COUNT_COL = 7, 9
LINES = {"all": None, "tenth": (100, 0.1), "permille": (200, 0.001)}   # first mask id, density


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=0, help="0: C3's 10 M")
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--k", type=int, default=0, help="0: C3's 1000")
    ap.add_argument("--masks", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    args = ap.parse_args()

    w = workload.C3
    if args.docs:
        w = workload.Workload(f"C3 shape at {args.docs} docs", args.docs, w.n_terms, w.k, w.n_queries, w.segments_per_shard, w.max_rank)
    k, nq = args.k or w.k, args.queries
    qr = synth.make_queries(w.n_queries, w.n_terms, w.max_rank)[:nq]
    corpus = workload.build_shard_corpus(w, qr, 1, 0)
    ctx = api.GpuContext(0, max_batch=nq, collect_timing=True)
    rng = np.random.default_rng(77)
    leaves = []
    for si, seg in enumerate(corpus.segments):
        n = seg.max_doc
        g = api.GpuSegment(ctx, n, seg.doc_base)
        g.add_field_norms(0, seg.norms)
        g.add_terms(0, np.array([EVERY], np.int64), np.array([0, n], np.int64), np.arange(n, dtype=np.int32), np.ones(n, dtype=np.int32))
        g.add_doc_values(SORT_COL, "int", rng.integers(-2**31, 2**31, size=n, dtype=np.int64).astype(np.int32))
        g.add_doc_values(COUNT_COL, "int", rng.integers(0, 1000, size=n).astype(np.int32))
        g.seal()
        for first, density in (v for v in LINES.values() if v):
            for j in range(args.masks):
                g.set_mask(first + j, synth.random_mask(n, density, 1000 * first + 16 * j + si))
        leaves.append(g)
    stats = api.IndexStatistics.from_corpus(corpus)
    stats.doc_freq[(0, EVERY)] = corpus.n_docs
    sr = api.GpuIndexSearcher(ctx, leaves, stats)
    every = api.TermQuery(0, EVERY)
    mgrs = [api.TopScoreDocCollectorManager(k)] * nq
    sorts = [api.SortField(SORT_COL, "int")] * nq
    colls = [api.TermsCollector(COUNT_COL, 10)] * nq
    text, docsets = {}, {}
    for name, v in LINES.items():
        ids = [None] * nq if v is None else [v[0] + (i % args.masks) for i in range(nq)]
        text[name] = [every if m is None else api.BooleanQuery((every,), 1, (api.MaskFilter(m),)) for m in ids]
        docsets[name] = [api.DocSetQuery(() if m is None else (api.MaskFilter(m),)) for m in ids]
    docsets["half_range"] = [api.DocSetQuery((), (), (api.RangeClause(SORT_COL, "int", -2**31, -1),))] * nq

    calls = {}
    for name in LINES:
        calls[("sorted", name, "text")] = lambda name=name: api.search_sorted_batch(sr, text[name], mgrs, sorts)
        calls[("sorted", name, "docset")] = lambda name=name: api.search_docset_sorted_batch(sr, docsets[name], mgrs, sorts)
        calls[("counted", name, "text")] = lambda name=name: api.count_terms_batch(sr, text[name], colls, 2048, mgrs)
        calls[("counted", name, "docset")] = lambda name=name: api.count_docset_terms_batch(sr, docsets[name], colls, 2048, mgrs)
    calls[("sorted", "half_range", "docset")] = lambda: api.search_docset_sorted_batch(sr, docsets["half_range"], mgrs, sorts)
    calls[("counted", "half_range", "docset")] = lambda: api.count_docset_terms_batch(sr, docsets["half_range"], colls, 2048, mgrs)

    # the two routes answer alike on the timed inputs
    hits = {}
    for name in LINES:
        a, b = calls[("sorted", name, "text")](), calls[("sorted", name, "docset")]()
        for x, y in zip(a, b):
            assert x.docs.tolist() == y.docs.tolist() and x.value_bits.tolist() == y.value_bits.tolist(), name
            assert (x.total_hits, x.relation_gte) == (y.total_hits, y.relation_gte), name
        a, b = calls[("counted", name, "text")](), calls[("counted", name, "docset")]()
        for x, y in zip(a, b):
            assert x.value_bits.tolist() == y.value_bits.tolist() and x.counts.tolist() == y.counts.tolist(), name
            assert (x.total_hits, x.hits_with_value, x.overflowed) == (y.total_hits, y.hits_with_value, y.overflowed) and not x.overflowed, name
        hits[name] = int(np.median([x.total_hits for x in b]))
    half = calls[("sorted", "half_range", "docset")]()[0]
    hits["half_range"] = int(half.total_hits)
    assert half.values.max() < 0 and abs(half.total_hits / corpus.n_docs - 0.5) < 0.01

    def timed(key):
        ctx.reset_stats()
        calls[key]()
        st = ctx.stats()
        assert st["scan_launches"] == 1 and st["maxscore_launches"] == 0, st
        return st["scan_ms"], st["scan_items"]

    for _ in range(args.warmup):
        for key in calls:
            timed(key)
    ms = {key: [[], [], []] for key in calls}
    items = {}
    for r in range(3):
        for _ in range(args.steps):
            for key in calls:
                t, items[key] = timed(key)
                ms[key][r].append(t)
    out = dict(docs=corpus.n_docs, queries=nq, k=k, steps=args.steps, masks_per_line=args.masks, median_hits=hits)
    for kind in ("sorted", "counted"):
        res = {}
        for name in list(LINES) + ["half_range"]:
            base_key = (kind, name if name in LINES else "all", "text")
            rounds = [float(np.median(r)) for r in ms[base_key]]
            base = float(np.median(rounds))
            mine = float(np.median([t for r in ms[(kind, name, "docset")] for t in r]))
            res[name] = dict(text_ms=round(base, 4), text_round_medians=[round(x, 4) for x in rounds], text_spread=round((max(rounds) - min(rounds)) / base, 4),
                             docset_ms=round(mine, 4), ratio=round(mine / base, 4), text_items=int(items[base_key]), docset_items=int(items[(kind, name, "docset")]))
        out[kind] = res
    print(json.dumps(out), flush=True)
    for leaf in leaves:
        leaf.release()
    ctx.close()


if __name__ == "__main__":
    main()
