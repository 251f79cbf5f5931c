#!/usr/bin/env python3
"""What the numeric range facet costs beside the terms aggregation it shares its traversal with: one process, bench.py's C3 corpus
(10 M docs, ten tiered segments; the postings of one 1024-query batch of its five-term disjunctions), the same batch through both
routes, timed by HIP events (nrtgpu_config.collect_timing -> nrtgpu_stats.scan_ms; for the terms route the interval holds
bm25_terms_count_kernel AND terms_compact_kernel).

  text      terms_five     nrtgpu_count_terms_batch over a column of 5 distinct values (max_buckets 16) -- the baseline
            terms_floor    ... over a random int column: every query overflows, the kernel only counts hits -- the traversal's floor
            int_4 / int_64     nrtgpu_count_ranges_batch, 4 / 64 ranges over the random int column (32-bit codes)
            five_4             ... 4 ranges over the five-value column (every hit on one of five LDS counters)
            long_4 / long_64   ... over a ten-year epoch-millis column (64-bit codes)
  docset    per selectivity (scripts/gpu_docset.py's: every doc, a tenth, a permille -- 16 masks per line):
            terms          nrtgpu_count_docset_terms_batch over a column of 1000 distinct values (max_buckets 2048)
            int_4 / int_64 / long_4 / long_64   nrtgpu_count_docset_ranges_batch

Same build, same plans, same postings.  total_hits of the routes must agree and the ranges that cover every value must count
every valued hit (checked before anything is timed).  Warm-up calls first; then three rounds of `--steps` runs, all lines
alternating; every line's median is reported with its spread and as a ratio to the median of its baseline's three round medians.
Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from nrtsearch_amd import api, synth, workload  # noqa: E402

EVERY = 1 << 40        # the term indexed in every doc (the doc-set lines' text twin is not timed: the docset terms kernel is the baseline)
RANDOM, FIVE, THOUSAND, MILLIS = 7, 8, 9, 12
T0, TEN_YEARS = 1_400_000_000_000, 10 * 365 * 86_400_000
LINES = {"all": None, "tenth": (100, 0.1), "permille": (200, 0.001)}   # first mask id, density


def int_ranges(n):
    """n ranges over the int32 range: n = 4 disjoint quarters; more: overlapping "at least" ranges and windows"""
    edges = np.linspace(-2**31, 2**31 - 1, n + 1).astype(np.int64)
    out = [(int(edges[i]), int(edges[i + 1]) - (i + 1 < n)) for i in range(min(n, 4))]
    out += [(int(edges[i]), 2**31 - 1) if i % 2 else (int(edges[i]), int(edges[min(i + 3, n)])) for i in range(4, n)]
    return tuple((api._value_bits("int", a), api._value_bits("int", b)) for a, b in out)


def long_ranges(n):
    """the same shapes over ten years of epoch millis: "the last day / week / month / year" when n = 4"""
    end = T0 + TEN_YEARS
    if n == 4:
        out = [(end - d * 86_400_000, end) for d in (1, 7, 30, 365)]
    else:
        edges = np.linspace(T0, end, n + 1).astype(np.int64)
        out = [(int(edges[i]), end) if i % 2 else (int(edges[i]), int(edges[min(i + 3, n)])) for i in range(n)]
    return tuple((api._value_bits64("long", a), api._value_bits64("long", b)) for a, b in out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=0, help="0: C3's 10 M")
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--masks", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    args = ap.parse_args()

    w = workload.C3
    if args.docs:
        w = workload.Workload(f"C3 shape at {args.docs} docs", args.docs, w.n_terms, w.k, w.n_queries, w.segments_per_shard, w.max_rank)
    nq = args.queries
    qr = synth.make_queries(w.n_queries, w.n_terms, w.max_rank)[:nq]
    corpus = workload.build_shard_corpus(w, qr, 1, 0)
    print(f"corpus: {corpus.n_docs} docs", file=sys.stderr, flush=True)
    ctx = api.GpuContext(0, max_batch=nq, collect_timing=True)
    rng = np.random.default_rng(77)
    leaves = []
    for si, seg in enumerate(corpus.segments):
        n = seg.max_doc
        g = api.GpuSegment(ctx, n, seg.doc_base)
        g.add_field_norms(0, seg.norms)
        g.add_terms(0, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
        g.add_doc_values(RANDOM, "int", rng.integers(-2**31, 2**31, size=n, dtype=np.int64).astype(np.int32))
        g.add_doc_values(FIVE, "int", rng.integers(0, 5, size=n).astype(np.int32))
        g.add_doc_values(THOUSAND, "int", rng.integers(0, 1000, size=n).astype(np.int32))
        g.add_doc_values64(MILLIS, "long", T0 + rng.integers(0, TEN_YEARS, size=n, dtype=np.int64))
        g.seal()
        for first, density in (v for v in LINES.values() if v):
            for j in range(args.masks):
                g.set_mask(first + j, synth.random_mask(n, density, 1000 * first + 16 * j + si))
        leaves.append(g)
    sr = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics.from_corpus(corpus))
    inner = workload.boolean_queries(qr)
    mgrs = [api.TopScoreDocCollectorManager(10)] * nq
    counters = {
        "int_4": api.RangeCounter(RANDOM, "int", int_ranges(4)), "int_64": api.RangeCounter(RANDOM, "int", int_ranges(64)),
        "five_4": api.RangeCounter(FIVE, "int", tuple((api._value_bits("int", a), api._value_bits("int", b)) for a, b in ((0, 0), (1, 2), (2, 4), (3, 9)))),
        "long_4": api.RangeCounter(MILLIS, "long", long_ranges(4)), "long_64": api.RangeCounter(MILLIS, "long", long_ranges(64)),
    }
    docsets = {name: [api.DocSetQuery(() if v is None else (api.MaskFilter(v[0] + (i % args.masks)),)) for i in range(nq)] for name, v in LINES.items()}

    calls = {("text", "terms_five"): lambda: api.count_terms_batch(sr, inner, [api.TermsCollector(FIVE, 10)] * nq, 16, mgrs),
             ("text", "terms_floor"): lambda: api.count_terms_batch(sr, inner, [api.TermsCollector(RANDOM, 10)] * nq, 4096, mgrs)}
    for name, c in counters.items():
        calls[("text", name)] = lambda c=c: api.count_ranges_batch(sr, inner, [c] * nq, mgrs)
    for line in LINES:
        calls[(line, "terms")] = lambda line=line: api.count_docset_terms_batch(sr, docsets[line], [api.TermsCollector(THOUSAND, 10)] * nq, 2048, mgrs)
        for name in ("int_4", "int_64", "long_4", "long_64"):
            calls[(line, name)] = lambda line=line, c=counters[name]: api.count_docset_ranges_batch(sr, docsets[line], [c] * nq, mgrs)

    # the routes answer alike on the timed inputs
    hits = {}
    for group in ["text"] + list(LINES):
        base = calls[(group, "terms_five" if group == "text" else "terms")]()
        assert not any(b.overflowed for b in base)
        hits[group] = int(np.median([b.total_hits for b in base]))
        for name in counters:
            if (group, name) not in calls:
                continue
            got = calls[(group, name)]()
            for b, r in zip(base, got):
                assert r.total_hits == b.total_hits == r.hits_with_value, (group, name)
                if name in ("int_4", "five_4"):
                    assert int(r.counts[:4].sum()) >= r.total_hits if name == "five_4" else int(r.counts.sum()) == r.total_hits, (group, name)
            if group == "text" and name == "five_4":   # against the terms route's buckets
                for b, r in zip(base, got):
                    by = dict(zip(b.values.tolist(), b.counts.tolist()))
                    assert r.counts.tolist() == [by.get(0, 0), by.get(1, 0) + by.get(2, 0), by.get(2, 0) + by.get(3, 0) + by.get(4, 0), by.get(3, 0) + by.get(4, 0)]
    print("the routes agree on the timed inputs", file=sys.stderr, flush=True)
    floor_overflowed = sum(int(b.overflowed) for b in calls[("text", "terms_floor")]())

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
        print(f"round {r + 1} of 3", file=sys.stderr, flush=True)
    out = dict(docs=corpus.n_docs, queries=nq, steps=args.steps, masks_per_line=args.masks, median_hits=hits, floor_queries_overflowed=floor_overflowed)
    for group in ["text"] + list(LINES):
        base_key = (group, "terms_five" if group == "text" else "terms")
        rounds = [float(np.median(r)) for r in ms[base_key]]
        base = float(np.median(rounds))
        res = dict(baseline=base_key[1], baseline_ms=round(base, 4), baseline_round_medians=[round(x, 4) for x in rounds],
                   baseline_spread=round((max(rounds) - min(rounds)) / base, 4), items=int(items[base_key]))
        for key in calls:
            if key[0] != group or key == base_key:
                continue
            runs = [t for r in ms[key] for t in r]
            med = float(np.median(runs))
            res[key[1]] = dict(kernel_ms=round(med, 4), min_ms=round(min(runs), 4), max_ms=round(max(runs), 4), ratio=round(med / base, 4))
        out[group] = res
    print(json.dumps(out), flush=True)
    for leaf in leaves:
        leaf.release()
    ctx.close()


if __name__ == "__main__":
    main()
