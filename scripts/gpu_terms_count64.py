#!/usr/bin/env python3
"""What the terms aggregation over a 64-bit column costs beside the 32-bit one ON THE SAME BUILD: one process, bench.py's C3 corpus
(10 M docs, ten tiered segments; the postings of one 1024-query batch of its five-term disjunctions), and per column cardinality
the same values held twice -- once as an int column, once widened to a LONG column -- counted by the same batch of queries through
nrtgpu_count_terms_batch and nrtgpu_count_terms64_batch, timed by HIP events (nrtgpu_config.collect_timing ->
nrtgpu_stats.scan_ms; the interval holds the counting kernel AND the compaction of the tables).

  five       5 distinct values       (max_buckets 16)
  thousand   1000 distinct values    (max_buckets 2048)
  sixty_k    60 000 distinct values  (max_buckets 65536; --queries-wide queries: a table of 2^17 slots each)
  docset     the doc-set form (nrtgpu_count_docset_terms_batch / ...64_batch) over `thousand` under one filter mask of
             density --density, --queries-docset queries

Same plan, same postings, same hit sets; 4 bytes of column per doc on one side, 8 on the other.  The two entries must return the
same buckets and counts (checked before anything is timed).  Warm-up calls first; then three rounds of `--steps` runs, the two
widths alternating; per line the median per-batch time of each entry, the ratio of the two and the spread of the 32-bit entry's
three round medians.  Prints one JSON line and, with --out, writes it to a file (profiles/terms_count64.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from nrtsearch_amd import api, build, synth, workload  # noqa: E402

COLUMNS = {"five": (5, 16), "thousand": (1000, 2048), "sixty_k": (60_000, 65536)}   # distinct values, max_buckets
FIELD32 = {"five": 8, "thousand": 9, "sixty_k": 10}
FIELD64 = {"five": 18, "thousand": 19, "sixty_k": 20}
MASK = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=0, help="0: C3's 10 M")
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--queries-wide", type=int, default=128, help="queries of the sixty_k lines")
    ap.add_argument("--queries-docset", type=int, default=64)
    ap.add_argument("--density", type=float, default=0.25, help="the doc-set lines' filter mask")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    w = workload.C3
    if args.docs:
        w = workload.Workload(f"C3 shape at {args.docs} docs", args.docs, w.n_terms, w.k, w.n_queries, w.segments_per_shard, w.max_rank)
    qr = synth.make_queries(w.n_queries, w.n_terms, w.max_rank)[: args.queries]
    corpus = workload.build_shard_corpus(w, qr, 1, 0)
    ctx = api.GpuContext(0, max_batch=args.queries, collect_timing=True)
    rng = np.random.default_rng(77)
    leaves = []
    for si, seg in enumerate(corpus.segments):
        g = api.GpuSegment(ctx, seg.max_doc, seg.doc_base)
        g.add_field_norms(0, seg.norms)
        g.add_terms(0, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
        for name, (distinct, _) in COLUMNS.items():
            v = rng.integers(0, distinct, size=seg.max_doc).astype(np.int32)
            g.add_doc_values(FIELD32[name], "int", v)
            g.add_doc_values64(FIELD64[name], "long", v.astype(np.int64))   # the same values, widened
        g.seal()
        g.set_mask(MASK, synth.random_mask(seg.max_doc, args.density, 900 + si))
        leaves.append(g)
    sr = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics.from_corpus(corpus))
    inner = workload.boolean_queries(qr)
    docsets = [api.DocSetQuery((api.MaskFilter(MASK),))] * args.queries_docset

    def call(name, wide):
        """-> the entry's results for one line"""
        if name == "docset":
            fn, field, kind = (api.count_docset_terms64_batch, FIELD64["thousand"], "long") if wide else (api.count_docset_terms_batch, FIELD32["thousand"], "int")
            return fn(sr, docsets, [api.TermsCollector(field, 10, True, kind)] * len(docsets), COLUMNS["thousand"][1])
        q = inner[: args.queries_wide] if name == "sixty_k" else inner
        fn, field, kind = (api.count_terms64_batch, FIELD64[name], "long") if wide else (api.count_terms_batch, FIELD32[name], "int")
        return fn(sr, q, [api.TermsCollector(field, 10, True, kind)] * len(q), COLUMNS[name][1])

    lines = list(COLUMNS) + ["docset"]
    buckets, overflowed = {}, {}
    for name in lines:   # the two widths agree, bucket for bucket
        narrow, wide = call(name, False), call(name, True)
        for a, b in zip(narrow, wide):
            assert (a.total_hits, a.hits_with_value, a.overflowed) == (b.total_hits, b.hits_with_value, b.overflowed), name
            assert a.values.astype(np.int64).tolist() == b.values.tolist() and a.counts.tolist() == b.counts.tolist(), name
        buckets[name] = int(np.median([len(b.counts) for b in wide]))
        overflowed[name] = sum(int(b.overflowed) for b in wide)

    def timed(name, wide):
        ctx.reset_stats()
        call(name, wide)
        st = ctx.stats()
        assert st["scan_launches"] == 1 and st["maxscore_launches"] == 0, st
        return st["scan_ms"], st["scan_items"]

    for _ in range(args.warmup):
        for name in lines:
            timed(name, False)
            timed(name, True)
    ms = {(name, wide): [[], [], []] for name in lines for wide in (False, True)}
    items = {}
    for r in range(3):
        for _ in range(args.steps):
            for name in lines:
                for wide in (False, True):
                    t, items[name] = timed(name, wide)
                    ms[(name, wide)][r].append(t)
    out = dict(label=args.label, build_id=build.build_id(), docs=w.n_docs, queries=args.queries, queries_wide=args.queries_wide,
               queries_docset=args.queries_docset, docset_density=args.density, terms=w.n_terms, steps=args.steps, median_buckets=buckets,
               overflowed=overflowed, items=items)
    for name in lines:
        rounds32 = [float(np.median(r)) for r in ms[(name, False)]]
        m32 = float(np.median(sum(ms[(name, False)], [])))
        m64 = float(np.median(sum(ms[(name, True)], [])))
        out[name] = dict(ms_32bit=round(m32, 4), ms_64bit=round(m64, 4), ratio=round(m64 / m32, 4),
                         spread_32bit=round((max(rounds32) - min(rounds32)) / float(np.median(rounds32)), 4),
                         min_max_64bit=[round(min(sum(ms[(name, True)], [])), 4), round(max(sum(ms[(name, True)], [])), 4)])
    text = json.dumps(out)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    for leaf in leaves:
        leaf.release()
    ctx.close()


if __name__ == "__main__":
    main()
