#!/usr/bin/env python3
"""What a terms count over a MULTI-VALUED column costs beside the same count over a single-valued one, on both routes, and what a
single-valued column pays when a mixed batch sends it through the kernels that handle both arities.

One process, bench.py's C3 corpus (10 M docs, ten tiered segments; the postings of one 1024-query batch of its five-term
disjunctions), two int columns drawn from the same 1000 distinct values: `multi` with 1..5 values per doc (3 on average) and
`single` with one; kernel time by HIP events (nrtgpu_config.collect_timing -> nrtgpu_stats.scan_ms; the interval holds the
compaction too).

  baselines  nrtgpu_count_terms_batch / nrtgpu_count_docset_terms_batch over `single`: bm25_terms_count_kernel and
             docset_count_kernel<DocsetTerms32, false>, the kernels a call without a multi-valued column launches -- untouched by the feature
  multi      the same calls over `multi`: bm25_terms_count_multi_kernel / docset_terms_count_multi_kernel
  mixed      every query but ONE counts `single`, that one counts `multi`: ONE launch of the *_multi kernels -- the price of their
             uniform branches for a single-valued column.  mixed_first: the multi-valued query is query 0 (its items start with
             the launch); mixed_last: it is the last query -- its items start when the others end, and the launch then waits for
             them.  Either way ONE multi-valued query among single-valued ones runs its walk alone, bound by memory latency, and
             the launch waits for it: these two lines show that tail, not the price of the branches
  idle       the price of the branches alone: query 0 of the batch is a query without hits (an absent term; a mask that accepts
             nothing); single_idle counts `single` under it (the baseline's kernels), mixed_idle counts `multi` under it -- ONE
             launch of the *_multi kernels in which every query that does any work is single-valued
  lines      text: the disjunctions; docset: `all` (no mask, 100 % accepted) and `permille` (random masks that accept 0.1 %; query i
             takes mask i mod --masks)

Before anything is timed the outputs are compared on the timed inputs: the mixed batch's single-valued queries equal the
baseline's answers field by field (and its multi-valued query the multi batch's); every multi-valued count has the baseline's total_hits; on `all` the buckets equal numpy's
bincount of every live doc's values, and the first text queries equal a count from the corpus postings.  Warm-up calls first;
then three rounds of --steps runs, all calls alternating; per case the median, the baseline's spread over its three round
medians, and the ratio.  Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from nrtsearch_amd import api, synth, workload  # noqa: E402

MULTI, SINGLE, DISTINCT, BOUND = 7, 9, 1000, 2048
MASK0, DENSITY = 200, 0.001
NOBODY, ABSENT = 199, 1 << 41   # a mask that accepts no doc; a term no leaf holds


def live_of(seg):
    if seg.live_bits is None:
        return np.ones(seg.max_doc, dtype=bool)
    return np.unpackbits(np.ascontiguousarray(seg.live_bits, dtype=np.uint64).view(np.uint8), bitorder="little")[: seg.max_doc].astype(bool)


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
    ctx = api.GpuContext(0, max_batch=nq, collect_timing=True)
    rng = np.random.default_rng(77)
    leaves, columns, n_values = [], [], 0
    for si, seg in enumerate(corpus.segments):
        n = seg.max_doc
        docs = np.repeat(np.arange(n, dtype=np.int32), rng.integers(1, 6, size=n))
        vals = rng.integers(0, DISTINCT, size=len(docs)).astype(np.int32)
        one = rng.integers(0, DISTINCT, size=n).astype(np.int32)
        columns.append((docs, vals, one))
        n_values += len(docs)
        g = api.GpuSegment(ctx, n, seg.doc_base)
        g.add_field_norms(0, seg.norms)
        g.add_terms(0, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
        g.add_doc_values_multi(MULTI, "int", vals, docs)
        g.add_doc_values(SINGLE, "int", one)
        g.seal()
        if seg.live_bits is not None:
            g.set_live_docs(seg.live_bits)
        for j in range(args.masks):
            g.set_mask(MASK0 + j, synth.random_mask(n, DENSITY, 1000 * MASK0 + 16 * j + si))
        g.set_mask(NOBODY, np.zeros((n + 63) // 64, dtype=np.uint64))
        leaves.append(g)
    sr = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics.from_corpus(corpus))
    text = workload.boolean_queries(qr)
    docsets = {"all": [api.DocSetQuery()] * nq, "permille": [api.DocSetQuery((api.MaskFilter(MASK0 + i % args.masks),)) for i in range(nq)]}
    single, multi = [api.TermsCollector(SINGLE, 10)] * nq, [api.TermsCollector(MULTI, 10)] * nq
    cases = {"single": single, "multi": multi, "mixed_first": multi[:1] + single[1:], "mixed_last": single[:-1] + multi[:1]}
    idle = {"single_idle": single, "mixed_idle": multi[:1] + single[1:]}   # under a query 0 without hits
    nowhere, nobody = api.TermQuery(0, ABSENT), api.DocSetQuery((api.MaskFilter(NOBODY),))

    calls = {}
    for case, colls in cases.items():
        calls[("text", case)] = lambda colls=colls: api.count_terms_batch(sr, text, colls, BOUND)
        for line, ds in docsets.items():
            calls[(line, case)] = lambda colls=colls, ds=ds: api.count_docset_terms_batch(sr, ds, colls, BOUND)
    for case, colls in idle.items():
        calls[("text", case)] = lambda colls=colls: api.count_terms_batch(sr, [nowhere] + text[1:], colls, BOUND)
        for line, ds in docsets.items():
            calls[(line, case)] = lambda colls=colls, ds=ds: api.count_docset_terms_batch(sr, [nobody] + ds[1:], colls, BOUND)

    # ---- the outputs on the timed inputs
    instances = {}
    for line in ["text"] + list(docsets):
        a, b = calls[(line, "single")](), calls[(line, "multi")]()
        for case, at in (("mixed_first", 0), ("mixed_last", nq - 1)):
            c = calls[(line, case)]()
            for qi, (x, y) in enumerate(zip(a, c)):
                x = b[qi] if qi == at else x
                assert x.value_bits.tolist() == y.value_bits.tolist() and x.counts.tolist() == y.counts.tolist(), (line, case, qi)
                assert (x.total_hits, x.hits_with_value, x.overflowed) == (y.total_hits, y.hits_with_value, y.overflowed), (line, case, qi)
        a0, c0 = calls[(line, "single_idle")](), calls[(line, "mixed_idle")]()
        assert a0[0].total_hits == c0[0].total_hits == 0
        for x, y, z in zip(a[1:], a0[1:], c0[1:]):
            assert x.value_bits.tolist() == y.value_bits.tolist() == z.value_bits.tolist() and x.counts.tolist() == y.counts.tolist() == z.counts.tolist(), line
            assert x.total_hits == y.total_hits == z.total_hits and x.hits_with_value == y.hits_with_value == z.hits_with_value, line
        for x, y in zip(a, b):
            assert x.total_hits == y.total_hits and not x.overflowed and not y.overflowed and x.hits_with_value == x.total_hits, line
        instances[line] = dict(median_hits=int(np.median([x.total_hits for x in a])), median_values=int(np.median([y.hits_with_value for y in b])))
    every = np.zeros(DISTINCT, dtype=np.int64)
    for seg, (docs, vals, _) in zip(corpus.segments, columns):
        every += np.bincount(vals[live_of(seg)[docs]], minlength=DISTINCT)
    got = calls[("all", "multi")]()[0]
    assert got.values.tolist() == list(range(DISTINCT)) and got.counts.tolist() == every.tolist()
    for qi, tc in enumerate(calls[("text", "multi")]()[:3]):
        exp = np.zeros(DISTINCT, dtype=np.int64)
        for seg, (docs, vals, _) in zip(corpus.segments, columns):
            hit = np.zeros(seg.max_doc, dtype=bool)
            for t in qr[qi].tolist():
                hit[seg.postings(int(t))[0]] = True
            exp += np.bincount(vals[(hit & live_of(seg))[docs]], minlength=DISTINCT)
        assert tc.counts.tolist() == exp[exp > 0].tolist() and tc.values.tolist() == np.nonzero(exp)[0].tolist(), qi

    def timed(key):
        ctx.reset_stats()
        calls[key]()
        st = ctx.stats()
        assert st["scan_launches"] == 1 and st["maxscore_launches"] == 0, st
        return st["scan_ms"]

    for _ in range(args.warmup):
        for key in calls:
            timed(key)
    ms = {key: [[], [], []] for key in calls}
    for r in range(3):
        for _ in range(args.steps):
            for key in calls:
                ms[key][r].append(timed(key))
    out = dict(docs=corpus.n_docs, queries=nq, steps=args.steps, values=n_values, distinct=DISTINCT, max_buckets=BOUND, masks_per_line=args.masks)
    for line in ["text"] + list(docsets):
        rounds = [float(np.median(r)) for r in ms[(line, "single")]]
        base = float(np.median(rounds))
        res = dict(instances[line], single_ms=round(base, 4), single_round_medians=[round(x, 4) for x in rounds],
                   single_spread=round((max(rounds) - min(rounds)) / base, 4))
        for case in ("multi", "mixed_first", "mixed_last"):
            mine = float(np.median([t for r in ms[(line, case)] for t in r]))
            res[case + "_ms"] = round(mine, 4)
            res[case + "_ratio"] = round(mine / base, 4)
        rounds = [float(np.median(r)) for r in ms[(line, "single_idle")]]
        base = float(np.median(rounds))
        mine = float(np.median([t for r in ms[(line, "mixed_idle")] for t in r]))
        res.update(single_idle_ms=round(base, 4), single_idle_spread=round((max(rounds) - min(rounds)) / base, 4), mixed_idle_ms=round(mine, 4),
                   mixed_idle_ratio=round(mine / base, 4))
        out[line] = res
    print(json.dumps(out), flush=True)
    for leaf in leaves:
        leaf.release()
    ctx.close()


if __name__ == "__main__":
    main()
