#!/usr/bin/env python3
"""The hybrid tail over a byte (int8) vector field against the float one, one process, one MI355X: 256 queries x
recall 1000 -> cosine rescore over 768-d rows -> top-100, 5 M rows per field, the SAME docs, docids and first pass for both --
nrtgpu_search_hybrid_bytes_batch and nrtgpu_search_hybrid_batch called alternately.  Every leaf uploads the same random block into
both fields (the tail gathers 1000 rows per query; their values do not matter for the timing).

Kernel times (hybrid_rescore_bytes_kernel, hybrid_rescore_kernel) are the profiler's:
    rocprofv3 --kernel-trace --stats -d OUT -o hybrid_bytes --output-format csv -- python scripts/gpu_hybrid_bytes.py
    python scripts/gpu_hybrid_bytes.py --trace OUT/.../hybrid_bytes_kernel_trace.csv
The second command prints the median per kernel over the launches behind the warm-up.  Without a profiler the run prints the
end-to-end call times only (first pass included).  JSON lines."""
import argparse
import csv
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

KERNELS = ("hybrid_rescore_bytes_kernel", "hybrid_rescore_kernel")


def log(**kw):
    print(json.dumps(kw), flush=True)


def medians(path, warmup):
    """Median duration per tail kernel from a rocprofv3 kernel trace (csv), the first `warmup` launches of each left out."""
    by = {k: [] for k in KERNELS}
    for row in csv.DictReader(open(path)):
        name = row.get("Kernel_Name", "")
        for k in KERNELS:
            if k + "(" in name or name.endswith(k) or f"{len(k)}{k}E" in name:   # demangled, bare or mangled
                by[k].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]) - int(row["Start_Timestamp"])))
    for k, v in by.items():
        d = [ns for _, ns in sorted(v)][warmup:]
        log(event="kernel_time", kernel=k, launches=len(d), median_us=round(float(np.median(d)) / 1e3, 1) if d else None,
            min_us=round(min(d) / 1e3, 1) if d else None, max_us=round(max(d) / 1e3, 1) if d else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=5_000_000)
    ap.add_argument("--seg-docs", type=int, default=1_250_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--trace", help="a rocprofv3 kernel trace (csv) of an earlier run: print the kernels' medians and leave")
    args = ap.parse_args()
    if args.trace:
        medians(args.trace, args.warmup)
        return
    from nrtsearch_amd import _lib, api, synth

    N, B, dim = args.docs, args.batch, args.dim
    t0 = time.time()
    qr = synth.make_queries(B, 5, 10000)
    ranks = sorted(set(int(r) for r in qr.reshape(-1)))
    lens = synth.doc_lengths(N)
    norms_all = synth.int_to_byte4(lens)
    n_seg = (N + args.seg_docs - 1) // args.seg_docs
    bases = np.minimum(np.arange(n_seg + 1, dtype=np.int64) * args.seg_docs, N)
    per_docs = [[] for _ in range(n_seg)]
    per_freqs = [[] for _ in range(n_seg)]
    doc_freq = {}
    for r in ranks:
        d, f = synth.term_postings(N, r)
        doc_freq[r] = int(len(d))
        cuts = np.searchsorted(d, bases)
        for s in range(n_seg):
            a, b = int(cuts[s]), int(cuts[s + 1])
            per_docs[s].append((d[a:b] - bases[s]).astype(np.int32))
            per_freqs[s].append(f[a:b])
    segments = []
    for s in range(n_seg):
        counts = np.asarray([len(x) for x in per_docs[s]], dtype=np.int64)
        segments.append(synth.SegmentData(
            max_doc=int(bases[s + 1] - bases[s]), doc_base=int(bases[s]), norms=norms_all[bases[s]: bases[s + 1]].copy(),
            term_ids=np.asarray(ranks, dtype=np.int64), offsets=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64),
            docids=np.ascontiguousarray(np.concatenate(per_docs[s]), dtype=np.int32),
            freqs=np.ascontiguousarray(np.concatenate(per_freqs[s]), dtype=np.int32)))
    del per_docs, per_freqs
    corpus = synth.Corpus(n_docs=N, doc_count=N, sum_total_term_freq=int(lens.astype(np.int64).sum()), segments=segments,
                          doc_freq=doc_freq)
    log(event="corpus", docs=N, segments=n_seg, postings=corpus.total_postings, build_s=round(time.time() - t0, 1))

    t0 = time.time()
    rng = np.random.default_rng(7)
    fblock = rng.standard_normal((args.seg_docs, dim), dtype=np.float32)
    bblock = rng.integers(-128, 128, size=(args.seg_docs, dim), dtype=np.int8)
    ctx = api.GpuContext(0, max_batch=B)
    leaves = []
    for seg in segments:
        g = api.GpuSegment(ctx, seg.max_doc, seg.doc_base)
        g.add_field_norms(0, seg.norms)
        g.add_terms(0, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
        g.add_vectors(7, fblock[: seg.max_doc])
        g.add_byte_vectors(8, bblock[: seg.max_doc])
        g.seal()
        leaves.append(g)
    del fblock, bblock
    log(event="upload", seconds=round(time.time() - t0, 1), device_gb=round(sum(l.device_bytes for l in leaves) / 2**30, 1))
    sr = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics.from_corpus(corpus))
    queries = [api.BooleanQuery(tuple(api.TermQuery(0, int(t)) for t in row)) for row in qr]
    mgr = api.TopScoreDocCollectorManager(1000)
    qf = rng.standard_normal((B, dim), dtype=np.float32)
    qb = rng.integers(-128, 128, size=(B, dim), dtype=np.int8)

    # the byte tail's answer at this size: fused == two calls for the first queries
    fused = sr.search_hybrid_bytes_batch(queries[:4], [mgr] * 4, 8, "cosine", qb[:4], 100, 1.0, 2.0)
    bad = 0
    for qi in range(4):
        two = sr.rescore_byte_vectors(sr.search(queries[qi], mgr), 8, "cosine", qb[qi], 100, 1.0, 2.0)
        bad += not (two.docs.tolist() == fused[qi].docs.tolist() and two.scores.view(np.uint32).tolist() == fused[qi].scores.view(np.uint32).tolist())
    log(event="parity_full_size", queries=4, mismatches=int(bad))

    L = _lib.load()
    m = sr._marshal(queries, [mgr] * B)
    outs = (_lib.TopDocs * B)()
    od = np.zeros((B, 100), np.int32)
    os_ = np.zeros((B, 100), np.float32)
    for qi in range(B):
        outs[qi].capacity = 100
        outs[qi].docs = od[qi].ctypes.data_as(C.POINTER(C.c_int32))
        outs[qi].scores = os_[qi].ctypes.data_as(C.POINTER(C.c_float))

    def float_call():
        _lib.check(L.nrtgpu_search_hybrid_batch(ctx._h, sr._segs, sr._bases, len(leaves), m.queries, B, 7, 0, qf.ctypes.data, dim,
                                                C.c_float(1.0), 1.0, 2.0, 100, outs))

    def byte_call():
        _lib.check(L.nrtgpu_search_hybrid_bytes_batch(ctx._h, sr._segs, sr._bases, len(leaves), m.queries, B, 8, 0, qb.ctypes.data, dim,
                                                      C.c_float(1.0), 1.0, 2.0, 100, outs))

    t_f, t_b = [], []
    for step in range(args.warmup + args.steps):      # alternately: both see the same machine
        t0 = time.perf_counter()
        float_call()
        t1 = time.perf_counter()
        byte_call()
        t2 = time.perf_counter()
        if step >= args.warmup:
            t_f.append((t1 - t0) * 1e3)
            t_b.append((t2 - t1) * 1e3)
    hits = float(np.mean([o.n_hits for o in outs]))
    log(event="hybrid_calls", docs=N, dim=dim, batch=B, steps=args.steps, float_call_ms_median=round(float(np.median(t_f)), 3),
        byte_call_ms_median=round(float(np.median(t_b)), 3), mean_window_hits=hits,
        note="whole calls, first pass included; the tail kernels' own times come from the profiler (see the docstring)")
    for g in leaves:
        g.release()
    ctx.close()


if __name__ == "__main__":
    main()
