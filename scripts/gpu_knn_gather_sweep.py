#!/usr/bin/env python3
"""The gather route of the filtered knn requests (nrtgpu_set_knn_gather) against the full pass, on the GPU.

    python scripts/gpu_knn_gather_sweep.py [--rows 2000000] [--dim 768] [--out profiles/knn_gather_sweep.log]

One corpus of --rows x --dim fp32 rows and one of as many int8 rows (eight leaves each), filters accepting 0.01 %, 0.1 %, 1 %, 3 %
and 10 % of the docs, 1 and 64 queries, k = 10.  The same request at knob 0 (the full pass over every row: the only route before
the knob existed) and at knob 1000 (only the accepted rows), in ONE process: a warm-up of each (the sketch, the accept sets, the
workspaces; the two answers are compared with == there), then five repetitions of each, interleaved.  A repetition is CALLS calls
in a row; reported per call:
  wall   host clock around the call (it returns after its stream has been synchronised): what the caller pays
  score  the scoring launches between HIP events (nrtgpu_stats.knn_score_ms with collect_timing: knn_sketch_kernel /
         knn_bytes_kernel / knn_gather_*_kernel; selections, the listing kernel, rescoring and copies are outside it)
as median and spread (max - min) over the five repetitions.  `wins`: the gather median is below the full pass's by more than
twice the larger of the two spreads (wall).  The last lines name, per query count, the crossover and the knob a deployment
should set: the largest swept acceptance at which the gather route won at both query counts, for both element types."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nrtsearch_amd import api   # noqa: E402

ACCEPT = [0.0001, 0.001, 0.01, 0.03, 0.10]
QUERIES = [1, 64]
REPS, F, K = 5, 1, 10


def pack_bits(flags):
    padded = np.zeros(((len(flags) + 63) // 64) * 64, dtype=bool)
    padded[: len(flags)] = flags
    return np.packbits(padded.reshape(-1, 64), axis=1, bitorder="little").view(np.uint64).reshape(-1)


def build(ctx, kind, rows, dim, rng):
    leaves, base, n_leaf = [], 0, rows // 8
    for _ in range(8):
        g = api.GpuSegment(ctx, n_leaf, base)
        if kind == "float":
            g.add_vectors(F, rng.standard_normal((n_leaf, dim), dtype=np.float32))
        else:
            g.add_byte_vectors(F, rng.integers(-128, 128, size=(n_leaf, dim), dtype=np.int8))
        g.seal()
        for mi, share in enumerate(ACCEPT):
            flags = np.zeros(n_leaf, dtype=bool)
            flags[rng.choice(n_leaf, size=max(1, round(n_leaf * share)), replace=False)] = True
            g.set_mask(mi + 1, pack_bits(flags))
        leaves.append(g)
        base += n_leaf
    return leaves


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--calls", type=int, default=10, help="calls per repetition")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# knn gather sweep: {a.rows} rows x {a.dim} dimensions in 8 leaves, k = {K}, {REPS} interleaved repetitions of {a.calls} calls; ms per call")
    say(f"# {'field':5s} {'accept':>7s} {'rows':>7s} {'q':>3s} | {'full wall':>10s} {'spread':>7s} {'score':>7s} | {'gather wall':>11s} {'spread':>7s} {'score':>7s} |"
        f" {'speedup':>7s} {'wins':>4s} | {'gather GB/s':>11s}")
    rng = np.random.default_rng(7)
    won = {}
    for kind in ("float", "byte"):
        ctx = api.GpuContext(device_id=0, max_batch=64, collect_timing=True)
        leaves = build(ctx, kind, a.rows, a.dim, rng)
        sr = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics())
        row_bytes = a.dim * (4 if kind == "float" else 1)
        for nq in QUERIES:
            Q = rng.standard_normal((nq, a.dim), dtype=np.float32) if kind == "float" else rng.integers(-128, 128, size=(nq, a.dim), dtype=np.int8)
            for mi, share in enumerate(ACCEPT):
                flt = api.MaskFilter(mi + 1)

                def call():
                    if kind == "float":
                        return sr.knn_search(F, "dot_product", Q, K, 1.0, flt, 0.0)
                    return sr.knn_search_bytes(F, "dot_product", Q, K, 1.0, flt, 0.0)

                answers = {}
                for knob in (0, 1000):   # warm-up; the routes must agree
                    ctx.set_knn_gather(knob)
                    before = ctx.stats()
                    answers[knob] = call()
                    after = ctx.stats()
                    if knob:
                        accepted = after["knn_rows"] - before["knn_rows"]
                        assert after["knn_sketch_launches"] == before["knn_sketch_launches"], "the request did not take the gather route"
                for x, y in zip(answers[0], answers[1000]):
                    assert x.docs.tolist() == y.docs.tolist() and x.scores.view(np.uint32).tolist() == y.scores.view(np.uint32).tolist()
                wall = {0: [], 1000: []}
                score = {0: [], 1000: []}
                for _ in range(REPS):
                    for knob in (0, 1000):
                        ctx.set_knn_gather(knob)
                        before = ctx.stats()["knn_score_ms"]
                        t0 = time.perf_counter()
                        for _ in range(a.calls):
                            call()
                        wall[knob].append((time.perf_counter() - t0) * 1e3 / a.calls)
                        score[knob].append((ctx.stats()["knn_score_ms"] - before) / a.calls)
                ctx.set_knn_gather(0)
                med = {kb: float(np.median(wall[kb])) for kb in wall}
                spr = {kb: float(np.max(wall[kb]) - np.min(wall[kb])) for kb in wall}
                sc = {kb: float(np.median(score[kb])) for kb in score}
                wins = med[0] - med[1000] > 2.0 * max(spr[0], spr[1000])
                won[(kind, nq, share)] = wins
                gbs = accepted * row_bytes / (sc[1000] * 1e-3) / 1e9 if sc[1000] > 0 else float("nan")
                say(f"  {kind:5s} {share * 100:6.2f}% {accepted:7d} {nq:3d} | {med[0]:10.3f} {spr[0]:7.3f} {sc[0]:7.3f} | {med[1000]:11.3f} {spr[1000]:7.3f} {sc[1000]:7.3f} |"
                    f" {med[0] / med[1000]:6.2f}x {'yes' if wins else 'no':>4s} | {gbs:11.1f}")
        for g in leaves:
            g.release()
        ctx.close()
    say()
    for nq in QUERIES:
        for kind in ("float", "byte"):
            w = [s for s in ACCEPT if won[(kind, nq, s)]]
            lost = [s for s in ACCEPT if not won[(kind, nq, s)]]
            say(f"# {kind}, {nq} quer{'y' if nq == 1 else 'ies'}: gather wins at {', '.join(f'{s * 100:g} %' for s in w) or 'no swept acceptance'}"
                + (f"; the crossover lies below {min(lost) * 100:g} %" if lost else "; no crossover inside the sweep (<= 10 %)"))
    both = [s for s in ACCEPT if all(won[(kind, nq, s)] for kind in ("float", "byte") for nq in QUERIES)]
    prefix = []
    for s in ACCEPT:     # the knob is a ceiling: every acceptance up to it must win
        if s not in both:
            break
        prefix.append(s)
    say(f"# knob for a deployment: {round(max(prefix) * 1000) if prefix else 0} permille"
        + (f" (gather won at both query counts on both element types up to {max(prefix) * 100:g} % acceptance)" if prefix else " (gather did not win at the smallest acceptance)"))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
