#!/usr/bin/env python3
"""What a pass of 64 knn requests with 64 DIFFERENT filters costs over a byte (int8) field, against the same 64 requests sent one
by one.  Modelled on scripts/gpu_knn_requests.py.  One GPU visit:

  requests  nrtgpu_knn_search_bytes_requests: 64 queries with 64 different 25 % filters in ONE call
  singles   the same 64 requests as 64 calls of nrtgpu_knn_search_bytes (what a deployment paid before), same build
  search    (--parent-root only) nrtgpu_knn_search_bytes, 64 queries, ONE 25 % filter, on this tree and on a built checkout of the
            parent commit.  This leg is needed only when the disassembly of knn_bytes_kernel's instantiations differs from the
            parent's; when it is identical the old entries launch the same machine code and the leg is skipped and recorded as
            "not measured"

Every configuration runs in a worker process of its own with a fresh context over the same seeded 1 M x 768 int8 rows; the
orchestrator hands out turns, so the configurations' repeats ALTERNATE on the device: 5 repeats, a call timed by the host clock
around the blocking entry (it returns after the device synchronise), a repeat = the median of its calls (`singles`: of the sum of
its 64 calls), a configuration = the median of its repeats, its spread = max - min of its repeats.  Before anything is timed the
answers of `requests` and `singles` are compared (a checksum over docids and score bits: they must be the same bits).  --out holds
{"runs": [...]}, a visit appends to it."""
import argparse
import json
import os
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELD, N_MASKS = 0, 64
STATS = ("knn_panels", "knn_score_launches", "knn_sketch_launches", "knn_second_passes", "knn_rows")


def log(*a):
    print(*a, flush=True)


def worker(args):
    """One build, one configuration: upload, warm up, then a repeat per line read from stdin ('go'), a JSON line back."""
    sys.path.insert(0, args.root)   # (the build's own package: its bindings name the symbols its library has)
    import numpy as np
    from nrtsearch_amd import api

    rng = np.random.default_rng(768)
    rows = rng.integers(-128, 128, size=(args.rows, args.dim), dtype=np.int8)
    queries = rng.integers(-128, 128, size=(64, args.dim), dtype=np.int8)
    ctx = api.GpuContext(0, max_batch=64)
    g = api.GpuSegment(ctx, args.rows, 0)
    g.add_byte_vectors(FIELD, rows)
    g.seal()
    del rows
    words = (args.rows + 63) // 64
    for m in range(1, N_MASKS + 1):   # 25 % of the docs each, all different
        bits = np.random.default_rng(1000 + m).random(words * 64) < 0.25
        g.set_mask(m, np.packbits(bits.reshape(-1, 64), axis=1, bitorder="little").view(np.uint64).reshape(-1))
    sr = api.GpuIndexSearcher(ctx, [g], api.IndexStatistics())
    filters = [api.MaskFilter(m) for m in range(1, N_MASKS + 1)]
    if args.config == "search":
        call = lambda: sr.knn_search_bytes(FIELD, "cosine", queries, args.k, filter=filters[0])   # noqa: E731
    elif args.config == "requests":
        call = lambda: sr.knn_search_bytes_requests(FIELD, "cosine", queries, [args.k] * 64, None, filters, None)   # noqa: E731
    else:
        call = lambda: [sr.knn_search_bytes(FIELD, "cosine", queries[i], args.k, filter=filters[i])[0] for i in range(64)]   # noqa: E731
    for _ in range(3):   # the accept sets are combined, the workspaces are sized, the code objects are loaded
        got = call()
    crc = 0
    for td in got:
        crc = zlib.crc32(td.scores.view(np.uint32).tobytes(), zlib.crc32(td.docs.tobytes(), crc))
    ctx.reset_stats()
    log(json.dumps({"ready": True, "crc": crc, "hits": int(sum(len(td.docs) for td in got))}))
    for line in sys.stdin:
        if line.strip() != "go":
            break
        ms = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            call()
            ms.append((time.perf_counter() - t0) * 1e3)
        log(json.dumps({"ms": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}))
    st = ctx.stats()
    log(json.dumps({"stats": {k: st[k] for k in STATS}}))
    g.release()
    ctx.close()


class Worker:
    def __init__(self, args, root, config):
        self.name = config
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--config", config, "--rows", str(args.rows),
               "--dim", str(args.dim), "--k", str(args.k), "--calls", str(args.calls)]
        self.p = subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        self.ready = self.read()

    def read(self):
        line = self.p.stdout.readline()
        if not line:
            raise SystemExit(f"worker {self.name} ended (exit {self.p.wait()}): nothing more is started")
        return json.loads(line)

    def repeat(self):
        self.p.stdin.write("go\n")
        self.p.stdin.flush()
        return self.read()["ms"]

    def close(self):
        self.p.stdin.close()
        stats = self.read()["stats"]
        if self.p.wait() != 0:
            raise SystemExit(f"worker {self.name} exit {self.p.returncode}")
        return stats


def summary(reps):
    s = sorted(reps)
    return {"median_ms": s[len(s) // 2], "spread_ms": s[-1] - s[0], "repeats_ms": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", help="a checkout of the parent commit with its library built: adds the `search` leg (only needed when "
                                          "the disassembly of knn_bytes_kernel differs from the parent's)")
    ap.add_argument("--root", default=ROOT, help="(worker) the tree whose package and library it loads")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_byte_requests_ab.json"))
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--config", default="requests")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    # one worker at a time is started (each uploads the rows); then the configurations take turns
    req, one = Worker(args, ROOT, "requests"), Worker(args, ROOT, "singles")
    if req.ready != one.ready:
        raise SystemExit(f"one call of 64 requests and 64 calls answer differently: {req.ready} / {one.ready}")
    reps_req, reps_one = [], []
    for _ in range(args.repeats):
        reps_one.append(one.repeat())
        reps_req.append(req.repeat())
    stats_req, stats_one = req.close(), one.close()
    res = {"rows": args.rows, "dim": args.dim, "queries": 64, "k": args.k, "similarity": "cosine", "calls_per_repeat": args.calls,
           "requests_64_filters_one_call": summary(reps_req), "the_same_as_64_knn_search_bytes_calls": summary(reps_one),
           "same_answers": True, "hits": req.ready["hits"], "launches": {"requests": stats_req, "singles": stats_one}}
    res["speedup"] = res["the_same_as_64_knn_search_bytes_calls"]["median_ms"] / res["requests_64_filters_one_call"]["median_ms"]
    if args.parent_root:
        if not os.path.exists(os.path.join(args.parent_root, "nrtsearch_amd", "libnrtgpu.so")):
            raise SystemExit("--parent-root: a built checkout of the parent commit is needed for the comparison")
        parent, new = Worker(args, os.path.abspath(args.parent_root), "search"), Worker(args, ROOT, "search")
        if parent.ready != new.ready:
            raise SystemExit(f"the two builds answer differently: {parent.ready} / {new.ready}")
        reps_parent, reps_new = [], []
        for _ in range(args.repeats):
            reps_parent.append(parent.repeat())
            reps_new.append(new.repeat())
        res["launches"].update(parent=parent.close(), new=new.close())
        res["knn_search_bytes_one_filter_parent"], res["knn_search_bytes_one_filter"] = summary(reps_parent), summary(reps_new)
        diff = res["knn_search_bytes_one_filter"]["median_ms"] - res["knn_search_bytes_one_filter_parent"]["median_ms"]
        res["difference_ms"] = diff
        res["inside_parent_spread"] = abs(diff) <= res["knn_search_bytes_one_filter_parent"]["spread_ms"]
    else:
        res["knn_search_bytes_one_filter_parent_vs_new"] = ("not measured: the instantiations of knn_bytes_kernel are, instruction for "
                                                            "instruction, the parent's (DESIGN 4.5e), so the old entries launch the same code")
    runs = json.load(open(args.out))["runs"] if os.path.exists(args.out) else []
    with open(args.out, "w") as f:
        json.dump({"runs": runs + [res]}, f, indent=1)
        f.write("\n")
    log(json.dumps(res))


if __name__ == "__main__":
    main()
