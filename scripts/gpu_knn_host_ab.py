#!/usr/bin/env python3
"""Host time per pass of the knn request entries, this tree's library against another build of the same kernels (the parent
commit's: --parent-lib), for changes to the vector HOST path that leave the device code alone.  Shapes as in
scripts/gpu_knn_requests.py and scripts/gpu_knn_byte_requests.py: 1 M x 768 rows (fp32 / int8), cosine, k = 100, 64 masks of 25 %.

  search_1      nrtgpu_knn_search(_bytes), ONE query per call, one 25 % filter -- where a pass's staging dominates
  search_64     the same with 64 queries per call
  requests_64   nrtgpu_knn_search(_bytes)_requests, 64 queries with 64 different filters in one call

One worker process per (library, element type) keeps its rows resident; the orchestrator hands out turns, so the two libraries'
rounds ALTERNATE on the device (which goes first alternates too): --rounds rounds of --calls calls, a call timed by the host clock
around the blocking entry, a round = the median of its calls.  The tree passes a configuration if the median of its rounds lies
inside the range (min .. max) of the parent's own rounds.  The two libraries' answers are compared (a checksum over docids and
score bits) before anything is timed.  Two PROCESSES of one library differ by more than the rounds of one process do (where their
buffers land: scripts/gpu_knn_requests.py): --tree-first starts this tree's workers before the parent's, and a difference that
changes sign with the order of the start is the processes', not the libraries'.  --out holds {"runs": [...]}, a visit appends to it."""
import argparse
import json
import os
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELD, N_MASKS = 0, 64
CONFIGS = ("search_1", "search_64", "requests_64")


def log(*a):
    print(*a, flush=True)


def worker(args):
    sys.path.insert(0, ROOT)
    import numpy as np
    from nrtsearch_amd import api

    rng = np.random.default_rng(768)
    ctx = api.GpuContext(0, max_batch=64)
    g = api.GpuSegment(ctx, args.rows, 0)
    if args.bytes:
        g.add_byte_vectors(FIELD, rng.integers(-128, 128, size=(args.rows, args.dim), dtype=np.int8))
        queries = rng.integers(-128, 128, size=(64, args.dim), dtype=np.int8)
    else:
        g.add_vectors(FIELD, rng.standard_normal((args.rows, args.dim), dtype=np.float32))
        queries = rng.standard_normal((64, args.dim), dtype=np.float32)
    g.seal()
    words = (args.rows + 63) // 64
    for m in range(1, N_MASKS + 1):   # 25 % of the docs each, all different
        bits = np.random.default_rng(1000 + m).random(words * 64) < 0.25
        g.set_mask(m, np.packbits(bits.reshape(-1, 64), axis=1, bitorder="little").view(np.uint64).reshape(-1))
    sr = api.GpuIndexSearcher(ctx, [g], api.IndexStatistics())
    search = sr.knn_search_bytes if args.bytes else sr.knn_search
    requests = sr.knn_search_bytes_requests if args.bytes else sr.knn_search_requests
    filters = [api.MaskFilter(m) for m in range(1, N_MASKS + 1)]
    calls = {"search_1": lambda: search(FIELD, "cosine", queries[:1], args.k, filter=filters[0]),
             "search_64": lambda: search(FIELD, "cosine", queries, args.k, filter=filters[0]),
             "requests_64": lambda: requests(FIELD, "cosine", queries, [args.k] * 64, None, filters, None)}
    crc = {}
    for name, call in calls.items():   # the sketch is built, the accept sets are combined, the workspaces are sized
        for _ in range(3):
            got = call()
        c = 0
        for td in got:
            c = zlib.crc32(td.scores.view(np.uint32).tobytes(), zlib.crc32(td.docs.tobytes(), c))
        crc[name] = c
    log(json.dumps({"ready": True, "crc": crc}))
    for line in sys.stdin:
        call = calls.get(line.strip())
        if call is None:
            break
        ms = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            call()
            ms.append((time.perf_counter() - t0) * 1e3)
        log(json.dumps({"ms": float(np.median(ms))}))
    g.release()
    ctx.close()


class Worker:
    def __init__(self, args, lib, bytes_):
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--rows", str(args.rows), "--dim", str(args.dim), "--k", str(args.k),
               "--calls", str(args.calls)] + (["--bytes"] if bytes_ else [])
        env = dict(os.environ)
        env.pop("NRTGPU_LIB_PATH", None)
        if lib:
            env["NRTGPU_LIB_PATH"] = os.path.abspath(lib)
        self.p = subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=env)
        self.ready = self.read()

    def read(self):
        line = self.p.stdout.readline()
        if not line:
            raise SystemExit(f"a worker ended (exit {self.p.wait()}): nothing more is started")
        return json.loads(line)

    def round(self, config):
        self.p.stdin.write(config + "\n")
        self.p.stdin.flush()
        return self.read()["ms"]

    def close(self):
        self.p.stdin.close()
        if self.p.wait() != 0:
            raise SystemExit(f"a worker exited with {self.p.returncode}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libnrtgpu.so built from the parent commit")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_host_refactor_ab.json"))
    ap.add_argument("--tree-first", action="store_true", help="start this tree's workers before the parent's")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--bytes", action="store_true")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        raise SystemExit("--parent-lib: the parent commit's library is needed for the comparison")
    res = {"started_first": "tree" if args.tree_first else "parent", "rows": args.rows, "dim": args.dim, "k": args.k, "calls_per_round": args.calls, "rounds": args.rounds, "configurations": {}}
    for bytes_ in (False, True):
        if args.tree_first:   # (one worker at a time is started: each uploads the rows)
            tree, parent = Worker(args, None, bytes_), Worker(args, args.parent_lib, bytes_)
        else:
            parent, tree = Worker(args, args.parent_lib, bytes_), Worker(args, None, bytes_)
        if parent.ready["crc"] != tree.ready["crc"]:
            raise SystemExit(f"the two libraries answer differently: {parent.ready} / {tree.ready}")
        for config in CONFIGS:
            ms = {"parent": [], "tree": []}
            for r in range(args.rounds):
                for who in (("parent", "tree") if (r % 2 == 0) != args.tree_first else ("tree", "parent")):
                    ms[who].append((parent if who == "parent" else tree).round(config))
            med = sorted(ms["tree"])[len(ms["tree"]) // 2]
            res["configurations"][("byte_" if bytes_ else "float_") + config] = {
                "parent_rounds_ms": ms["parent"], "tree_rounds_ms": ms["tree"], "parent_median_ms": sorted(ms["parent"])[len(ms["parent"]) // 2],
                "tree_median_ms": med, "inside_parent_range": min(ms["parent"]) <= med <= max(ms["parent"])}
        parent.close()
        tree.close()
    res["same_answers"] = True
    runs = json.load(open(args.out))["runs"] if os.path.exists(args.out) else []
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"runs": runs + [res]}, f, indent=1)
        f.write("\n")
    log(json.dumps(res))


if __name__ == "__main__":
    main()
