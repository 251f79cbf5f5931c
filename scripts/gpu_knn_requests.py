#!/usr/bin/env python3
"""What per-query accept sets cost the filtered knn entry that existed before them, and what a pass of 64 DIFFERENT filters costs
(DESIGN 4.5d).  One GPU visit, two builds side by side:

  search    nrtgpu_knn_search, 64 queries, ONE 25 % filter, on this tree and on a built checkout of the parent commit
            (--parent-root: its nrtsearch_amd package with its libnrtgpu.so), over the same seeded 1 M x 768 rows
  requests  nrtgpu_knn_search_requests, 64 queries with 64 different 25 % filters, this tree's library only
  loop_*    (--closed-loop-s > 0) 64 Python threads, one request each with a filter of its own, in a closed loop for that many
            seconds per repeat: on nrtgpu_knn_search (a pass per request) against nrtgpu_knn_search_coalesced (shared passes).
            Queries/s of PYTHON callers: the interpreter lock serialises everything around the blocking call, so the figure
            bounds what the coalescer gives native request threads from below -- reported, not judged

Every (build, configuration) runs in a worker process of its own with a fresh context (nothing of one configuration -- accept
sets, sketch skips, workspaces -- is there for the next); the orchestrator hands out turns, so the two builds' repeats ALTERNATE
on the device: 5 repeats of 20 calls each, a call timed by the host clock around the blocking entry (it returns after the device
synchronise), a repeat = the median of its calls, a configuration = the median of its repeats.  The margin of the comparison is
the PARENT's own spread (max - min of its 5 repeats): a difference inside it counts as no change.  The two builds' answers are
compared (a checksum over docids and score bits) before anything is timed.  Two PROCESSES of one build differ by more than the
repeats of one process do (where their buffers land): --new-first starts this tree's worker before the parent's, and the record
of every visit is kept -- --out holds {"runs": [...]}, a visit appends to it."""
import argparse
import json
import os
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELD, N_MASKS = 0, 64


def log(*a):
    print(*a, flush=True)


def worker(args):
    """One build, one configuration: upload, warm up, then a repeat per line read from stdin ('go'), a JSON line back."""
    sys.path.insert(0, args.root)   # (the build's own package: its bindings name the symbols its library has)
    import numpy as np
    from nrtsearch_amd import api

    rng = np.random.default_rng(768)
    vecs = rng.standard_normal((args.rows, args.dim), dtype=np.float32)
    queries = rng.standard_normal((64, args.dim), dtype=np.float32)
    ctx = api.GpuContext(0, max_batch=64)
    g = api.GpuSegment(ctx, args.rows, 0)
    g.add_vectors(FIELD, vecs)
    g.seal()
    del vecs
    words = (args.rows + 63) // 64
    for m in range(1, N_MASKS + 1):   # 25 % of the docs each, all different
        bits = np.random.default_rng(1000 + m).random(words * 64) < 0.25
        g.set_mask(m, np.packbits(bits.reshape(-1, 64), axis=1, bitorder="little").view(np.uint64).reshape(-1))
    sr = api.GpuIndexSearcher(ctx, [g], api.IndexStatistics())
    if args.config.startswith("loop_"):
        return closed_loop(args, ctx, g, sr, queries)
    if args.config == "search":
        call = lambda: sr.knn_search(FIELD, "cosine", queries, args.k, filter=api.MaskFilter(1))   # noqa: E731
    else:
        filters = [api.MaskFilter(m) for m in range(1, N_MASKS + 1)]
        call = lambda: sr.knn_search_requests(FIELD, "cosine", queries, [args.k] * 64, None, filters, None)   # noqa: E731
    for _ in range(3):   # the sketch is built, the accept sets are combined, the workspaces are sized
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
    log(json.dumps({"stats": {k: st[k] for k in ("knn_panels", "knn_score_launches", "knn_sketch_launches", "knn_second_passes", "knn_rows")}}))
    g.release()
    ctx.close()


def closed_loop(args, ctx, g, sr, queries):
    import threading
    import numpy as np
    from nrtsearch_amd import api
    entry = sr.knn_search_coalesced if args.config == "loop_coalesced" else \
        (lambda f, s, q, k, filter=None: sr.knn_search(f, s, q, k, filter=filter)[0])
    for i in range(4):
        entry(FIELD, "cosine", queries[i], args.k, filter=api.MaskFilter(i + 1))
    ctx.reset_stats()
    log(json.dumps({"ready": True, "crc": 0}))
    for line in sys.stdin:
        if line.strip() != "go":
            break
        done, errors = [0] * 64, []
        t_end = time.perf_counter() + args.closed_loop_s

        def caller(i):
            try:
                while time.perf_counter() < t_end:
                    entry(FIELD, "cosine", queries[i], args.k, filter=api.MaskFilter(i + 1))
                    done[i] += 1
            except Exception as e:   # noqa: BLE001
                errors.append(repr(e))

        t0 = time.perf_counter()
        threads = [threading.Thread(target=caller, args=(i,)) for i in range(64)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        if errors:
            raise SystemExit(errors[0])
        log(json.dumps({"ms": 0.0, "qps": sum(done) / (time.perf_counter() - t0)}))
    st = ctx.stats()
    log(json.dumps({"stats": {k: st[k] for k in ("knn_panels", "knn_score_launches", "knn_sketch_launches", "knn_second_passes", "knn_rows")}}))
    g.release()
    ctx.close()


class Worker:
    def __init__(self, args, root, config):
        self.name = config
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--config", config, "--rows", str(args.rows),
               "--dim", str(args.dim), "--k", str(args.k), "--calls", str(args.calls), "--closed-loop-s", str(args.closed_loop_s)]
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
        self.last = self.read()
        return self.last["ms"]

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
    ap.add_argument("--parent-root", help="a checkout of the parent commit with its library built (nrtsearch_amd/libnrtgpu.so)")
    ap.add_argument("--root", default=ROOT, help="(worker) the tree whose package and library it loads")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--closed-loop-s", type=float, default=0.0, help="seconds per repeat of the closed loop of 64 Python threads (0: skip)")
    ap.add_argument("--new-first", action="store_true", help="start (and time) this tree's worker before the parent's")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_requests_ab.json"))
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--config", default="search")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    if not args.parent_root or not os.path.exists(os.path.join(args.parent_root, "nrtsearch_amd", "libnrtgpu.so")):
        raise SystemExit("--parent-root: a built checkout of the parent commit is needed for the comparison")
    # one worker at a time is started (each uploads the rows); then the two builds take turns
    if args.new_first:
        new = Worker(args, ROOT, "search")
        parent = Worker(args, os.path.abspath(args.parent_root), "search")
    else:
        parent = Worker(args, os.path.abspath(args.parent_root), "search")
        new = Worker(args, ROOT, "search")
    if parent.ready["crc"] != new.ready["crc"]:
        raise SystemExit(f"the two builds answer differently: {parent.ready} / {new.ready}")
    reps_parent, reps_new = [], []
    for _ in range(args.repeats):
        if args.new_first:
            reps_new.append(new.repeat())
        reps_parent.append(parent.repeat())
        if not args.new_first:
            reps_new.append(new.repeat())
    stats_parent, stats_new = parent.close(), new.close()
    req = Worker(args, ROOT, "requests")
    reps_req = [req.repeat() for _ in range(args.repeats)]
    stats_req = req.close()
    res = {"started_first": "new" if args.new_first else "parent", "rows": args.rows, "dim": args.dim, "queries": 64, "k": args.k, "calls_per_repeat": args.calls,
           "knn_search_one_filter_parent": summary(reps_parent), "knn_search_one_filter": summary(reps_new),
           "knn_search_requests_64_filters": summary(reps_req),
           "same_answers": True, "launches": {"parent": stats_parent, "new": stats_new, "requests": stats_req}}
    diff = res["knn_search_one_filter"]["median_ms"] - res["knn_search_one_filter_parent"]["median_ms"]
    res["difference_ms"] = diff
    res["inside_parent_spread"] = abs(diff) <= res["knn_search_one_filter_parent"]["spread_ms"]
    if args.closed_loop_s > 0:
        loops = {"loop_search": Worker(args, ROOT, "loop_search"), "loop_coalesced": Worker(args, ROOT, "loop_coalesced")}
        qps = {name: [] for name in loops}
        for _ in range(3):
            for name, w in loops.items():
                w.repeat()
                qps[name].append(w.last["qps"])
        res["closed_loop_64_python_threads"] = {
            "what": "queries/s, 64 Python threads with a 25 % filter each; bounded by the interpreter lock around the blocking calls",
            "seconds_per_repeat": args.closed_loop_s,
            "knn_search_qps": sorted(qps["loop_search"])[1], "knn_search_coalesced_qps": sorted(qps["loop_coalesced"])[1],
            "repeats_qps": qps, "launches": {name: w.close() for name, w in loops.items()}}
    runs = json.load(open(args.out))["runs"] if os.path.exists(args.out) else []
    with open(args.out, "w") as f:
        json.dump({"runs": runs + [res]}, f, indent=1)
        f.write("\n")
    log(json.dumps(res))


if __name__ == "__main__":
    main()
