"""Host time of the Python binding alone (nrtsearch_amd/api.py), this tree's beside another commit's: no GPU, no built library.

The library is the recorder of tests/test_api_calls_host.py with its recording switched off (every entry returns NRTGPU_OK at once), so
what is timed is the marshalling, the output arrays and the TopDocs lists.  Per shape: the median of 2000 calls, five repeats; inside a
repeat the two bindings take turns call by call, so both see the same machine.

    python scripts/api_wrapper_ab.py <a directory holding the other commit's nrtsearch_amd/*.py> profiles/api_wrapper_ab.json
"""
import ctypes as C
import importlib.util
import json
import os
import statistics
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.test_api_calls_host import Recorder   # noqa: E402

CALLS, REPEATS = 2000, 5


class Quiet(Recorder):
    def _call(self, entry, args):
        return 0


def binding(directory: str, name: str):
    """The api module of the nrtsearch_amd package in `directory`, imported as package `name`, over a library that returns at once."""
    path = os.path.join(directory, "nrtsearch_amd")
    spec = importlib.util.spec_from_file_location(name, os.path.join(path, "__init__.py"), submodule_search_locations=[path])
    sys.modules[name] = pkg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pkg)
    api = importlib.import_module(name + ".api")
    quiet = Quiet()
    sys.modules[name + "._lib"].load = lambda: quiet
    return api


def shapes(api):
    stats = api.IndexStatistics()
    stats.fields[0] = api.CollectionStatistics(1000, 50000)
    stats.doc_freq.update({(0, t): 10 + t for t in range(8)})
    ctx = types.SimpleNamespace(_h=C.c_void_p(0x1000))
    leaves = [types.SimpleNamespace(_h=C.c_void_p(0x2000 + 16 * i), doc_base=500 * i) for i in range(2)]
    sr = api.GpuIndexSearcher(ctx, leaves, stats)
    qv = np.random.default_rng(5).standard_normal((64, 128)).astype(np.float32)
    out = {"knn_exact 64 x k 10": lambda: sr.knn_exact(5, "cosine", qv, 10)}
    for n in (64, 256):
        queries = [api.BooleanQuery(tuple(api.TermQuery(0, (qi + j) % 8) for j in range(3))) for qi in range(n)]
        managers = [api.TopScoreDocCollectorManager(10)] * n
        fsq = [api.FunctionScoreQuery(q, (api.WeightFunction(2.0, 3),)) for q in queries]
        out[f"search_batch {n} x num_hits 10"] = lambda queries=queries, managers=managers: sr.search_batch(queries, managers)
        out[f"search_function_score_batch {n} x num_hits 10"] = lambda fsq=fsq, managers=managers: sr.search_function_score_batch(fsq, managers)
    return out


def main():
    other, path = sys.argv[1], sys.argv[2]
    sides = {"parent": shapes(binding(other, "nrtsearch_amd_parent")), "tree": shapes(binding(ROOT, "nrtsearch_amd_tree"))}
    out = {"method": f"scripts/api_wrapper_ab.py: the two bindings over a library stand-in that returns at once, one CPU process; per shape the median of "
                     f"{CALLS} calls, {REPEATS} repeats, the bindings taking turns call by call; microseconds per call",
           "rule": "the tree's median (of its repeats' medians) may exceed the parent's by no more than max - min of the parent's repeats"}
    for name in sides["tree"]:
        repeats = {side: [] for side in sides}
        for fn in (sides["parent"][name], sides["tree"][name]):
            for _ in range(50):
                fn()
        for _ in range(REPEATS):
            t = {side: [] for side in sides}
            for _ in range(CALLS):
                for side in sides:
                    fn = sides[side][name]
                    t0 = time.perf_counter_ns()
                    fn()
                    t[side].append(time.perf_counter_ns() - t0)
            for side in sides:
                repeats[side].append(round(statistics.median(t[side]) / 1e3, 2))
        p, tr = statistics.median(repeats["parent"]), statistics.median(repeats["tree"])
        spread = round(max(repeats["parent"]) - min(repeats["parent"]), 2)
        out[name] = {"parent_repeat_medians_us": repeats["parent"], "tree_repeat_medians_us": repeats["tree"], "parent_us": p, "tree_us": tr,
                     "parent_spread_us": spread, "within_rule": tr <= p + spread}
        print(name, out[name], flush=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
