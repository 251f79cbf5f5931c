"""Which refusal wins: the twelve vector entries of the C ABI (the five exact / knn request searches over a float field, their five
twins over a byte field, the two two-call rescorers) handed every single bad argument they refuse and every pair of two at once,
through ctypes -- not through api.py's own checks.  Per case the return code and nrtgpu_last_error() must equal the line of
tests/golden/knn_refusals.txt, which was recorded from the library as it was BEFORE the vector entries shared one call description,
one leaf walk and one field check (the recording command is the golden's first line): the entries differ in the order of their
checks and in some texts, and those differences are part of the ABI's behaviour.

The cases are the golden's: a bad argument that an entry does not refuse (a negative boost of nrtgpu_knn_exact) has no line there.
Fixture: two sealed leaves of 64 rows, both with a float field and a byte field of 24 dimensions; mask 1 is set on leaf 0 only."""
import ctypes as C
import functools
import itertools
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "knn_refusals.txt")
ROWS, DIM, FF, FB, NQ, MAX_K = 64, 24, 1, 2, 3, 1024

SEARCH = ("ctx", "segs", "bases", "n_segs", "field", "sim", "queries", "n_queries", "dim", "k", "boost")
COALESCED = ("ctx", "segs", "bases", "n_segs", "field", "sim", "queries", "dim", "k", "boost")
RESCORE = ("ctx", "segs", "bases", "n_segs", "field", "sim", "queries", "dim", "boost", "docs", "first", "n", "qw", "rw", "window", "out")
SHAPES = {
    "knn_exact": SEARCH + ("out",),
    "knn_search": SEARCH + ("mask", "min_score", "out"),
    "knn_search_requests": SEARCH[:-2] + ("ks", "boosts", "masks", "min_scores", "out"),
    "knn_exact_coalesced": COALESCED + ("out",),
    "knn_search_coalesced": COALESCED + ("mask", "min_score", "out"),
    "rescore_vectors": RESCORE,
}
# entry -> (its shape, a byte entry)
ENTRIES = {
    "nrtgpu_knn_exact": ("knn_exact", False), "nrtgpu_knn_search": ("knn_search", False),
    "nrtgpu_knn_search_requests": ("knn_search_requests", False), "nrtgpu_knn_exact_coalesced": ("knn_exact_coalesced", False),
    "nrtgpu_knn_search_coalesced": ("knn_search_coalesced", False),
    "nrtgpu_knn_exact_bytes": ("knn_exact", True), "nrtgpu_knn_search_bytes": ("knn_search", True),
    "nrtgpu_knn_search_bytes_requests": ("knn_search_requests", True), "nrtgpu_knn_exact_bytes_coalesced": ("knn_exact_coalesced", True),
    "nrtgpu_knn_search_bytes_coalesced": ("knn_search_coalesced", True),
    "nrtgpu_rescore_vectors": ("rescore_vectors", False), "nrtgpu_rescore_byte_vectors": ("rescore_vectors", True),
}
# case -> (the argument it spoils, the bad value).  The per-request arrays of the requests entries take the value for member 1 of 3.
NULL = object()
CASES = {
    "ctx_null": ("ctx", NULL), "segs_null": ("segs", NULL), "queries_null": ("queries", NULL), "out_null": ("out", NULL),
    "bases_null": ("bases", NULL), "docs_null": ("docs", NULL), "first_null": ("first", NULL), "ks_null": ("k", NULL),
    "n_queries_0": ("n_queries", 0), "n_queries_neg": ("n_queries", -1), "n_segs_neg": ("n_segs", -1), "n_neg": ("n", -1),
    "window_0": ("window", 0),
    "k_0": ("k", 0), "k_over": ("k", MAX_K + 1),
    "dim_0": ("dim", 0), "dim_2049": ("dim", 2049), "dim_25": ("dim", 25),
    "sim_4": ("sim", 4),
    "boost_neg": ("boost", -1.0), "boost_nan": ("boost", math.nan), "boost_inf": ("boost", math.inf),
    "mask_neg": ("mask", -1), "mask_1": ("mask", 1), "mask_77": ("mask", 77),
    "min_score_neg": ("min_score", -0.5), "min_score_nan": ("min_score", math.nan),
    "zero_query": ("queries", 0),
    "other_type": ("field", "other"),
}
ARG_OF = {"k": ("k", "ks"), "boost": ("boost", "boosts"), "mask": ("mask", "masks"), "min_score": ("min_score", "min_scores")}


def applies(case, shape):
    arg = CASES[case][0]
    if case == "ks_null":
        return "ks" in SHAPES[shape]
    if case == "bases_null":
        return shape == "rescore_vectors"   # (the searches take NULL doc bases: zeros)
    return any(a in SHAPES[shape] for a in ARG_OF.get(arg, (arg,)))


@functools.lru_cache(maxsize=None)
def cases_of(entry):
    """Every single bad argument of the entry, then every pair that spoils two different arguments."""
    shape = ENTRIES[entry][0]
    singles = [c for c in CASES if applies(c, shape)]
    return [(c,) for c in singles] + [p for p in itertools.combinations(singles, 2) if CASES[p[0]][0] != CASES[p[1]][0]]


class Fixture:
    def __init__(self):
        from nrtsearch_amd import _lib, api
        self.lib, self.api = _lib.load(), api
        rng = np.random.default_rng(17)
        self.ctx = api.GpuContext(device_id=0, max_batch=8)
        self.leaves = []
        for i in range(2):
            g = api.GpuSegment(self.ctx, ROWS, i * ROWS)
            g.add_vectors(FF, rng.standard_normal((ROWS, DIM)).astype(np.float32))
            g.add_byte_vectors(FB, rng.integers(-128, 128, size=(ROWS, DIM), dtype=np.int8))
            if i == 0:
                g.set_mask(1, np.full(1, 0x5555555555555555, dtype=np.uint64))
            g.seal()
            self.leaves.append(g)
        self.sr = api.GpuIndexSearcher(self.ctx, self.leaves, api.IndexStatistics())
        # (room for the largest dimension and count a case names: a refusal must not depend on what lies behind a short buffer)
        self.qf = rng.standard_normal((NQ, 2049)).astype(np.float32)
        self.qb = rng.integers(1, 128, size=(NQ, 2049), dtype=np.int8)
        self.zf, self.zb = np.zeros_like(self.qf), np.zeros_like(self.qb)
        self.docs, self.first = np.array([1, ROWS + 6], np.int32), np.array([2.0, 1.0], np.float32)
        self.outs = (_lib.TopDocs * NQ)()
        self.od, self.os = np.zeros((NQ, 16), np.int32), np.zeros((NQ, 16), np.float32)
        for q in range(NQ):
            self.outs[q].capacity = 16
            self.outs[q].docs = C.cast(self.od.ctypes.data + q * 64, C.POINTER(C.c_int32))
            self.outs[q].scores = C.cast(self.os.ctypes.data + q * 64, C.POINTER(C.c_float))

    def close(self):
        for g in self.leaves:
            g.release()
        self.ctx.close()

    def call(self, entry, case):
        shape, byte = ENTRIES[entry]
        v = {"ctx": self.ctx._h, "segs": self.sr._segs, "bases": self.sr._bases, "n_segs": 2, "field": FB if byte else FF, "sim": 0,
             "queries": (self.qb if byte else self.qf).ctypes.data, "n_queries": NQ, "dim": DIM, "k": 5, "boost": 1.0, "mask": 0,
             "min_score": 0.0, "out": self.outs, "docs": self.docs.ctypes.data, "first": self.first.ctypes.data, "n": 2, "qw": 1.0,
             "rw": 2.0, "window": 2}
        for c in case:
            arg, bad = CASES[c]
            if bad is NULL:
                bad = None
            elif c == "zero_query":
                bad = (self.zb if byte else self.zf).ctypes.data
            elif c == "other_type":
                bad = FF if byte else FB
            v[arg] = bad
        keep = []   # (the per-request arrays live until the call has returned)
        args = []
        for a in SHAPES[shape]:
            if a in ("ks", "boosts", "masks", "min_scores"):
                one = v[{"ks": "k", "boosts": "boost", "masks": "mask", "min_scores": "min_score"}[a]]
                if one is None:
                    args.append(None)
                    continue
                good = {"ks": 5, "boosts": 1.0, "masks": 0, "min_scores": 0.0}[a]
                arr = np.array([good, one, good], np.int32 if a in ("ks", "masks") else np.float32)
                keep.append(arr)
                args.append(arr.ctypes.data)
            elif a in ("boost", "min_score"):
                args.append(C.c_float(v[a]))
            elif a in ("qw", "rw"):
                args.append(C.c_double(v[a]))
            else:
                args.append(v[a])
        rc = int(getattr(self.lib, entry)(*args))
        return rc, (self.lib.nrtgpu_last_error() or b"").decode() if rc else ""


def line_of(entry, case, rc, err):
    return f"{entry} {'+'.join(case)} {rc} {err}"


def record(path, command):
    fx = Fixture()
    lines, passed = [f"# recorded from the commit before the vector host path was taken apart: {command}"], []
    for entry in ENTRIES:
        refused = set()
        for case in cases_of(entry):
            if len(case) == 2 and not (case[0] in refused and case[1] in refused):
                continue   # (an argument the entry does not refuse alone: no case)
            rc, err = fx.call(entry, case)
            if rc == 0:
                passed.append(line_of(entry, case, rc, ""))
                continue
            if len(case) == 1:
                refused.add(case[0])
            lines.append(line_of(entry, case, rc, err))
    fx.close()
    open(path, "w").write("\n".join(lines) + "\n")
    print(f"{len(lines) - 1} refusals recorded; not refused: {len(passed)}")
    for l in passed:
        print("  ", l)


@pytest.mark.gpu
def test_every_entry_refuses_what_it_refused_with_the_same_code_and_text():
    want = [l for l in open(GOLDEN).read().split("\n") if l and not l.startswith("#")]
    assert len(want) > 1000 and {l.split(" ", 1)[0] for l in want} == set(ENTRIES)
    fx = Fixture()
    try:
        wrong = []
        for w in want:
            entry, names, _ = w.split(" ", 2)
            case = tuple(names.split("+"))
            assert case in cases_of(entry), w
            got = line_of(entry, case, *fx.call(entry, case))
            if got != w:
                wrong.append((got, w))
    finally:
        fx.close()
    assert not wrong, f"{len(wrong)} of {len(want)} cases differ; the first (got, recorded): {wrong[:5]}"


if __name__ == "__main__":
    # NRTGPU_LIB_PATH=<the parent commit's libnrtgpu.so> python tests/test_knn_refusals_gpu.py --record tests/golden/knn_refusals.txt
    assert len(sys.argv) == 3 and sys.argv[1] == "--record"
    record(sys.argv[2], "NRTGPU_LIB_PATH=<libnrtgpu.so built from that commit> python tests/test_knn_refusals_gpu.py --record tests/golden/knn_refusals.txt")
