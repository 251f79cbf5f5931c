"""A function score over a multi-match query without a GPU: the arithmetic the kernel compiles
(nrtgpu_function_score_multi_match_value == plan.h: multi_match_group / multi_match_fold / multi_match_value, then
function_score_value) against the NumPy reference's per-doc rule, the reference itself against the two references it is built on
where it degenerates to one of them, the refusals (those that need a context against the stand-in runtime of tests/mockhip), and
the condition on the GPU tests' inputs that the composition is observable."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from nrtsearch_amd import _lib, build

from tests import _function_score_multi_match_ref as ref
from tests import _function_score_ref as fs_ref
from tests import _multi_match_ref as mm_ref
from tests.test_function_score_host import _fs
from tests.test_multi_match_host import _groups, _same, _score_pool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
INV, UNS = _lib.NRTGPU_ERR_INVALID_ARG, _lib.NRTGPU_ERR_UNSUPPORTED
MODE_PAIRS = [(s, b) for s in ("multiply", "sum") for b in ("multiply", "sum", "replace")]
TOKENS = (2, 4, 7)
FUNCTIONS = ((7, 1.5), (9, 3.0), (0, 0.5))


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _value(lib, g, scores, matched, fs, matched_functions, occur=None, msm=0, n_terms=None):
    sc = np.ascontiguousarray(scores, dtype=f32)
    oc = None if occur is None else np.ascontiguousarray(occur, dtype=np.int32)
    score, hit = C.c_float(0), C.c_int32(-1)
    rc = lib.nrtgpu_function_score_multi_match_value(C.byref(g), len(sc) if n_terms is None else n_terms, None if oc is None else oc.ctypes.data,
                                                     int(msm), sc.ctypes.data, int(matched), C.byref(fs), int(matched_functions),
                                                     C.byref(score), C.byref(hit))
    return rc, f32(score.value), hit.value


def test_value_is_the_reference_rule(lib):
    """Both shapes, 1..8 groups, 0..8 functions, every score_mode x boost_mode; min_score 0, and at the final score of one of the docs
    with min_excluded 0 and 1; docs the groups reject stay no hits whatever the functions say."""
    rng = np.random.default_rng(177)
    ties = [0.0, 1.0, 0.3, float(np.nextafter(f32(1), f32(0)))]
    weights_pool = [0.25, 0.5, 1.25, 1.5, 2.5, 3.0, 11.0, 1.0 + 2.0 ** -23, 0.1]
    n_docs, checked, rejected, boundary = 16, 0, 0, 0
    for shape in ("cross_fields", "best_fields"):
        best = shape == "best_fields"
        for n_groups in range(1, 9):
            for n_functions in range(0, 9):
                n_clauses = int(rng.integers(n_groups, min(32, 3 * n_groups) + 1))
                group_of = list(range(n_groups)) + rng.integers(0, n_groups, n_clauses - n_groups).tolist()
                rng.shuffle(group_of)
                sizes = [group_of.count(g) for g in range(n_groups)]
                scores = _score_pool(rng, n_clauses * n_docs).reshape(n_clauses, n_docs)
                matched = rng.random((n_clauses, n_docs)) < rng.choice([0.4, 0.8])
                weights = [float(f32(w)) for w in rng.choice(weights_pool, n_functions)]
                member = [rng.random(n_docs) < 0.5 for _ in range(n_functions)]
                if n_functions >= 2:
                    member[1] = None   # a function without a filter: every doc
                if best:
                    operator, msm = [("must", 0), ("should", 0), ("should", tuple(int(rng.integers(0, s + 2)) for s in sizes))][int(rng.integers(0, 3))]
                else:
                    variants = [("must", 0)] + [("should", m) for m in range(0, n_groups + 2)]
                    operator, msm = variants[int(rng.integers(0, len(variants)))]
                tb = ties[int(rng.integers(0, 4))]
                g = _groups(shape, group_of, mins=list(msm) if isinstance(msm, tuple) else ([msm] * n_groups if best else None),
                            tie_breaker=tb, group_occur=int(operator == "must" and not best))
                occur = [int(operator == "must" and best)] * n_clauses
                inner, inner_hit = mm_ref.combine(shape, group_of, scores, matched, operator, msm, tb)
                for sm, bm in MODE_PAIRS:
                    free, _ = ref.value(shape, group_of, scores, matched, operator, msm, tb, member, weights, sm, bm)
                    pivot = float(free[int(np.argsort(free)[n_docs // 2])])   # a final score some doc has: the boundary of the test
                    for ms, mex in ((0.0, 0), (pivot, 0), (pivot, 1), (0.0, 1)):
                        exp_score, exp_hit = ref.value(shape, group_of, scores, matched, operator, msm, tb, member, weights, sm, bm, ms, bool(mex))
                        fs = _fs(weights, sm, bm, ms, mex)
                        for d in range(n_docs):
                            cbits = sum(1 << c for c in range(n_clauses) if matched[c, d])
                            fbits = sum(1 << i for i in range(n_functions) if member[i] is None or member[i][d])
                            rc, got, hit = _value(lib, g, scores[:, d], cbits, fs, fbits, occur, 0 if best else msm)
                            assert rc == 0 and hit == int(exp_hit[d]), (shape, group_of, operator, msm, tb, weights, sm, bm, ms, mex, d)
                            if hit:
                                assert got.view(np.uint32) == exp_score[d].view(np.uint32), (shape, group_of, operator, msm, tb, weights, sm, bm, ms, mex, d)
                                checked += 1
                                boundary += int(ms > 0 and got == f32(ms))
                            if not inner_hit[d]:
                                assert hit == 0
                                # ... also with every function matching and no min_score
                                assert _value(lib, g, scores[:, d], cbits, _fs(weights, sm, bm), 0xFF, occur, 0 if best else msm)[2] == 0
                                rejected += 1
    assert checked > 20_000 and rejected > 1_000 and boundary > 100


def test_no_functions_is_the_multi_match_reference(oracle):
    fields = mm_ref.build_index()
    for shape, groups in (("cross_fields", mm_ref.cross_fields_groups(TOKENS, (0, 1, 2))), ("best_fields", mm_ref.best_fields_groups(TOKENS, (0, 1, 2)))):
        for slicing in (oracle.DEFAULT_SLICING, (2_000, 2)):
            for k, thr, op, msm in ((10, 1000, "should", 0), (300, 100, "must", 0), (1024, 2**31 - 1, "should", 2)):
                kw = dict(operator=op, msm=msm, tie_breaker=0.3, total_hits_threshold=thr, slicing=slicing)
                _same(ref.search(oracle, fields, groups, shape, k, **kw), mm_ref.search(oracle, fields, groups, shape, k, **kw), (shape, k, op))


def test_one_should_group_is_the_function_score_reference(oracle):
    fields = mm_ref.build_index()
    masks = ref.function_masks(fields)
    one_group = [[(0, t, 1.0) for t in TOKENS]]
    for sm, bm in MODE_PAIRS:
        for k, thr, ms, mex in ((10, 1000, 0.0, False), (300, 2**31 - 1, 1.0, False), (100, 100, 1.0, True)):
            got = ref.search(oracle, fields, one_group, "best_fields", k, tie_breaker=0.3, functions=FUNCTIONS, score_mode=sm, boost_mode=bm, min_score=ms,
                             min_excluded=mex, masks=masks, total_hits_threshold=thr)
            exp = fs_ref.search(oracle, fields[0], TOKENS, k, FUNCTIONS, sm, bm, ms, mex, masks=masks, total_hits_threshold=thr)
            _same(got, exp, (sm, bm, k))


def test_the_composition_is_observable_on_the_test_index(oracle):
    """A condition on the GPU tests' inputs: the functions reorder the page (a kernel that ignored them could not pass) and, without
    a min_score, leave the set of hits alone."""
    fields = mm_ref.build_index()
    masks = ref.function_masks(fields)
    for shape, groups in (("cross_fields", mm_ref.cross_fields_groups(TOKENS, (0, 1, 2))), ("best_fields", mm_ref.best_fields_groups(TOKENS, (0, 1, 2)))):
        plain = mm_ref.search(oracle, fields, groups, shape, 100, tie_breaker=0.3)
        boosted = ref.search(oracle, fields, groups, shape, 100, tie_breaker=0.3, functions=FUNCTIONS, masks=masks)
        shared = len(set(plain[0].tolist()) & set(boosted[0].tolist()))
        print(f"{shape}: {shared} shared docs of 100, total_hits {plain[2]} / {boosted[2]}")
        assert shared < 50, (shape, shared)
        assert plain[2] == boosted[2]


def test_refusals_that_need_no_device(lib):
    one = [f32(1.0)] * 4
    ok_g, ok_fs = _groups(0, [0, 0, 1, 1]), _fs([1.5, 2.0])
    assert _value(lib, ok_g, one, 15, ok_fs, 3)[0] == 0
    # the groups' refusals come through with their status ...
    for g, kw, code in [(_groups(2, [0, 0, 1, 1]), {}, INV), (_groups(0, [0, 0, 1, 1], n_groups=9), {}, INV), (_groups(0, [0, 0, 2, 2], n_groups=3), {}, INV),
                        (_groups(0, [0, 0, 1, 1], tie_breaker=1.5), {}, INV), (_groups(0, [0, 0, 1, 1]), {"occur": [0, 1, 0, 0]}, INV),
                        (_groups(1, [0, 0, 1, 1]), {"msm": 1}, INV), (_groups(1, [0, 0, 1, 1]), {"occur": [1, 0, 1, 1]}, UNS),
                        (_groups(1, [0] * 33), {"n_terms": 33, "scores": [f32(1.0)] * 33}, UNS)]:
        rc, _, _ = _value(lib, g, kw.get("scores", one), 15, ok_fs, 3, kw.get("occur"), kw.get("msm", 0), kw.get("n_terms"))
        assert rc == code and lib.nrtgpu_last_error().decode() != "", (g.shape, g.n_groups, kw, rc)
    # ... and so do the functions'
    bad_fs = [(_fs([1.0] * 8, n=9), INV), (_fs([1.0], n=-1), INV), (_fs([1.0], null=True), INV), (_fs([1.0], 2, 0), INV), (_fs([1.0], 0, 3), INV),
              (_fs([1.0], min_score=-1.0), INV), (_fs([1.0], min_score=float("nan")), INV), (_fs([1.0], min_excluded=2), INV),
              (_fs([0.0]), INV), (_fs([float("nan")]), INV), (_fs([float("inf")]), INV), (_fs([1.0, -2.0]), UNS)]
    for fs, code in bad_fs:
        rc, _, _ = _value(lib, ok_g, one, 15, fs, 1)
        assert rc == code and lib.nrtgpu_last_error().decode() != "", (fs.n_functions, fs.score_mode, fs.boost_mode, fs.min_score, rc)
    # both wrong: the groups are checked first
    assert _value(lib, _groups(1, [0, 0, 1, 1]), one, 15, _fs([0.0]), 1, occur=[1, 0, 1, 1])[0] == UNS
    assert _value(lib, _groups(0, [0, 0, 1, 1], tie_breaker=1.5), one, 15, _fs([1.0, -2.0]), 1)[0] == INV
    sc = np.ones(4, f32)
    out = (C.byref(C.c_float()), C.byref(C.c_int32()))
    assert lib.nrtgpu_function_score_multi_match_value(None, 4, None, 0, sc.ctypes.data, 15, C.byref(ok_fs), 0, *out) == INV
    assert lib.nrtgpu_function_score_multi_match_value(C.byref(ok_g), 4, None, 0, None, 15, C.byref(ok_fs), 0, *out) == INV
    assert lib.nrtgpu_function_score_multi_match_value(C.byref(ok_g), 4, None, 0, sc.ctypes.data, 15, None, 0, *out) == INV
    assert lib.nrtgpu_function_score_multi_match_value(C.byref(ok_g), 4, None, 0, sc.ctypes.data, 15, C.byref(ok_fs), 0, None, out[1]) == INV
    assert lib.nrtgpu_function_score_multi_match_value(C.byref(ok_g), 4, None, 0, sc.ctypes.data, 15, C.byref(ok_fs), 0, out[0], None) == INV
    # the entries that need a context refuse a NULL one before anything else
    assert lib.nrtgpu_search_function_score_multi_match_batch(None, None, None, 0, None, None, None, 1, None) == INV
    assert lib.nrtgpu_function_score_multi_match_supported(None, None, 0, None, None, None) == INV
    # the widest accepted shape: 8 groups over 32 clauses, 8 functions
    assert _value(lib, _groups(0, list(range(8)) * 4, tie_breaker=1.0, group_occur=1), [f32(1.0)] * 32, 2**32 - 1, _fs([1.5] * 8, "sum", "sum"), 0xFF)[0] == 0


@pytest.fixture(scope="module")
def mockhip(tmp_path_factory):
    if not (shutil.which("gcc") and os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h")):
        pytest.skip("gcc or the HIP headers are not here")
    build.build()
    out = str(tmp_path_factory.mktemp("mockhip") / "libmockhip.so")
    subprocess.run(["gcc", "-O1", "-w", "-fPIC", "-shared", "-I/opt/rocm/include", os.path.join(ROOT, "tests", "mockhip", "mockhip.c"), "-o", out],
                   check=True)
    return out


def test_host_side_against_the_stand_in_runtime(mockhip):
    e = dict(os.environ, LD_PRELOAD=mockhip)
    e.pop("NRTGPU_LIB_PATH", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mockhip", "function_score_multi_match_host.py")], env=e, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "done" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    got = dict(line.split(" ", 1) for line in r.stdout.strip().split("\n") if " " in line)
    I, U = str(INV), str(UNS)
    expect = {
        "cross_supported": "0", "best_supported": "0", "best_must_supported": "0", "no_functions_supported": "0", "eight_functions_supported": "0",
        "flat_must_supported": "0", "flat_msm_supported": "0", "flat_dismax_supported": "0",
        "flat_must_old_entry": U, "flat_msm_old_entry": U, "flat_dismax_old_entry": U,
        "search_cross": "0", "search_batch_of_4": "0", "search_batch_above_max_batch": I,
        "diagnostics_items": "0 1", "stats_counted": "1",
        "disjunction_max_set": I, "query_tie_breaker_set": I, "k_zero": I, "null_groups": I, "null_functions": I,
        "min_competitive_score": U, "mixed_group": U, "33_clauses": U,
        "nine_functions": I, "weight_zero": I, "score_mode_2": I, "min_score_negative": I, "weight_negative": U,
        "mixed_group_and_weight_zero": U, "weight_zero_and_function_mask_not_resident": I,
        "function_mask_not_resident": U, "function_mask_on_one_leaf": U, "filter_mask_not_resident": U, "five_fields": U,
        "weights_span_too_many_binades": U,
        "flag_no_fixed_point": U, "flag_no_fixed_point_search": U, "flag_packed_postings": U, "flag_packed_postings_search": U,
        "flag_before_function_mask": "flags",
    }
    assert got == expect, {k: (got.get(k), v) for k, v in expect.items() if got.get(k) != v}
