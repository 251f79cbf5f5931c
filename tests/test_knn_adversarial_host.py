"""The worst-case kNN data of tests/_knn_adversarial.py IS worst-case, and the library's certification bounds cover it -- on the
CPU.  For every case, against the module's numpy emulation of the fp16 sketch and its restatement of the oracle's fp32 sums:
  (a) the winners' results are pairwise distinct and exceed every decoy's by at least 4 fp32 ulps of the score,
  (b) every decoy's estimate is strictly above every winner's, and there are at least k_int + k decoys,
  (c) |estimate - result| of every row is at most E,
  (d) need / E is at least the ratio recorded next to the case (- 0.02 for another numpy's summation order), and at least 0.8 for
      the dot_product, max_inner_product and l2_norm cases at 64 and 100 dimensions.
(a) and (b) are conditions on the data: a case that fails them is rebuilt, not relaxed.  E comes twice: restated in the helper
module, and from the library's own code through nrtgpu_debug_knn_bounds of the development library (skipped when the library
has not been built); the two agree to an fp32 ulp, and (c), (d), "the certification refuses" and "the second pass's theta keeps
the winners" are held against the library's.  With that, these mutations of the library fail HERE, without a GPU (each was
applied, the development library rebuilt and this file run):
  2^-10 -> 2^-11 in knn_bound16                 (c) fails for every case
  score_boost dropped from knn_bound16          (c) fails at boost 4, (d) at boost 0.25
  knn_estimate_lower returning s                "the second pass's theta keeps the winners" fails for every case
  knn_result_upper returning m                  "the certification refuses" fails for every case"""
import json
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests import _knn_adversarial as ka

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "nrtsearch_amd", "libnrtgpu.so")
DEV_LIB = os.path.join(ROOT, "nrtsearch_amd", "libnrtgpu_dev.so")
BOOSTED = [("dot_64", 4.0), ("dot_64", 0.25), ("cosine_64", 4.0), ("mip_64", 0.25), ("l2_64", 4.0)]
ALL = [(n, 1.0) for n in ka.CASE_NAMES] + BOOSTED


@pytest.fixture(scope="module")
def measured():
    """{(name, boost): measure()} with the restated bound: computed once."""
    return {(n, b): ka.measure(ka.build(n, b)) for n, b in ALL}


@pytest.fixture(scope="module")
def hook():
    if not os.path.exists(LIB):
        pytest.skip("the library has not been built")
    from nrtsearch_amd import _lib, api, build
    build.build_dev()
    prev = _lib._lib
    _lib._lib = _lib.load_dev()
    try:
        yield api.debug_knn_bounds
    finally:
        _lib._lib = prev


def library_bound(hook, sim, rdim, num, boost, m=0.0, s=0.0):
    """The hook takes the rows' largest |element| and derives the scale itself: rows_unit = 2^(e - 14) with absmax < 2^e."""
    rows_absmax = num["rows_unit"] * 2.0 ** 13      # any value in [2^(e-1), 2^e)
    return hook(sim, rdim, num["nq"], num["q_l1"], num["q_absmax"], num["nv_max"], num["nv_min"], rows_absmax, boost, m, s)


def check_conditions(case, r):
    nw, nd = len(case.winners), len(case.decoys)
    ulp = float(np.spacing(np.float32(r["w_res"].min())))
    assert r["winners_distinct"], case.name                                                                     # (a)
    assert float(r["w_res"].min()) - float(r["d_res"].max()) >= 4 * ulp, (case.name, r["gap_ulps"])
    assert float(r["d_est"].min()) > float(r["w_est"].max()), case.name                                         # (b)
    assert nd >= r["k_int"] + case.k and nw == case.k, case.name
    if len(r["other_res"]):      # rows that are neither: below every winner, and never among the nominations
        assert float(r["other_res"].max()) < float(r["d_res"].min()) and float(r["other_est"].max()) < float(r["w_est"].min()), case.name


@pytest.mark.parametrize("name,boost", ALL, ids=[f"{n}-x{b:g}" for n, b in ALL])
def test_the_cases_are_adversarial(measured, oracle, name, boost):
    case, r = ka.build(name, boost), measured[(name, boost)]
    check_conditions(case, r)
    assert r["max_err_ratio"] <= 1.0, (name, r["max_err_ratio"])                                                # (c)
    assert r["ratio"] >= case.ratio - 0.02, (name, r["ratio"], case.ratio)                                      # (d)
    if case.dim in (64, 100) and case.sim_name != "cosine" and case.k == 10:
        assert r["ratio"] >= 0.8, (name, r["ratio"])
    assert not r["certifies"] and r["second_theta_keeps_winners"], name
    # the restated oracle IS the oracle: its scores through the C oracle, bit for bit, and a float64 reference within the fp32
    # sum's own error (gamma |q||v|) -- the winners' lead is real, not an artefact of the order of summation, where it is larger
    sim = r["sim"]
    for rows, res in ((case.winners[:3], r["w_res"][:3]), (case.decoys[:3], r["d_res"][:3])):
        for v, s in zip(rows, res):
            assert np.float32(np.float32(oracle.vector_score(sim, case.query, v)) * np.float32(boost)) == s, name
    if sim in (1, 3):
        q64 = case.query.astype(np.float64)
        w64, d64 = case.winners.astype(np.float64) @ q64, case.decoys.astype(np.float64) @ q64
        assert w64.min() > d64.max(), name


def test_the_recorded_ratios_are_the_measured_ones(measured):
    for n in ka.CASE_NAMES:
        assert abs(measured[(n, 1.0)]["ratio"] - ka.build(n).ratio) <= 0.02, (n, measured[(n, 1.0)]["ratio"])


@pytest.mark.parametrize("name", ["dot_64", "mip_64"])
def test_two_leaves_with_different_sketch_scales_stay_adversarial(name):
    case = ka.build(name)
    extra, scale = ka.two_leaf_extra(case)
    assert scale * 2.0 ** 6 == ka.pow2_scale(np.abs(case.decoys).max())
    r = ka.measure(case, extra_rows=extra, extra_scale=scale)
    check_conditions(case, r)
    assert r["max_err_ratio"] <= 1.0 and not r["certifies"] and r["second_theta_keeps_winners"]


def test_deleted_decoys_leave_the_case_adversarial():
    case = ka.build("dot_64")
    r = ka.measure(case, dead_decoys=ka.DEAD_DECOYS)
    assert len(case.decoys) - len(ka.DEAD_DECOYS) >= r["k_int"] + case.k
    assert float(r["d_est"].min()) > float(r["w_est"].max()) and not r["certifies"] and r["second_theta_keeps_winners"]


@pytest.mark.parametrize("name,boost", ALL, ids=[f"{n}-x{b:g}" for n, b in ALL])
def test_the_librarys_bounds_cover_the_cases_and_no_more(measured, hook, name, boost):
    case, r = ka.build(name, boost), measured[(name, boost)]
    sim, num = r["sim"], r["numbers"]
    lib = library_bound(hook, sim, r["rdim"], num, boost, m=r["m_est"], s=r["kth"])
    e_lib, e_here = lib["e16"], r["E"]
    assert abs(e_lib - e_here) <= float(np.spacing(np.float32(e_here))), (name, e_lib, e_here)
    assert abs(lib["e32"] - ka.bound32(sim, r["rdim"], num["nq"], num["nv_max"], boost)) <= float(np.spacing(np.float32(lib["e32"])))
    assert lib["q_scale"] == 1.0 / num["q_unit"] and lib["rows_scale"] == 1.0 / num["rows_unit"] and lib["q_scale_usable"] and lib["rows_scale_usable"]
    assert r["max_err_ratio"] * e_here <= e_lib, (name, r["max_err_ratio"] * e_here / e_lib)                    # (c)
    ratio = r["need"] / e_lib
    assert ratio >= case.ratio - 0.02, (name, ratio)                                                            # (d)
    if case.dim in (64, 100) and case.sim_name != "cosine" and case.k == 10:
        assert ratio >= 0.8, (name, ratio)
    # the certification refuses (the nominations are all decoys), and the second pass's theta keeps every winner
    assert not r["kth"] > lib["result_upper16"], (name, r["kth"], lib["result_upper16"])
    assert float(r["w_est"].min()) >= lib["estimate_lower16"], (name, float(r["w_est"].min()), lib["estimate_lower16"])
    # plan.h's two functions against their restatements
    assert math.isclose(lib["result_upper16"], ka.result_upper(sim, r["m_est"], e_lib, boost), rel_tol=1e-12)
    assert math.isclose(lib["estimate_lower16"], ka.estimate_lower(sim, r["kth"], e_lib, boost), rel_tol=1e-12)
    assert math.isclose(lib["result_upper32"], ka.result_upper(sim, r["m_est"], lib["e32"], boost), rel_tol=1e-12)
    assert math.isclose(lib["estimate_lower32"], ka.estimate_lower(sim, r["kth"], lib["e32"], boost), rel_tol=1e-12)


def test_no_sketch_from_a_scale_that_is_not_a_finite_normal_float(hook):
    """host_math.h: knn_sketch_scale.  A largest |element| of 2^-113 still scales (2^126, reciprocal 2^-126: the smallest normal
    float); anything below does not -- 2^(14 - e) is 2^127 or inf and its reciprocal subnormal or 0 -- nor does inf or NaN.  Zero
    keeps the scale 1."""
    def scale(absmax):
        d = hook(1, 64, 1.0, 1.0, absmax, 1.0, 1.0, absmax)
        assert (d["q_scale"], d["q_scale_usable"]) == (d["rows_scale"], d["rows_scale_usable"])
        return d["q_scale"], d["q_scale_usable"]
    assert scale(1.0) == (2.0 ** 13, True) and scale(1.999) == (2.0 ** 13, True) and scale(2.0) == (2.0 ** 12, True)
    assert scale(2.0 ** -113) == (2.0 ** 126, True)
    assert scale(float(np.nextafter(np.float32(2.0 ** -113), np.float32(0)))) == (1.0, False)
    assert scale(2.0 ** -120) == (1.0, False) and scale(2.0 ** -149) == (1.0, False)
    assert scale(2.0 ** 100) == (2.0 ** -87, True) and scale(float(np.finfo(np.float32).max)) == (2.0 ** -114, True)
    assert scale(float("inf")) == (1.0, False) and scale(float("nan")) == (1.0, False)
    assert scale(0.0) == (1.0, True)


def test_a_query_too_small_to_scale_sends_its_panel_to_the_fp32_rows(tmp_path):
    """knn_impl's side of the same decision, on the stand-in runtime (tests/mockhip: kernels do nothing, so the rows' largest
    |element| reads 0 and the field keeps a sketch at scale 1): a panel nominates from the sketch unless one of its queries has a
    largest |element| below 2^-113 or an infinite one."""
    if not (shutil.which("gcc") and os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h") and os.path.exists(LIB)):
        pytest.skip("gcc, the HIP headers or the built library are not here")
    mock = str(tmp_path / "libmockhip.so")
    subprocess.run(["gcc", "-O1", "-w", "-fPIC", "-shared", "-I/opt/rocm/include", os.path.join(ROOT, "tests", "mockhip", "mockhip.c"), "-o", mock],
                   check=True)
    e = dict(os.environ, LD_PRELOAD=mock)
    e.pop("NRTGPU_LIB_PATH", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mockhip", "knn_scale_decision.py")], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "done" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
    panels = [json.loads(line[6:]) for line in r.stdout.split("\n") if line.startswith("PANEL ")]
    assert len(panels) == 24
    for p in panels:
        assert p["launches"] > 0, p
        assert (p["sketch"] > 0) == (p["name"] in ("ordinary", "edge", "zero")), p
