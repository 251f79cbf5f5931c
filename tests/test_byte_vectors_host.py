"""Byte (int8) vector fields without a GPU: the score function the kernel compiles (nrtgpu_byte_vector_score == plan.h:
knn_byte_score) against a numpy restatement of include/nrtgpu.h's table, against the fp32 oracle where both are exact, and
against the reference's own worked numbers (tests/golden/byte_vector_scores.json); then the host paths -- upload, fork,
search, every refusal -- against the stand-in HIP runtime of tests/mockhip.

All comparisons of the C function are BIT equality: its inputs are exact integers and every step is one IEEE operation."""
import ctypes as C
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from nrtsearch_amd import _lib, api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "nrtsearch_amd", "libnrtgpu.so")
SIMS = {"cosine": 0, "dot_product": 1, "l2_norm": 2, "max_inner_product": 3}
f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def c_score(lib, sim, dim, dot, nq, nv):
    out = C.c_float()
    rc = lib.nrtgpu_byte_vector_score(int(sim), int(dim), int(dot), int(nq), int(nv), C.byref(out))
    assert rc == 0, (sim, dim, dot, nq, nv, lib.nrtgpu_last_error())
    return f32(out.value)


def to_score(sim, x, dim):
    """ByteVectorFieldDef.similarityToScore's four shapes over a float32 argument x (l2_norm: x is the SQUARED distance), float32
    scalars, one rounding per operation."""
    x = f32(x)
    if sim == 0:
        return f32(f32(f32(1.0) + x) / f32(2.0))
    if sim == 1:
        return f32(f32(0.5) + f32(x / f32(dim * 32768)))
    if sim == 2:
        return f32(f32(1.0) / f32(f32(1.0) + x))
    return f32(f32(1.0) / f32(f32(1.0) + f32(f32(-1.0) * x))) if x < 0 else f32(x + f32(1.0))


def restated(sim, dim, dot, nq, nv):
    """include/nrtgpu.h's table: from the three integers to the unboosted score."""
    dot, nq, nv = int(dot), int(nq), int(nv)
    if sim == 0:
        if nq == 0 or nv == 0:
            return f32(0.0)
        return to_score(0, f32(f64(dot) / np.sqrt(f64(nq) * f64(nv))), dim)
    if sim == 2:
        return to_score(2, f32(nq + nv - 2 * dot), dim)      # int -> float32: round to nearest even
    return to_score(sim, f32(dot), dim)


def bits(x):
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


def integer_cases(dim):
    """(dot, nq, nv) of 2 000 seeded random int8 pairs plus the corners."""
    rng = np.random.default_rng(1000 + dim)
    q = rng.integers(-128, 128, size=(2000, dim), dtype=np.int8).astype(np.int64)
    v = rng.integers(-128, 128, size=(2000, dim), dtype=np.int8).astype(np.int64)
    cases = list(zip((q * v).sum(1).tolist(), (q * q).sum(1).tolist(), (v * v).sum(1).tolist()))
    lo, hi = np.full(dim, -128, dtype=np.int64), np.full(dim, 127, dtype=np.int64)
    for a, b in ((lo, lo), (hi, lo), (hi, hi)):                      # the largest integers of either sign
        cases.append((int((a * b).sum()), int((a * a).sum()), int((b * b).sum())))
    cases.append((0, int((hi * hi).sum()), int((lo * lo).sum())))   # dot = 0
    cases.append((int((hi * hi).sum()), int((hi * hi).sum()), int((hi * hi).sum())))   # d2 = 0 (a row equal to the query)
    cases.append((0, 0, 0))
    if dim * 16384 * 2 > (1 << 24) + 3:     # d2 just above 2^24, where (float)d2 rounds (odd values: ties and non-ties)
        for d2 in ((1 << 24) + 1, (1 << 24) + 2, (1 << 24) + 3, (1 << 25) + 2, (1 << 25) + 6):
            if d2 <= dim * 16384 * 2:
                nq = d2 // 2
                cases.append((0, nq, d2 - nq))
    return cases


@pytest.mark.parametrize("dim", [3, 128, 768, 2048])
@pytest.mark.parametrize("sim", [0, 1, 2, 3])
def test_score_function_is_the_table_bit_for_bit(lib, sim, dim):
    cases = integer_cases(dim)
    assert len(cases) >= 2006
    bad = []
    for dot, nq, nv in cases:
        got, exp = c_score(lib, sim, dim, dot, nq, nv), restated(sim, dim, dot, nq, nv)
        if bits(got) != bits(exp):
            bad.append((dot, nq, nv, float(got), float(exp)))
    assert not bad, f"sim {sim} dim {dim}: {len(bad)} of {len(cases)} differ, first {bad[:3]}"


@pytest.mark.parametrize("dim", [3, 64, 256])
@pytest.mark.parametrize("sim", [0, 2, 3])
def test_score_function_is_the_fp32_oracle_where_both_are_exact(lib, oracle, sim, dim):
    """int8 vectors at these dimensions: every partial sum of the fp32 oracle is an integer below 2^24, hence exact, so the new
    function must return the oracle's bits for cosine, l2_norm and max_inner_product."""
    rng = np.random.default_rng(77 + 10 * dim + sim)
    n_checked = 0
    for _ in range(500):
        q = rng.integers(-128, 128, size=dim, dtype=np.int8)
        v = rng.integers(-128, 128, size=dim, dtype=np.int8)
        if sim == 0 and (not q.any() or not v.any()):
            continue     # cosine of a zero vector: refused by the reference, not a pair the oracle defines
        qi, vi = q.astype(np.int64), v.astype(np.int64)
        got = c_score(lib, sim, dim, int((qi * vi).sum()), int((qi * qi).sum()), int((vi * vi).sum()))
        exp = oracle.vector_score(sim, q.astype(np.float32), v.astype(np.float32))
        assert bits(got) == bits(exp), (sim, dim, q.tolist(), v.tolist(), float(got), float(exp))
        n_checked += 1
    assert n_checked >= 490


def test_the_references_worked_numbers(lib):
    """tests/golden/byte_vector_scores.json: the constants of the reference's own similarityToScore tests.  dot_product to the
    bit (the reference's expression, evaluated in float32); the others go through similarityToScore's float argument, so they
    check the SHAPE of the formula -- on the restatement the C function is held to bit for bit above, and on the C function itself
    where integers reach the constant."""
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "byte_vector_scores.json")))
    assert len(gold["cases"]) == 7
    for c in gold["cases"]:
        sim, dim, tol = SIMS[c["sim"]], c["dim"], c["tolerance"]
        if c["sim"] == "dot_product":
            exp = f32(f32(0.5) + f32(f32(c["numerator"]) / f32(c["denominator"])))
            i = c["integers"]
            assert bits(c_score(lib, sim, dim, i["dot"], i["q_norm2"], i["v_norm2"])) == bits(exp), c["at"]
            assert bits(to_score(sim, c["similarity"], dim)) == bits(exp), c["at"]
            continue
        arg = c["similarity"] ** 2 if c["sim"] == "l2_norm" else c["similarity"]    # the reference squares the distance itself
        assert abs(float(to_score(sim, arg, dim)) - c["expected"]) <= tol, c["at"]
        if "integers" in c:
            i = c["integers"]
            assert abs(float(c_score(lib, sim, dim, i["dot"], i["q_norm2"], i["v_norm2"])) - c["expected"]) <= tol, c["at"]


def test_score_function_refuses_what_int8_pairs_cannot_produce(lib):
    out = C.c_float()
    for args in ((4, 3, 0, 1, 1), (-1, 3, 0, 1, 1), (0, 0, 0, 1, 1), (0, 2049, 0, 1, 1), (1, 3, 3 * 16384 + 1, 1, 1), (2, 3, 0, -1, 1),
                 (2, 3, 0, 1, 3 * 16384 + 1)):
        assert lib.nrtgpu_byte_vector_score(*args, C.byref(out)) == _lib.NRTGPU_ERR_INVALID_ARG, args
    assert lib.nrtgpu_byte_vector_score(0, 3, 0, 1, 1, None) == _lib.NRTGPU_ERR_INVALID_ARG
    assert bits(c_score(lib, 0, 3, 0, 5, 0)) == 0          # a zero row under cosine scores 0: never NaN


def test_the_python_mirror_takes_int8_only():
    with pytest.raises(TypeError):
        api._int8_rows(np.array([[-129.0, 1.0, 2.0]], dtype=np.float32), "queries")
    with pytest.raises(TypeError):
        api._int8_rows(np.array([[1, 2, 3]], dtype=np.int32), "vectors")
    assert api._int8_rows(np.array([-50, 5, 100], dtype=np.int8), "queries").shape == (1, 3)
    assert "normalized_cosine" not in api.GpuIndexSearcher.BYTE_SIMILARITY


@pytest.fixture(scope="module")
def mockhip(tmp_path_factory):
    if not (shutil.which("gcc") and os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h")):
        pytest.skip("gcc or the HIP headers are not here")
    build.build()
    out = str(tmp_path_factory.mktemp("mockhip") / "libmockhip.so")
    subprocess.run(["gcc", "-O1", "-w", "-fPIC", "-shared", "-I/opt/rocm/include", os.path.join(ROOT, "tests", "mockhip", "mockhip.c"), "-o", out],
                   check=True)
    return out


def test_host_paths_of_byte_fields_against_the_stand_in_runtime(mockhip):
    """tests/mockhip/byte_vectors_host.py: upload into two segments, seal, liveDocs, fork, searches with 1 and 130 queries (kernels
    do nothing there: no hits, but no crash and no hang), every refusal with its status code, the device bytes."""
    e = dict(os.environ, LD_PRELOAD=mockhip)
    e.pop("NRTGPU_LIB_PATH", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mockhip", "byte_vectors_host.py")], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "done" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    got = dict(line.split(" ", 1) for line in r.stdout.strip().split("\n") if " " in line)
    I, U, T = str(_lib.NRTGPU_ERR_INVALID_ARG), str(_lib.NRTGPU_ERR_UNSUPPORTED), str(_lib.NRTGPU_ERR_TIMEOUT)
    expect = {"search_1": "0", "search_130": "0", "search_knn_130": "0", "search_fork": "0", "relation": "1",
              "float_rows_into_byte_field": I, "byte_rows_into_float_field": I, "float_search_over_byte_field": I,
              "float_knn_search_over_byte_field": I, "rescore_over_byte_field": I, "hybrid_over_byte_field": I, "byte_search_over_float_field": I, "wrong_dim": I, "upload_dim_2049": U,
              "search_dim_2049": U, "k_1025": U, "sim_4": I, "negative_boost": I, "zero_query_cosine": I, "zero_query_dot_product": "0", "expired_deadline": T,
              "bytes_grew_by_at_least_rows": "True", "fork_holds_no_second_copy": "True", "float_array_is_a_type_error": "True",
              "normalized_cosine_refused": "True"}
    assert {k: got.get(k) for k in expect} == expect
    assert "byte" in got["float_search_message"] and "float" in got["byte_search_message"] and "byte" in got["hybrid_message"]
