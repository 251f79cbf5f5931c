"""The rescorers over a float vector field without a GPU: the host paths of nrtgpu_rescore_vectors and nrtgpu_search_hybrid_batch --
calls with 1 and 130 queries, 0 hits, the window on both sides of the hit count, the refusals with status code and message, the
deadline -- run against the stand-in HIP runtime of tests/mockhip (tests/mockhip/float_rescore_host.py), as
tests/test_byte_rescore_host.py does for their byte twins.  Both element types go through one host path (vectors.cpp:
rescore_hits_impl, stage_rescore_inputs); the values expected here were recorded from the library as it was BEFORE the float
entries moved onto it, except the NULL-segment case, which that library answered by dereferencing the pointer.  What the kernels
compute is tests/test_float_rescore_gpu.py's business."""
import os
import shutil
import subprocess
import sys

import pytest

from nrtsearch_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mockhip(tmp_path_factory):
    if not (shutil.which("gcc") and os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h")):
        pytest.skip("gcc or the HIP headers are not here")
    build.build()
    out = str(tmp_path_factory.mktemp("mockhip") / "libmockhip.so")
    subprocess.run(["gcc", "-O1", "-w", "-fPIC", "-shared", "-I/opt/rocm/include", os.path.join(ROOT, "tests", "mockhip", "mockhip.c"), "-o", out],
                   check=True)
    return out


def test_host_paths_of_the_float_rescorers_against_the_stand_in_runtime(mockhip, tmp_path):
    e = dict(os.environ, LD_PRELOAD=mockhip, MOCKHIP_TRACE=str(tmp_path / "launches.txt"))
    e.pop("NRTGPU_LIB_PATH", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mockhip", "float_rescore_host.py"), "--null-segment"], env=e, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "done" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    got = dict(line.split(" ", 1) for line in r.stdout.strip().split("\n") if " " in line)
    I, U, T = str(_lib.NRTGPU_ERR_INVALID_ARG), str(_lib.NRTGPU_ERR_UNSUPPORTED), str(_lib.NRTGPU_ERR_TIMEOUT)
    expect = {
        # calls that go through (the kernels do nothing there: a hit in a leaf with rows scores 0, the hit in the leaf without
        # rows keeps query_weight x its first score and leads; the others follow in docid order)
        "hybrid_1": "0", "hybrid_130": "0", "hybrid_window_above_max_k": "0", "rescore_5_hits": "0",
        # hits in leaf 0 (dense rows: 1, 7), leaf 1 (sparse ord -> doc map: 3009 has a row, 3008 has none) and leaf 2 (no vectors: 5000):
        # one gather launch for each of the two leaves with rows, none for the third
        "rescore_hit_docs": "[1, 3009, 5000, 7, 3008]",
        "rescore_launches": str(["_ZN6nrtgpu22rescore_vectors_kernelEPKfS1_iS1_fifPKlS1_iddPf 1 256 0"] * 2),
        "rescore_window_below_the_hits": "[5000, 1, 7]", "rescore_window_above_the_hits": "[5000, 1, 7, 3008, 3009]",
        "rescore_no_vectors_leaf_score": "[0.75, 0.0, 0.0, 0.0, 0.0]", "rescore_no_hits": "0", "rescore_no_hits_window": "0",
        "hybrid_after_the_deadline_was_cleared": "0",
        # the float rescore entry checks neither the boost nor the weights (its byte twin refuses these)
        "rescore_negative_weight": "0", "rescore_negative_boost": "0", "rescore_nan_boost": "0", "rescore_infinite_weight": "0",
        # refusals
        "hybrid_sim_4": I, "hybrid_sim_4_message": "bad rescore arguments",
        "rescore_sim_4": I, "rescore_sim_4_message": "bad rescore arguments",
        "hybrid_wrong_dim": I, "hybrid_wrong_dim_message": f"nrtgpu error {I}: vector dimension mismatch",
        "rescore_wrong_dim": I, "rescore_wrong_dim_message": f"nrtgpu error {I}: segment 0: field 4 has dimension 100, query has 99",
        "hybrid_byte_field": I,
        "hybrid_byte_field_message": f"nrtgpu error {I}: segment 0: field 3 holds byte (int8) vectors: the hybrid tail rescores float vector fields only",
        "rescore_byte_field": I,
        "rescore_byte_field_message": f"nrtgpu error {I}: segment 0: field 3 holds byte (int8) vectors: search it with nrtgpu_knn_exact_bytes / nrtgpu_knn_search_bytes",
        "hybrid_negative_query_weight": U,
        "hybrid_negative_weight_message": f"nrtgpu error {U}: hybrid tail: negative weights (combined scores must stay >= 0)",
        "hybrid_window_0": I,
        "rescore_hit_outside_every_segment": I, "rescore_outside_message": f"nrtgpu error {I}: hit 1 (doc 6000) is outside every segment",
        "hybrid_expired_deadline": T, "hybrid_expired_deadline_message": f"nrtgpu error {T}: deadline passed before the search was planned",
        # a NULL pointer in the middle of `segs`: refused as the byte entry refuses it, and the next call is served
        "rescore_null_segment": I, "rescore_null_segment_message": "segment 1 is NULL", "rescore_after_the_null_segment": "0",
    }
    assert {k: got.get(k) for k in expect} == expect
