"""The rescorers over a byte (int8) vector field without a GPU: nrtgpu_rescore_byte_vectors and nrtgpu_search_hybrid_bytes_batch are
declared, exported and bound; the Python mirror takes int8 only; and the host paths -- calls with 1 and 130 queries, every
refusal of include/nrtgpu.h with its status code and message, the deadline -- run against the stand-in HIP runtime of
tests/mockhip (tests/mockhip/byte_rescore_host.py).  What the kernels compute is tests/test_byte_rescore_gpu.py's business."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from nrtsearch_amd import _lib, api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nrtgpu_rescore_byte_vectors", "nrtgpu_search_hybrid_bytes_batch")


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_both_entries_are_declared_exported_and_bound_like_their_float_twins(lib):
    header = open(os.path.join(ROOT, "include", "nrtgpu.h")).read()
    for name, twin in zip(ENTRIES, ("nrtgpu_rescore_vectors", "nrtgpu_search_hybrid_batch")):
        assert re.search(r"^int\s+%s\(" % name, header, flags=re.M), f"{name} is not declared in include/nrtgpu.h"
        assert name in _lib.ABI_SYMBOLS
        fn = getattr(lib, name)          # AttributeError: not exported
        assert fn.argtypes is not None and list(fn.argtypes) == list(getattr(lib, twin).argtypes)
        proto = re.search(r"^int\s+%s\((.*?)\);" % name, header, flags=re.M | re.S).group(1)
        assert "const int8_t* query" in proto and "float*" not in proto.replace("const float* first_scores", "")
    # the header no longer parks the rescorers as out of scope for byte fields
    out_of_scope = re.search(r"Out of scope for byte fields.*?\*/", header, flags=re.S).group(0).split("-----")[0]
    assert "nrtgpu_rescore_vectors" not in out_of_scope and "hybrid tail" not in out_of_scope
    assert "nrtgpu_knn_exact_coalesced" in out_of_scope and "nrtgpu_dist_*" in out_of_scope and "Java" in out_of_scope


def test_the_python_mirror_of_the_rescorers_takes_int8_only():
    """No device is reached: the array's type and the similarity's name are checked before anything is marshalled."""
    sr = api.GpuIndexSearcher.__new__(api.GpuIndexSearcher)
    hits = api.TopDocs(np.array([1], dtype=np.int32), np.array([1.0], dtype=np.float32), 1, False)
    for bad in (np.ones(8, dtype=np.float32), np.ones(8, dtype=np.int32), np.ones(8, dtype=np.uint8), [1.0, 2.0]):
        with pytest.raises(TypeError):
            sr.rescore_byte_vectors(hits, 3, "cosine", bad, 1)
        with pytest.raises(TypeError):
            sr.search_hybrid_bytes_batch([api.TermQuery(0, 1)], [api.TopScoreDocCollectorManager(10)], 3, "cosine", bad, 1)
    with pytest.raises(ValueError):
        sr.rescore_byte_vectors(hits, 3, "normalized_cosine", np.ones(8, dtype=np.int8), 1)
    with pytest.raises(ValueError):
        sr.search_hybrid_bytes_batch([api.TermQuery(0, 1)], [api.TopScoreDocCollectorManager(10)], 3, "normalized_cosine",
                                     np.ones((1, 8), dtype=np.int8), 1)


@pytest.fixture(scope="module")
def mockhip(tmp_path_factory):
    if not (shutil.which("gcc") and os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h")):
        pytest.skip("gcc or the HIP headers are not here")
    build.build()
    out = str(tmp_path_factory.mktemp("mockhip") / "libmockhip.so")
    subprocess.run(["gcc", "-O1", "-w", "-fPIC", "-shared", "-I/opt/rocm/include", os.path.join(ROOT, "tests", "mockhip", "mockhip.c"), "-o", out],
                   check=True)
    return out


def test_host_paths_of_the_byte_rescorers_against_the_stand_in_runtime(mockhip):
    e = dict(os.environ, LD_PRELOAD=mockhip)
    e.pop("NRTGPU_LIB_PATH", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mockhip", "byte_rescore_host.py")], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "done" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    got = dict(line.split(" ", 1) for line in r.stdout.strip().split("\n") if " " in line)
    I, U, T = str(_lib.NRTGPU_ERR_INVALID_ARG), str(_lib.NRTGPU_ERR_UNSUPPORTED), str(_lib.NRTGPU_ERR_TIMEOUT)
    expect = {
        # calls that must go through (kernels do nothing there: no hits, but no crash and no hang)
        "hybrid_1": "0", "hybrid_130": "0", "hybrid_window_above_max_k": "0", "rescore_4_hits": "0", "rescore_keeps_window": "True",
        "rescore_no_hits": "0", "rescore_negative_weight": "0", "hybrid_zero_query_l2_norm": "0", "rescore_zero_query_dot_product": "0",
        "float_hybrid_over_float_field": "0", "hybrid_after_the_deadline_was_cleared": "0",
        # the issue's table, per entry
        "hybrid_sim_4": I, "rescore_sim_4": I,
        "hybrid_zero_query_cosine": I, "rescore_zero_query_cosine": I,
        "hybrid_wrong_dim": I, "rescore_wrong_dim": I,
        "hybrid_float_field": I, "rescore_float_field": I,
        "hybrid_negative_boost": I, "hybrid_infinite_boost": I, "hybrid_nan_boost": I, "rescore_negative_boost": I, "rescore_nan_boost": I,
        "hybrid_dim_2049": U, "rescore_dim_2049": U,
        "hybrid_negative_query_weight": U, "hybrid_negative_rescore_weight": U,
        "rescore_hit_outside_every_segment": I, "rescore_infinite_weight": I, "hybrid_window_0": I,
        # a float call on the byte field still refuses (tests/test_byte_vectors_host.py pins the same)
        "float_rescore_over_byte_field": I, "float_hybrid_over_byte_field": I,
        "hybrid_expired_deadline": T,
        "hybrid_float_array_is_a_type_error": "True", "rescore_float_array_is_a_type_error": "True", "rescore_int32_array_is_a_type_error": "True",
        "hybrid_normalized_cosine_refused": "True", "rescore_normalized_cosine_refused": "True",
    }
    assert {k: got.get(k) for k in expect} == expect
    assert "float" in got["hybrid_float_field_message"] and "float" in got["rescore_float_field_message"]
    assert "negative weights" in got["hybrid_negative_weight_message"]
    assert "outside every segment" in got["rescore_outside_message"]
