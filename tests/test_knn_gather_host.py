"""The host side of the gather route of the filtered knn requests (nrtgpu_set_knn_gather; vectors_gather.cpp) without a GPU:
tests/mockhip/knn_gather_host.py against the stand-in HIP runtime with MOCKHIP_TRACE -- the setter's argument check, which kernels
a request enqueues at knob 0, 10 and 1000 for filters accepting 0.5 %, 5 % and 100 % of the rows, that a context nobody called the
setter on launches what tests/golden/vector_host_launch_trace.txt recorded for the same requests, and that a float field searched
only on the gather route builds no fp16 sketch."""
import os
import shutil
import subprocess
import sys

import pytest

from nrtsearch_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "vector_host_launch_trace.txt")
FULL_FLOAT = {"knn_panel_fp16_kernel", "knn_sketch_kernel", "knn_select_kernel"}
GATHER_FLOAT = ["knn_accept_rows_kernel", "knn_gather_score_kernel", "knn_select_kernel"]
GATHER_BYTES = ["knn_accept_rows_kernel", "knn_gather_bytes_kernel", "knn_select_kernel"]
GATHER_ONLY = ("knn_accept_rows_kernel", "knn_gather_score_kernel", "knn_gather_bytes_kernel")


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    if not (shutil.which("gcc") and os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h")):
        pytest.skip("gcc or the HIP headers are not here")
    build.build()
    tmp = tmp_path_factory.mktemp("knn_gather_host")
    mock = str(tmp / "libmockhip.so")
    subprocess.run(["gcc", "-O1", "-w", "-fPIC", "-shared", "-I/opt/rocm/include", os.path.join(ROOT, "tests", "mockhip", "mockhip.c"), "-o", mock],
                   check=True)
    e = dict(os.environ, LD_PRELOAD=mock, MOCKHIP_TRACE=str(tmp / "launches.txt"))
    e.pop("NRTGPU_LIB_PATH", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mockhip", "knn_gather_host.py")], env=e, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and r.stdout.endswith("done\n"), (r.stdout[-2000:], r.stderr[-2000:])
    return dict(line.split(" ", 1) for line in r.stdout.strip().split("\n") if " " in line)


def test_the_setter_takes_0_to_1000_permille(host_run):
    I = str(_lib.NRTGPU_ERR_INVALID_ARG)
    assert {k: host_run[k] for k in ("set_minus_1", "set_1001", "set_null_ctx", "set_1000", "set_0")} == \
        {"set_minus_1": I, "set_1001": I, "set_null_ctx": I, "set_1000": "0", "set_0": "0"}


def golden_block(step):
    lines = open(GOLDEN).read().split("\n")
    at = next(i for i, l in enumerate(lines) if l.startswith(f"== {step} "))
    out = []
    for l in lines[at + 1:]:
        if l.startswith("== ") or not l:
            break
        out.append(l)
    return out


def test_a_default_context_launches_the_recorded_schedule(host_run):
    """Nobody called the setter: the filtered requests of tests/mockhip/vector_launch_trace.py enqueue, line for line (kernel, grid,
    block, dynamic shared bytes), what the golden trace holds for them."""
    assert host_run["default_float"].split("|") == golden_block("knn_search_sketch")
    assert host_run["default_bytes"].split("|") == golden_block("knn_search_bytes")
    assert not any(k in host_run["default_float"] + host_run["default_bytes"] for k in GATHER_ONLY)


@pytest.mark.parametrize("kind", ["float", "bytes"])
def test_the_route_per_knob_and_filter(host_run, kind):
    """gather iff the knob is > 0 and the filter's share of the rows is at most the knob (and fits one candidate list: all of these
    do): knob 10 = 1 % takes the 0.5 % filter only, knob 1000 every filter, knob 0 none."""
    gather = GATHER_FLOAT if kind == "float" else GATHER_BYTES
    for knob in (0, 10, 1000):
        for mask, share in (("half_pct", 5), ("5pct", 50), ("all", 1000)):
            names = host_run[f"route_{kind}_{knob}_{mask}"].split(",")
            stats = host_run[f"stats_{kind}_{knob}_{mask}"]
            if knob > 0 and share <= knob:
                assert names == gather, (knob, mask, names)
                # (the stand-in's listing kernel counts no row: +0 rows; one timed scoring launch, no sketch launch, no second pass)
                assert stats == "knn_panels=+1 knn_score_launches=+1 knn_rows=+0 knn_sketch_launches=+0 knn_second_passes=+0", (knob, mask, stats)
            else:
                assert not any(k in names for k in GATHER_ONLY), (knob, mask, names)
                assert (set(names) == FULL_FLOAT) if kind == "float" else (set(names) == {"knn_bytes_kernel", "knn_select_kernel"}), (knob, mask, names)
                assert "knn_rows=+70100" in stats or "knn_rows=+140200" in stats, (knob, mask, stats)    # every row (float: and its second pass)
    # the row list is made once per call, every pass of 64 queries scores and selects
    assert host_run["route_float_1000_all_130_queries"].split(",") == GATHER_FLOAT + GATHER_FLOAT[1:] * 2


def test_the_full_passes_refusals_hold_on_the_gather_route(host_run):
    I, U, T = str(_lib.NRTGPU_ERR_INVALID_ARG), str(_lib.NRTGPU_ERR_UNSUPPORTED), str(_lib.NRTGPU_ERR_TIMEOUT)
    expect = {"expired_deadline_float": T, "expired_deadline_bytes": T, "wrong_dim": I, "float_entry_on_byte_field": I,
              "byte_entry_on_float_field": I, "unknown_mask": U, "k_1025": U}
    assert {k: host_run[k] for k in expect} == expect


def test_a_field_searched_only_on_the_gather_route_builds_no_sketch(host_run):
    assert host_run["gather_only_kernels"].split(",") == GATHER_FLOAT
    assert host_run["gather_only_growth_below_sketch"] == "True"
    assert host_run["full_pass_builds_sketch"] == "True"
