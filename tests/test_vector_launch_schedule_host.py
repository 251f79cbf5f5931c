"""The launch schedule of the vector paths' host code, without a GPU: tests/mockhip/vector_launch_trace.py runs the exact searches
(float and byte rows; the sketch and the fp32 rows; the knn request with a filter and a score threshold; a leaf long enough for
the deferred selection), the two-call rescorers and the fused hybrid tails against the stand-in HIP runtime with MOCKHIP_TRACE,
and what it prints -- per step the deltas of the knn counters and every kernel launched with its grid, block and dynamic shared
bytes -- must equal tests/golden/vector_host_launch_trace.txt line for line.  The golden file was recorded from the library as it
was BEFORE the float and byte paths shared their host code (KnnRun, stage_rescore_inputs, rescore_hits_impl), so it pins that
the shared code kept every launch, every grid and the order of launches and selections."""
import os
import shutil
import subprocess
import sys

import pytest

from nrtsearch_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "vector_host_launch_trace.txt")


def test_the_vector_paths_launch_what_the_recorded_schedule_says(tmp_path):
    if not (shutil.which("gcc") and os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h")):
        pytest.skip("gcc or the HIP headers are not here")
    build.build()
    mock = str(tmp_path / "libmockhip.so")
    subprocess.run(["gcc", "-O1", "-w", "-fPIC", "-shared", "-I/opt/rocm/include", os.path.join(ROOT, "tests", "mockhip", "mockhip.c"), "-o", mock],
                   check=True)
    e = dict(os.environ, LD_PRELOAD=mock, MOCKHIP_TRACE=str(tmp_path / "launches.txt"))
    e.pop("NRTGPU_LIB_PATH", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mockhip", "vector_launch_trace.py")], env=e, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and r.stdout.endswith("done\n"), (r.stdout[-2000:], r.stderr[-2000:])
    got, want = r.stdout.split("\n"), open(GOLDEN).read().split("\n")
    steps = [l.split()[1] for l in got if l.startswith("== ")]
    assert steps == [l.split()[1] for l in want if l.startswith("== ")]
    assert sum("knn_sketch_kernel" in l for l in got) > 0 and sum("knn_bytes_kernel" in l for l in got) > 0   # (the trace names kernels)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"line {i + 1}: launched `{g}`, the recorded schedule has `{w}`"
    assert len(got) == len(want)
