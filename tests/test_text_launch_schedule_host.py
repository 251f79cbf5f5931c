"""What the text paths' host code puts on a stream, without a GPU: tests/mockhip/text_launch_trace.py runs the batch entry (one
query, a few, enough for the parallel unpack; MaxScore and exhaustive-scan items in one call; speculation on and off;
collect_timing on and off; the blocking wait), its two-pass path (one tagged query: a follow-up launch; forty: a batch of its own),
the hybrid entries over float and byte rows (clean and with a tagged query), the device-resident entries (synchronous, through the
launcher thread -- clean and with a tagged hit total, which nrtgpu_pending_wait answers with a whole-batch re-run -- and one shard of
two with a guess buffer), the merge of gathered lists, a function-score and a multi-match batch, a coalesced call and every
entry's refusals against the stand-in HIP runtime with MOCKHIP_TRACE and MOCKHIP_TRACE_OPS.  What it prints -- per step the deltas
of the context's counters, the diagnostics, and every kernel launch (grid, block, dynamic shared bytes), copy (kind, bytes, offsets
inside their allocations), memset (offset, extent), event record, stream wait and synchronisation, in order -- must equal
tests/golden/text_host_launch_trace.txt line for line.  The golden file was recorded from the library as it was BEFORE search.cpp
and finalscore.cpp shared their plan layout, merge staging, two-pass driver and result unpacking, so it pins that the shared code
kept every blob size, the extent of the zeroing memset, the order of waits, records and copies, the number of copies back, and
which of two faults of one bad call each entry names.  (Since then re-recorded in the function-score and multi-match steps only, twelve
lines: those kernels take one more pointer, the zeroing memset also covers the per-slice counts of hits behind a cursor, and the
relation comes from slice_relation_past_kernel.)

The paths of dist.cpp that call merge_lists_on_device and hybrid_tail_on_device need a communicator (nrtgpu_dist_init), which
cannot be had without the RCCL stand-in and a second process: tests/test_dist_two_ranks_host.py runs them under the same mock."""
import os
import shutil
import subprocess
import sys

import pytest

from nrtsearch_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "text_host_launch_trace.txt")


def body(lines, step):
    at = next(i for i, l in enumerate(lines) if l.startswith(f"== {step} "))
    end = next((i for i in range(at + 1, len(lines)) if lines[i].startswith("== ")), len(lines))
    return lines[at + 1: end]


def launches(lines, step):
    """the kernel launches of one step, in order"""
    return [l.split()[0] for l in body(lines, step) if l.startswith("_Z")]


def counter(lines, step, name):
    line = next(l for l in lines if l.startswith(f"== {step} "))
    return int(next(f for f in line.split() if f.startswith(name + "=+")).split("+")[1])


def test_the_text_paths_enqueue_what_the_recorded_schedule_says(tmp_path):
    if not (shutil.which("gcc") and os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h")):
        pytest.skip("gcc or the HIP headers are not here")
    build.build()
    mock = str(tmp_path / "libmockhip.so")
    subprocess.run(["gcc", "-O1", "-w", "-fPIC", "-shared", "-I/opt/rocm/include", os.path.join(ROOT, "tests", "mockhip", "mockhip.c"), "-o", mock],
                   check=True)
    e = dict(os.environ, LD_PRELOAD=mock, MOCKHIP_TRACE=str(tmp_path / "launches.txt"), MOCKHIP_TRACE_OPS="1")
    e.pop("NRTGPU_LIB_PATH", None)
    e.pop("TEXT_TRACE_PROFILE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mockhip", "text_launch_trace.py")], env=e, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and r.stdout.endswith("done\n"), (r.stdout[-2000:], r.stderr[-2000:])
    got, want = r.stdout.split("\n"), open(GOLDEN).read().split("\n")
    steps = [l.split()[1] for l in got if l.startswith("== ")]
    assert steps == [l.split()[1] for l in want if l.startswith("== ")]
    # the trace names kernels, and one call ran both scorers over items of their own
    for kernel in ("bm25_maxscore_kernel", "bm25_scan_kernel"):
        grids = [int(l.split()[1]) for l in body(got, "search_batch_mixed") if kernel in l]
        assert len(grids) == 1 and grids[0] > 0, kernel
    # a two-pass step shows two rounds of launches and counts its re-runs
    one = launches(got, "search_batch_16")
    for step, reruns in (("search_batch_16_one_tagged", 1), ("search_batch_64_forty_tagged", 40), ("search_hybrid_batch_one_tagged", 1),
                         ("search_hybrid_bytes_batch_one_tagged", 1), ("begin_wait_device_pre_tagged", 1)):
        twice = launches(got, step)
        assert len(twice) % 2 == 0 and twice[: len(twice) // 2] == twice[len(twice) // 2:] and len(twice) >= 2 * len(one), (step, twice)
        assert counter(got, step, "spec_reruns") == reruns, step
    assert launches(got, "search_batch_16_untagged_again") == one
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"line {i + 1}: the library did `{g}`, the recorded schedule has `{w}`"
    assert len(got) == len(want)
