"""Which requests the two single-query entries send to the device together, and what each caller is told, without a GPU:
tests/mockhip/coalescer_batches.py parks the callers of every scenario behind nrtgpu_debug_hold_coalescers (the development library),
so each batch / panel is formed by construction, and prints per scenario the deltas of the context's counters and the sorted
multiset of (rc, error text) over the callers.  nrtgpu_search_bm25_coalesced: one batch of 32; 8 and 8 under two thread-slice
lists; 80 as 64 then 16; a request the planner refuses failing alone after the member-by-member re-run; a deadline that passes in
the queue; a failed launch re-run member by member.  nrtgpu_knn_exact_coalesced: two similarities as two panels; 80 as 64 then 16;
the deadline; a failed launch told to every member of the panel; a wrong dimension refused before it is queued.  After every
scenario nothing is pending, and a lone call of each entry still succeeds.

What it prints must equal tests/golden/coalescer_batches.txt line for line.  The golden file was recorded from the library as it
was BEFORE the two entries shared one coalescer (csrc/coalescer.h), so it pins that the shared mechanism kept every cohort, every
error code and text, and every counter."""
import os
import shutil
import subprocess
import sys

from nrtsearch_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "coalescer_batches.txt")


def test_the_coalescers_form_the_recorded_batches_and_tell_every_caller_the_recorded_answer(tmp_path):
    assert shutil.which("gcc") and os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"), "gcc and the HIP headers build the stand-in runtime"
    dev_lib = build.build_dev()
    mock = str(tmp_path / "libmockhip.so")
    subprocess.run(["gcc", "-O1", "-w", "-fPIC", "-shared", "-I/opt/rocm/include", os.path.join(ROOT, "tests", "mockhip", "mockhip.c"), "-o", mock],
                   check=True)
    e = dict(os.environ, LD_PRELOAD=mock, NRTGPU_LIB_PATH=dev_lib, MOCKHIP_SYNC_US="300")
    for knob in ("NRTGPU_CO_COHORT", "NRTGPU_KCO_COHORT", "MOCKHIP_TRACE"):
        e.pop(knob, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mockhip", "coalescer_batches.py")], env=e, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and r.stdout.endswith("done\n"), (r.stdout[-2000:], r.stderr[-2000:])
    got, want = r.stdout.split("\n"), open(GOLDEN).read().split("\n")
    # what the recorded result says, spelled out: the cohorts, who is told what, nothing left behind
    step = {l.split()[1]: dict(f.split("=+") for f in l.split()[2:]) for l in got if l.startswith("== ")}
    assert (step["bm25_32_same_leaves"]["batches"], step["bm25_32_same_leaves"]["queries"]) == ("1", "32")
    assert step["bm25_8_and_8_by_slices"]["batches"] == "2" and step["bm25_80_is_64_then_16"]["batches"] == "2"
    assert step["knn_32_cosine_16_l2"]["knn_panels"] == "2" and step["knn_80_is_64_then_16"]["knn_panels"] == "2"
    assert sum("rc -6 `deadline passed while the request waited for a batch`" in l and l.startswith("1 x ") for l in got) == 1
    assert sum("rc -6 `deadline passed while the request waited for a panel`" in l and l.startswith("1 x ") for l in got) == 1
    assert all(l == "pending 0 0" for l in got if l.startswith("pending")) and got.count("lone 0 0") == 2
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"line {i + 1}: the library did `{g}`, the recorded result has `{w}`"
    assert len(got) == len(want)


def test_the_coalescer_alone_serves_32_closed_loop_callers(tmp_path):
    """tests/standalone/coalescer_stress.cpp includes nothing but csrc/coalescer.h: 32 threads, mixed compatibility keys, some deadlines
    shorter than a batch, a "device" that sleeps 200 us.  The program checks that every call returns once with its own answer and
    that nothing stays pending; here the plain build runs for a second (its header says how to build it under a sanitizer)."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler builds the program"
    exe = str(tmp_path / "coalescer_stress")
    subprocess.run([cxx, "-std=c++17", "-O1", "-pthread", os.path.join(ROOT, "tests", "standalone", "coalescer_stress.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, "1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("coalescer_stress ok"), (r.stdout[-500:], r.stderr[-2000:])
