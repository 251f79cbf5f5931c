"""The knn request entries over a byte field without a device: the header / ctypes pairing of nrtgpu_knn_search_bytes_requests,
nrtgpu_knn_search_bytes_coalesced and nrtgpu_knn_exact_bytes_coalesced, and -- on the stand-in HIP runtime of tests/mockhip, through
tests/mockhip/knn_byte_requests_host.py -- what they launch and which panels their coalesced callers form:

  * requests that are all equal launch exactly what nrtgpu_knn_search_bytes launches (knn_bytes_kernel, the same grids and LDS bytes);
  * requests that differ launch knn_bytes_requests_kernel, four panels of 16 (P = 4) above 16 members and one otherwise, with the
    grids and the dynamic LDS of the plain kernel's pass (the queue is 4096 entries in both at this dimension);
  * the old entry launches the same before and after (tests/test_vector_launch_schedule_host.py pins its trace line for line);
  * cohorts of coalesced byte callers form as the float ones do (tests/golden/coalescer_batches.txt): two similarities / two boosts
    are two panels, 80 callers are 64 then 16, a deadline that passes in the queue is one TIMEOUT, a bad request fails alone before
    it is queued, and float and byte callers parked together never share a panel."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "nrtsearch_amd", "libnrtgpu.so")
CTYPE_OF = {"nrtgpu_ctx*": C.c_void_p, "const nrtgpu_seg* const*": C.c_void_p, "const int32_t*": C.c_void_p, "const float*": C.c_void_p,
            "const int8_t*": C.c_void_p, "int32_t": C.c_int32, "float": C.c_float}
ENTRIES = {"nrtgpu_knn_search_bytes_requests": 14, "nrtgpu_knn_search_bytes_coalesced": 13, "nrtgpu_knn_exact_bytes_coalesced": 11}


def test_the_three_entries_are_bound_as_the_header_declares_them():
    from nrtsearch_amd import _lib, build
    build.build()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nrtgpu.h")).read(), flags=re.S)
    lib = _lib.load()
    for name, n_args in ENTRIES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/nrtgpu.h"
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        want = []
        for p in params:
            ctype = p.rsplit(" ", 1)[0]   # the declaration without the parameter's name
            want.append(C.POINTER(_lib.TopDocs) if ctype == "nrtgpu_topdocs*" else CTYPE_OF[ctype])
        assert sum(p.startswith("const int8_t*") for p in params) == 1, name   # the queries are int8
        fn = getattr(lib, name)
        assert list(fn.argtypes) == want and len(want) == n_args, name
        assert fn.restype in (C.c_int, C.c_int32)
    from nrtsearch_amd import api
    for method in ("knn_search_bytes_requests", "knn_search_bytes_coalesced", "knn_exact_bytes_coalesced"):
        assert callable(getattr(api.GpuIndexSearcher, method))


@pytest.fixture(scope="module")
def script(tmp_path_factory):
    """What tests/mockhip/knn_byte_requests_host.py prints: {step: (knn_panels delta, [lines])}."""
    assert shutil.which("gcc") and os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"), "gcc and the HIP headers build the stand-in runtime"
    from nrtsearch_amd import build
    dev_lib = build.build_dev()
    tmp = tmp_path_factory.mktemp("mockhip")
    mock = str(tmp / "libmockhip.so")
    subprocess.run(["gcc", "-O1", "-w", "-fPIC", "-shared", "-I/opt/rocm/include", os.path.join(ROOT, "tests", "mockhip", "mockhip.c"), "-o", mock],
                   check=True)
    e = dict(os.environ, LD_PRELOAD=mock, NRTGPU_LIB_PATH=dev_lib, MOCKHIP_SYNC_US="300", MOCKHIP_TRACE=str(tmp / "launches.txt"))
    for knob in ("NRTGPU_KCO_COHORT", "MOCKHIP_TRACE_OPS"):
        e.pop(knob, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mockhip", "knn_byte_requests_host.py")], env=e, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and r.stdout.endswith("done\n"), (r.stdout[-2000:], r.stderr[-2000:])
    steps, cur = {}, None
    for line in r.stdout.split("\n"):
        if line.startswith("== "):
            cur = line.split()[1]
            steps[cur] = (int(line.split("knn_panels=+")[1]), [])
        elif cur and line and not line.startswith(("lone", "done")):
            steps[cur][1].append(line)
    steps["lone"] = (0, [l for l in r.stdout.split("\n") if l.startswith("lone")])
    return steps


def _launches(lines):
    """[(kernel, P, D, grid, block, lds)]"""
    out = []
    for l in lines:
        name, grid, block, lds = l.split()
        m = re.match(r"_ZN6nrtgpu\d+(knn_bytes\w*?kernel)ILi(\d)ELi(\d)EEE", name)
        assert m, l
        out.append((m.group(1), int(m.group(2)), int(m.group(3)), int(grid), int(block), int(lds)))
    return out


def test_equal_requests_launch_what_knn_search_bytes_launches(script):
    for n in (5, 70):
        panels, old = script[f"search_bytes_{n}"]
        assert script[f"requests_equal_{n}"] == (panels, old) and old, n
        assert all(k == "knn_bytes_kernel" for k, *_ in _launches(old))
    assert {p for _, p, *_ in _launches(script["search_bytes_5"][1])} == {1} and script["search_bytes_5"][0] == 1
    assert [p for _, p, *_ in _launches(script["search_bytes_70"][1])] == [4, 4, 1, 1] and script["search_bytes_70"][0] == 2
    assert script["search_bytes_5_again"] == script["search_bytes_5"]   # the old entry, after the new kernel has run


def test_mixed_requests_launch_the_requests_kernel(script):
    plain = _launches(script["search_bytes_70"][1])
    panels, lines = script["requests_mixed_70"]
    mixed = _launches(lines)
    assert panels == 2 and all(k == "knn_bytes_requests_kernel" for k, *_ in mixed)
    # a pass of 64 on four panels, a pass of 6 on one; the rounds, grids, ring depth and dynamic LDS of the plain kernel's passes
    assert [m[1:] for m in mixed] == [p[1:] for p in plain]
    assert all(m[4] == 1024 and m[2] == 2 for m in mixed)   # 100 dimensions: two steps, a ring of two
    for name, p in (("requests_mixed_17", 4), ("requests_mixed_16", 1)):   # P = 4 above 16 members, P = 1 otherwise
        panels, lines = script[name]
        got = _launches(lines)
        assert panels == 1 and got and all(k == "knn_bytes_requests_kernel" and pp == p for k, pp, *_ in got), name


def test_cohorts_of_coalesced_byte_callers_form_as_float_ones_do(script):
    assert script["breq_32_cosine_16_l2"] == (2, ["48 x rc 0 ``", "pending 0 0 0 0 0"])
    assert script["breq_80_is_64_then_16"] == (2, ["80 x rc 0 ``", "pending 0 0 0 0 0"])
    assert script["breq_deadline_expires_in_the_queue"] == (1, ["1 x rc -6 `deadline passed while the request waited for a panel`", "11 x rc 0 ``",
                                                                "pending 0 0 0 0 0"])
    assert script["bexact_two_boosts"] == (2, ["48 x rc 0 ``", "pending 0 0 0 0 0"])
    assert script["bexact_80_is_64_then_16"] == (2, ["80 x rc 0 ``", "pending 0 0 0 0 0"])
    # eight callers each of the float request entry, the byte request entry and the byte exact entry: three queues, three panels
    assert script["float_and_byte_callers_never_share"] == (3, ["24 x rc 0 ``", "pending 0 0 0 0 0"])
    assert script["lone"][1] == ["lone 0 0 0 0 0 0 0"]


def test_a_bad_request_fails_alone_before_it_is_queued(script):
    panels, lines = script["breq_bad_requests_fail_alone"]
    assert panels == 0 and lines[-1] == "pending 0 0 0 0 0"
    assert sorted(lines[:-1]) == sorted(["1 x rc -4 `query 0: filter mask 77 is not resident on segment 0`",
                                         "1 x rc -1 `query 0: a zero vector: cosine similarity is not defined for`",
                                         "1 x rc -1 `segment 0: field 2 has dimension 100, query has 24`"])
