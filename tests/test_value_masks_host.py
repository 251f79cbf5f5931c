"""Filter masks built from doc value columns (nrtgpu_segment_set_mask_from_values, nrtgpu_segment_get_mask), the part that needs
no device: the struct's size and the exported symbols, the refusals decided before any device is touched, what the binding
marshals and refuses, the NumPy reference of the GPU tests (tests/_value_masks_ref.py) against a brute-force Python loop, and --
against tests/mockhip -- the whole refusal table with its precedence and the host bookkeeping."""
import ctypes as C
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

from nrtsearch_amd import _lib, api, build

from tests import _field_sort_ref as fs
from tests import _value_masks_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV, UNS, STATE = _lib.NRTGPU_ERR_INVALID_ARG, _lib.NRTGPU_ERR_UNSUPPORTED, _lib.NRTGPU_ERR_STATE


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_struct_size_and_symbols(lib):
    assert C.sizeof(_lib.ValueClause) == 32
    for name, off in (("kind", 0), ("field_id", 4), ("lower_bits", 8), ("upper_bits", 12), ("n_values", 16), ("reserved", 20), ("value_bits", 24)):
        assert getattr(_lib.ValueClause, name).offset == off, name
    assert (_lib.NRTGPU_CLAUSE_RANGE, _lib.NRTGPU_CLAUSE_EXISTS, _lib.NRTGPU_CLAUSE_IN_SET, _lib.NRTGPU_MAX_SET_VALUES) == (0, 1, 2, 4096)
    for sym in ("nrtgpu_segment_set_mask_from_values", "nrtgpu_segment_get_mask"):
        assert sym in _lib.ABI_SYMBOLS and getattr(lib, sym) is not None
    header = open(os.path.join(ROOT, "include", "nrtgpu.h")).read()
    for text in ("#define NRTGPU_CLAUSE_IN_SET 2", "#define NRTGPU_MAX_SET_VALUES 4096", "} nrtgpu_value_clause;"):
        assert text in header


def test_null_and_out_of_range_arguments_are_refused_without_a_device(lib):
    vc = (_lib.ValueClause * 1)()
    cnt = C.c_int64(0)
    buf = (C.c_uint64 * 4)()
    assert lib.nrtgpu_segment_set_mask_from_values(None, 5, vc, 1, C.byref(cnt)) == INV and b"NULL" in lib.nrtgpu_last_error()
    assert lib.nrtgpu_segment_set_mask_from_values(None, 5, None, 1, None) == INV
    assert lib.nrtgpu_segment_get_mask(None, 5, buf, 4) == INV and b"NULL" in lib.nrtgpu_last_error()
    assert lib.nrtgpu_segment_get_mask(None, 5, None, 4) == INV


def test_the_binding_marshals_the_three_kinds_and_refuses_what_it_can_see(lib):
    VC = api.ValueClause
    payload = np.array([0xFFC12345, 0x80000000], dtype=np.uint32)
    clauses = [VC.range_(7, "float", -0.0, np.inf), VC.exists(8), VC.in_set(9, "int", [3, -1, 3]), VC.in_set(7, "float", payload)]
    vc, keep = api._marshal_value_clauses(clauses)
    got = [(c.kind, c.field_id, c.lower_bits, c.upper_bits, c.n_values, c.reserved, bool(c.value_bits)) for c in vc]
    assert got == [(0, 7, 0x80000000, 0x7F800000, 0, 0, False), (1, 8, 0, 0, 0, 0, False), (2, 9, 0, 0, 3, 0, True), (2, 7, 0, 0, 2, 0, True)]
    assert [vc[2].value_bits[i] for i in range(3)] == [3, 0xFFFFFFFF, 3]           # any order, duplicates kept: the library sorts
    assert [vc[3].value_bits[i] for i in range(2)] == payload.tolist()             # raw bits: a NaN keeps its payload on the way in
    assert np.frombuffer(VC.in_set(9, "float", np.array([1.5, -2.0], np.float32)).value_bits, np.uint32).tolist() == [0x3FC00000, 0xC0000000]
    assert VC.range_(9, "int", -1, 3) == VC("range", 9, "int", 0xFFFFFFFF, 3)
    with pytest.raises(ValueError):
        api._marshal_value_clauses([])
    with pytest.raises(ValueError):
        api._marshal_value_clauses([VC.exists(1)] * 5)
    with pytest.raises(ValueError):
        VC.in_set(9, "int", [])
    with pytest.raises(ValueError):
        VC.in_set(9, "int", np.arange(4097, dtype=np.int32))
    with pytest.raises(ValueError):
        api._marshal_value_clauses([VC("in_set", 9, "int")])
    with pytest.raises(TypeError):
        VC.in_set(9, "int", np.array([1.0, 2.0]))              # no silent cast
    with pytest.raises(api.UnsupportedQuery):
        VC.range_(9, "long", 0, 1)
    with pytest.raises(api.UnsupportedQuery):
        VC.in_set(9, "double", [0.5])
    with pytest.raises(api.UnsupportedQuery):
        api._marshal_value_clauses([VC("prefix", 9)])


# ---- the reference against a brute-force loop ----------------------------------------------------------------------------------
def _compare(kind, a, b):
    """Integer.compare / Float.compare on raw bits, the long way."""
    if kind == "int":
        x, y = (v - 2**32 if v >= 2**31 else v for v in (a, b))
        return (x > y) - (x < y)
    x, y = (struct.unpack("<f", struct.pack("<I", v))[0] for v in (a, b))
    if x < y:
        return -1
    if x > y:
        return 1
    ia, ib = (0x7FC00000 if f != f else v for f, v in ((x, a), (y, b)))   # equal, or a NaN: floatToIntBits compared as ints
    ia, ib = (v - 2**32 if v >= 2**31 else v for v in (ia, ib))
    return (ia > ib) - (ia < ib)


def _brute(max_doc, clauses):
    words = [0] * ((max_doc + 63) // 64)
    for doc in range(max_doc):
        ok = True
        for (arity, docs, bits), clause in clauses:
            owners = range(max_doc) if docs is None else [int(d) for d in docs]
            mine = [int(b) for d, b in zip(owners, np.asarray(bits).tolist()) if d == doc]
            if clause[0] == "exists":
                passes = bool(mine)
            elif clause[0] == "range":
                passes = any(_compare(clause[1], clause[2], v) <= 0 and _compare(clause[1], v, clause[3]) <= 0 for v in mine)
            else:
                passes = any(_compare(clause[1], v, int(m)) == 0 for v in mine for m in clause[2])
            ok = ok and passes
        if ok:
            words[doc >> 6] |= 1 << (doc & 63)
    return words


EDGE = {"int": fs.VALUES["int"], "float": np.concatenate([fs.VALUES["float"][:-1], np.array([0x7FC00000, 0x7F800001, 0xFFC12345], np.uint32)])}


@pytest.mark.parametrize("kind", ["int", "float"])
def test_the_reference_agrees_with_a_brute_force_loop(kind):
    """Checks tests/_value_masks_ref.py ALONE on 200-doc columns of each arity: +-0.0, NaNs with payloads, +-inf, both int ends."""
    n = 200
    rng = np.random.default_rng(5 if kind == "int" else 6)
    pool = EDGE[kind]
    sparse_docs = np.nonzero(rng.random(n) < 0.7)[0].astype(np.int32)
    per_doc = rng.choice([0, 0, 1, 2, 5], size=n)
    multi_docs = np.repeat(np.arange(n, dtype=np.int32), per_doc)
    columns = {"dense": ("single", None, rng.choice(pool, size=n)), "sparse": ("single", sparse_docs, rng.choice(pool, size=len(sparse_docs))),
               "multi": ("multi", multi_docs, rng.choice(pool, size=len(multi_docs))), "none": ("multi", np.zeros(0, np.int32), np.zeros(0, np.uint32))}
    order = np.argsort(fs.order_key(kind, pool), kind="stable")
    lo, hi = int(pool[order[1]]), int(pool[order[-2]])
    clauses = [("exists",), ("range", kind, fs.KIND_MIN[kind], fs.KIND_MAX[kind]), ("range", kind, lo, hi), ("range", kind, hi, lo), ("range", kind, lo, lo),
               ("in_set", kind, pool[:1]), ("in_set", kind, np.array([lo, hi, lo], np.uint32)), ("in_set", kind, np.array([12345], np.uint32)), ("in_set", kind, pool)]
    if kind == "float":
        clauses += [("range", kind, 0xFF800000, 0x7F800000), ("range", kind, 0x7FC00000, 0xFFC00001), ("in_set", kind, np.array([0x80000000], np.uint32)),
                    ("in_set", kind, np.array([0], np.uint32)), ("in_set", kind, np.array([0x7FC00055], np.uint32))]
    checked = nonempty = 0
    for name, col in columns.items():
        for clause in clauses:
            words, count = ref.mask_words(n, [(col, clause)])
            exp = _brute(n, [(col, clause)])
            assert [int(w) for w in words] == exp, (name, clause)
            assert count == sum(bin(w).count("1") for w in exp)
            checked += 1
            nonempty += int(count > 0)
    both = [(columns["dense"], clauses[2]), (columns["multi"], clauses[6]), (columns["sparse"], clauses[0]), (columns["multi"], clauses[1])]
    words, count = ref.mask_words(n, both)
    assert [int(w) for w in words] == _brute(n, both) and 0 < count < n
    assert checked == 4 * len(clauses) and nonempty >= 2 * len(clauses)
    if kind == "float":   # the float identities, spelled out on one column of five docs
        col = ("single", None, np.array([0x80000000, 0, 0x7FC00000, 0xFFC12345, 0x7F800000], np.uint32))
        docs = lambda clause: np.nonzero(ref.clause_docs(5, col, clause))[0].tolist()   # noqa: E731
        assert docs(("in_set", "float", np.array([0x80000000], np.uint32))) == [0] and docs(("in_set", "float", np.array([0], np.uint32))) == [1]
        assert docs(("in_set", "float", np.array([0x7F800001], np.uint32))) == [2, 3] and docs(("exists",)) == [0, 1, 2, 3, 4]
        assert docs(("range", "float", 0xFF800000, 0x7F800000)) == [0, 1, 4] and docs(("range", "float", 0x7FC00000, 0x7FC00000)) == [2, 3]


# ---- against the stand-in runtime ------------------------------------------------------------------------------------------------
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
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mockhip", "value_masks_host.py")], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "done" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    got = dict(line.split(" ", 1) for line in r.stdout.strip().split("\n") if " " in line)
    inv, uns, state = str(INV), str(UNS), str(STATE)
    expect = {
        "range": "0 0", "exists": "0", "in_set": "0", "in_set_4096": "0", "four_mixed": "0", "column_without_values": "0", "null_out_count": "0",
        "seg_null": inv, "clauses_null": inv, "mask_id_zero": inv, "mask_id_negative": inv, "n_clauses_zero": inv, "n_clauses_five": inv,
        "kind_three": inv, "kind_negative": inv, "reserved": inv, "in_set_no_values": inv, "in_set_4097": inv, "in_set_null_values": inv,
        "range_with_n_values": inv, "exists_with_values": inv, "names_the_clause": "1",
        "unsealed": state, "invalid_before_unsealed": inv, "unsealed_before_unsupported": state,
        "column_not_resident": uns, "names_the_field": "1", "postings_field_is_no_column": uns,
        "invalid_in_clause_1_before_unsupported_in_clause_0": inv,
        "get_null_seg": inv, "get_null_bits": inv, "get_short": inv, "get_not_registered": uns, "get_short_before_not_registered": inv,
        "get_more_room": "0",
        "get_round_trips_set_mask": "1", "a_failed_call_keeps_the_old_mask_unsupported": "1 1", "a_failed_call_keeps_the_old_mask_invalid": "1 1",
        "a_rebuild_drops_the_accept_sets": "1 1", "the_rebuilt_mask_replaced_the_old": "1", "a_built_mask_is_resident_for_a_query": "1",
        "dropped_like_any_mask": uns, "device_bytes_unchanged": "1",
        "a_fork_starts_without_masks": uns, "a_forks_masks_are_its_own": "1 1", "the_parent_keeps_its_mask": "1",
    }
    assert got == expect, {k: (got.get(k), v) for k, v in expect.items() if got.get(k) != v}
