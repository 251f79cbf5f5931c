"""64-bit doc value columns without a device: the structs, the order-preserving coding and the packed sort key through
nrtgpu_sort_key64 (the very function the kernels compile) against Python's own integer compares, nrtgpu_range_accepts64 over the
edge values, the refusals that need no context, the reference against a brute-force loop, and -- against tests/mockhip -- every
refusal that needs a context, the precedence of the statuses, predicate == entry, and the fit boundary."""
import ctypes as C
import os
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest

from nrtsearch_amd import _lib, api, build

from tests import _field_sort64_ref as ref
from tests import _field_sort_ref as fs
from tests import _value_masks64_ref as mref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV, UNS, STATE = _lib.NRTGPU_ERR_INVALID_ARG, _lib.NRTGPU_ERR_UNSUPPORTED, _lib.NRTGPU_ERR_STATE
LONGS = [ref.INT64_MIN, -1, 0, 1, ref.INT64_MAX]
# -inf, -1.5, -0.0, +0.0, 4.9e-324, 3.25, +inf, then NaN in three payloads (one code)
DOUBLE_BITS = [0xFFF0000000000000, ref.bits_of("double", -1.5), 0x8000000000000000, 0, 1, ref.bits_of("double", 3.25), 0x7FF0000000000000,
               0x7FF8000000000000, 0x7FF0000000000001, 0xFFF8000000000123]


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_struct_sizes_and_symbols(lib):
    assert C.sizeof(_lib.FieldSort64) == 32 and C.sizeof(_lib.FieldDocs64) == 40 and C.sizeof(_lib.ValueClause64) == 32
    assert _lib.FieldSort64.missing_bits.offset == 8 and _lib.FieldSort64.after_bits.offset == 24
    assert _lib.FieldDocs64.value_bits.offset == 16 and _lib.FieldDocs64.total_hits.offset == 24
    for name in ("nrtgpu_segment_add_doc_values64", "nrtgpu_sort_key64", "nrtgpu_search_sorted64_batch", "nrtgpu_sorted64_supported",
                 "nrtgpu_search_docset_sorted64_batch", "nrtgpu_docset_sorted64_supported", "nrtgpu_segment_set_mask_from_values64",
                 "nrtgpu_range_accepts64"):
        assert hasattr(lib, name) and name in _lib.ABI_SYMBOLS


def _three_way(kind, x_bits, y_bits):
    """compare(y, x) as the library's coding sees it: the ordinal of a doc WITHOUT a value whose missing value is y in the window
    [x, x] -- 0 below, 1 equal, 2 above (descending key, one docid bit, doc 0: key = (ordinal + 1) << 1 | 1)."""
    key = api.sort_key64(kind, True, x_bits, x_bits, y_bits, 1, False, 0, 0)
    assert key & 1 == 1
    return (key >> 1) - 2


@pytest.mark.parametrize("kind,bits", [("long", [ref.bits_of("long", v) for v in LONGS]), ("double", DOUBLE_BITS)])
def test_the_coding_is_strictly_monotone_in_the_kinds_order(lib, kind, bits):
    for i, x in enumerate(bits):
        for j, y in enumerate(bits):
            a, b = ref.order_int(kind, y), ref.order_int(kind, x)
            assert _three_way(kind, x, y) == (a > b) - (a < b), (kind, hex(x), hex(y))
    if kind == "double":   # the three NaNs are one value, above +inf; -0.0 strictly below +0.0
        assert _three_way(kind, bits[7], bits[8]) == 0 and _three_way(kind, bits[8], bits[9]) == 0
        assert _three_way(kind, bits[6], bits[9]) == 1 and _three_way(kind, bits[3], bits[2]) == -1


def _decode(key, reverse, lo, span, db):
    """The header's packing, undone in Python: (global doc, ascending ordinal)."""
    f = key >> db
    doc = (1 << db) - 1 - (key & ((1 << db) - 1))
    return doc, (f - 1 if reverse else span + 2 - (f - 1))


def test_packed_keys_order_like_a_python_sort(lib):
    """3000 seeded cases: the key order equals (value order, docid ascending), a key is never 0, it decodes back, and the sort is
    refused exactly when span + 3 > 2^(64 - db) - 1."""
    rnd = random.Random(64)
    fit = refused = 0
    for case in range(3000):
        kind = "double" if case % 10 == 9 else "long"
        n = rnd.choice([1, 5, 64, 200])
        base = rnd.choice([0, 1000, 2**20, 2**30 - 500])
        w = rnd.choice([1, 3, 2**10, 2**32, 2**33, 2**40, 2**62])
        if kind == "long":
            start = rnd.choice([ref.INT64_MIN, ref.INT64_MAX - (w - 1), 1_700_000_000_000, -w // 2, rnd.randrange(-2**62, 2**61)])
            pool = [start + rnd.randrange(w) for _ in range(8)] + [start, start + w - 1]
            val_bits = [ref.bits_of("long", rnd.choice(pool)) for _ in range(n)]
            mn, mx = ref.bits_of("long", ref.INT64_MIN), ref.bits_of("long", ref.INT64_MAX)
        else:   # 1.5 + j ulp, or its negative: the codes of doubles of one sign and binade are consecutive integers
            w = min(w, 2**40)
            sign = rnd.choice([0, 1 << 63])
            pool = [(ref.bits_of("double", 1.5) + rnd.randrange(w)) | sign for _ in range(8)]
            val_bits = [rnd.choice(pool) for _ in range(n)]
            mn, mx = 0xFFF0000000000000, ref.CANONICAL_NAN
        has = [rnd.random() >= 0.2 for _ in range(n)]
        missing = rnd.choice([mn, mx, rnd.choice(val_bits)])
        reverse = rnd.random() < 0.5
        db = max(1, (base + n - 1).bit_length())
        present = [ref.order_int(kind, b) for b, h in zip(val_bits, has) if h]
        lo_bits = min((b for b, h in zip(val_bits, has) if h), key=lambda b: ref.order_int(kind, b), default=missing)
        hi_bits = max((b for b, h in zip(val_bits, has) if h), key=lambda b: ref.order_int(kind, b), default=missing)
        span = (max(present) - min(present)) if present else 0
        fits = span + 3 <= 2**(64 - db) - 1
        if not fits:
            with pytest.raises(_lib.NrtGpuError) as e:
                api.sort_key64(kind, reverse, lo_bits, hi_bits, missing, db, has[0], val_bits[0], base)
            assert e.value.code == UNS and f"{db}-bit docids leave {64 - db}" in str(e.value), str(e.value)
            refused += 1
            continue
        fit += 1
        keys = [api.sort_key64(kind, reverse, lo_bits, hi_bits, missing, db, h, b, base + i) for i, (b, h) in enumerate(zip(val_bits, has))]
        assert all(0 < k < 2**64 for k in keys) and len(set(keys)) == n
        sorts_as = [ref.order_int(kind, b if h else missing) for b, h in zip(val_bits, has)]
        expect = sorted(range(n), key=lambda i: (-sorts_as[i] if reverse else sorts_as[i], i))
        assert sorted(range(n), key=lambda i: -keys[i]) == expect, (case, kind, n, base, w, reverse)
        lo_o, m_o = ref.order_int(kind, lo_bits), ref.order_int(kind, missing)
        for i, k in enumerate(keys):
            doc, u = _decode(k, reverse, lo_o, span, db)
            assert doc == base + i
            if 1 <= u <= span + 1:
                assert lo_o + (u - 1) == sorts_as[i]
            else:   # a sentinel: only the missing value lies outside the window
                assert not has[i] and (u == 0) == (m_o < lo_o) and (u == span + 2) == (m_o > lo_o + span)
    assert fit > 2000 and refused > 100, (fit, refused)


def test_sort_key64_refuses_bad_arguments_before_the_fit(lib):
    ok = dict(kind=2, reverse=0, lo=ref.bits_of("long", 5), hi=ref.bits_of("long", 9), missing=0, db=10, has=1, value=ref.bits_of("long", 7), doc=3)
    out = C.c_uint64(0)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.nrtgpu_sort_key64(a["kind"], a["reverse"], C.c_uint64(a["lo"]), C.c_uint64(a["hi"]), C.c_uint64(a["missing"]), a["db"], a["has"],
                                     C.c_uint64(a["value"]), a["doc"], a.get("out", C.byref(out)))

    assert call() == 0 and out.value != 0
    for bad in (dict(kind=1), dict(kind=4), dict(reverse=2), dict(has=2), dict(has=-1), dict(db=0), dict(db=32), dict(doc=-1), dict(doc=1 << 10),
                dict(lo=ref.bits_of("long", 10)), dict(value=ref.bits_of("long", 4)), dict(value=ref.bits_of("long", 10)), dict(out=None)):
        assert call(**bad) == INV, bad
    # a window that does not fit: unsupported, with the bits; an invalid argument beside it wins
    wide = dict(lo=ref.bits_of("long", ref.INT64_MIN), hi=ref.bits_of("long", ref.INT64_MAX), value=0)
    assert call(**wide) == UNS and b"span needs 65 bits, 10-bit docids leave 54" in lib.nrtgpu_last_error()
    assert call(**wide, reverse=2) == INV
    assert call(lo=0, hi=2**40 - 1 - 3 + 1, value=0, db=24) == UNS and b"span needs 41 bits, 24-bit docids leave 40" in lib.nrtgpu_last_error()
    assert call(lo=0, hi=2**40 - 1 - 3, value=0, db=24) == 0
    # FLOAT64 {-1.0, 1.0}: doubles of different sign never fit
    assert call(kind=3, lo=ref.bits_of("double", -1.0), hi=ref.bits_of("double", 1.0), value=ref.bits_of("double", 1.0)) == UNS


def test_range_accepts64_over_the_edge_values(lib):
    for kind, bits in (("long", [ref.bits_of("long", v) for v in LONGS]), ("double", DOUBLE_BITS)):
        for lo in bits:
            for hi in bits:
                for v in bits:
                    exp = ref.order_int(kind, lo) <= ref.order_int(kind, v) <= ref.order_int(kind, hi)
                    assert api.range_accepts64(kind, lo, hi, v) is exp, (kind, hex(lo), hex(hi), hex(v))
    inf, ninf, nan = 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000000000
    assert not api.range_accepts64("double", ninf, inf, 0xFFF8000000000123)    # [-inf, +inf] drops the NaN docs
    assert api.range_accepts64("double", nan, nan, 0x7FF0000000000001)         # [NaN, NaN] keeps only them
    assert not api.range_accepts64("double", nan, nan, inf)
    assert not api.range_accepts64("double", 0, 0, 0x8000000000000000) and api.range_accepts64("double", 0x8000000000000000, 0, 0)
    out = C.c_int32(0)
    assert lib.nrtgpu_range_accepts64(1, C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.byref(out)) == INV
    assert lib.nrtgpu_range_accepts64(2, C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), None) == INV


def test_null_arguments_are_refused_without_a_device(lib):
    v = np.zeros(4, dtype=np.int64)
    assert lib.nrtgpu_segment_add_doc_values64(None, 0, 2, 4, None, v.ctypes.data) == INV
    q, s, out, d, vc = _lib.Bm25Query(), _lib.FieldSort64(), _lib.FieldDocs64(), _lib.DocsetQuery(), _lib.ValueClause64()
    assert lib.nrtgpu_search_sorted64_batch(None, None, None, 0, C.byref(q), C.byref(s), 1, C.byref(out)) == INV
    assert lib.nrtgpu_sorted64_supported(None, None, 0, C.byref(q), C.byref(s)) == INV
    assert lib.nrtgpu_search_docset_sorted64_batch(None, None, None, 0, C.byref(d), C.byref(s), 1, C.byref(out)) == INV
    assert lib.nrtgpu_docset_sorted64_supported(None, None, 0, C.byref(d), C.byref(s)) == INV
    assert lib.nrtgpu_segment_set_mask_from_values64(None, 5, C.byref(vc), 1, None) == INV
    assert b"NULL" in lib.nrtgpu_last_error()


def test_the_binding_refuses_what_it_can_see(lib):
    seg = api.GpuSegment.__new__(api.GpuSegment)   # (no context: the checks below come before the library is called)
    seg._h = None
    with pytest.raises(TypeError):
        seg.add_doc_values64(7, "long", np.zeros(4, dtype=np.int32))
    with pytest.raises(TypeError):
        seg.add_doc_values64(7, "double", np.zeros(4, dtype=np.float32))
    with pytest.raises(ValueError):
        seg.add_doc_values64(7, "long", np.zeros(4, dtype=np.int64), np.arange(3))
    with pytest.raises(KeyError):
        seg.add_doc_values64(7, "int", np.zeros(4, dtype=np.int64))
    with pytest.raises(api.UnsupportedQuery):
        api.ValueClause64.range_(9, "int", 0, 1)
    with pytest.raises(api.UnsupportedQuery):
        api._field_sorts64([api.SortField64(7, "float")], None, 1)
    with pytest.raises(ValueError):
        seg.set_mask_from_values64(5, [])
    assert api._value_bits64("double", -0.0) == 1 << 63 and api._value_bits64("long", -1) == 2**64 - 1
    t = api.TopFieldDocs64(np.zeros(1, np.int32), np.array([-0.0], np.float64), 1, False)
    assert t.value_bits.dtype == np.uint64 and t.value_bits.tolist() == [1 << 63]
    c = api.ValueClause64.range_(9, "long", -5, 2**40)
    assert (c.lower_bits, c.upper_bits) == (2**64 - 5, 2**40)


@pytest.mark.parametrize("kind", ["long", "double"])
def test_the_reference_agrees_with_a_brute_force_sort(kind):
    """Checks tests/_field_sort64_ref.py alone, against Python's sorted() over per-doc tuples on a 200-doc index: it passes
    without the feature."""
    corpus = fs.make_corpus([150, 50], {1: 0.6, 2: 0.3}, seed=3, delete_fraction=0.05)
    rng = np.random.default_rng(4)
    pool = np.array([ref.bits_of("long", v) for v in LONGS + [1_700_000_000_000, 1_700_000_000_000 + 2**32]] if kind == "long" else DOUBLE_BITS, dtype=np.uint64)
    d0 = np.nonzero(rng.random(150) < 0.7)[0].astype(np.int32)
    columns = [(d0, rng.choice(pool, size=len(d0))), None]
    for reverse in (False, True):
        for missing in (int(pool[0]), int(pool[-3]), int(pool[2])):
            hits = ref.text_hits(corpus, (1, 2), 1)
            rows = []
            for si, seg in enumerate(corpus.segments):
                value = {}
                if columns[si] is not None:
                    value = {int(d): int(b) for d, b in zip(columns[si][0], columns[si][1])}
                for d in range(seg.max_doc):
                    live = (int(seg.live_bits[d >> 6]) >> (d & 63)) & 1
                    matched = any(d in seg.postings(t)[0].tolist() for t in (1, 2))
                    if live and matched:
                        b = value.get(d, missing)
                        o = ref.order_int(kind, b)
                        rows.append((-o if reverse else o, seg.doc_base + d, int(ref.canonical_bits(kind, [b])[0])))
            rows.sort()
            docs, bits, total, gte = ref.search(corpus, hits, columns, kind, 20, reverse, missing)
            assert total == len(rows) and not gte
            assert docs.tolist() == [r[1] for r in rows[:20]] and bits.tolist() == [r[2] for r in rows[:20]]
            after = (rows[7][1], rows[7][2])
            docs, bits, total2, _ = ref.search(corpus, hits, columns, kind, 5, reverse, missing, after=after)
            assert total2 == total and docs.tolist() == [r[1] for r in rows[8:13]]
    # the mask reference against a loop
    col = (d0, columns[0][1])
    for clause in (("exists",), ("range", int(pool[1]), int(pool[4])), ("range", int(pool[4]), int(pool[1]))):
        got = fs._bits(mref.mask(150, [(col, kind, clause)]), 150)
        value = {int(d): int(b) for d, b in zip(*col)}
        for d in range(150):
            exp = d in value and (clause[0] == "exists" or ref.order_int(kind, clause[1]) <= ref.order_int(kind, value[d]) <= ref.order_int(kind, clause[2]))
            assert bool(got[d]) == exp


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
    e.pop("NRTGPU_PACKED_POSTINGS", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mockhip", "field_sort64_host.py")], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "done" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    got = dict(line.split(" ", 1) for line in r.stdout.strip().split("\n") if " " in line)
    inv, uns, state, ok = str(INV), str(UNS), str(STATE), "0"
    expect = {
        # the column
        "add_kind_0": inv, "add_kind_4": inv, "add_n_negative": inv, "add_n_too_many": inv, "add_null_docs_short": inv, "add_null_values": inv,
        "add_docs_descending": inv, "add_docs_out_of_range": inv, "add_ok_sparse": ok, "add_second_64": inv, "add_second_32": inv,
        "add_second_multi": inv, "add_64_on_a_32_field": inv, "add_empty_column": ok, "add_after_seal": state, "device_bytes_counts_8_per_doc": "1",
        # the sorted entries: what runs, the 32-bit table, the new refusals; text == predicate and docset == predicate on each (both
        # statuses are printed)
        "text_runs": "0 0", "docset_runs": "0 0", "text_runs_without_a_value_anywhere": "0 0",
        "reverse_2": f"{inv} {inv}", "has_after_2": f"{inv} {inv}", "after_doc_negative": f"{inv} {inv}", "query_has_after": f"{inv} {inv}",
        "num_hits_0": f"{inv} {inv}", "kinds_differ": f"{inv} {inv}", "kinds_differ_names_them": "1",
        "no_column": f"{uns} {uns}", "narrow_column": f"{uns} {uns}", "narrow_names_the_32_bit_entry": "1",
        "multi_column": f"{uns} {uns}", "dismax": f"{uns} {uns}", "must_next_to_should": f"{uns} {uns}", "min_competitive": f"{uns} {uns}",
        "filter_mask_not_resident": f"{uns} {uns}", "does_not_fit": f"{uns} {uns}", "does_not_fit_says": "1",
        "invalid_in_query_1_before_unsupported_in_query_0": inv,
        "docset_reverse_2": f"{inv} {inv}", "docset_k_0": f"{inv} {inv}", "docset_no_column": f"{uns} {uns}", "docset_narrow_column": f"{uns} {uns}",
        "docset_narrow_names_the_32_bit_entry": "1", "docset_range_32_beside": "0 0", "docset_range_over_the_64_bit_column": f"{uns} {uns}",
        "docset_mask_not_resident": f"{uns} {uns}", "docset_does_not_fit": f"{uns} {uns}", "docset_kinds_differ": f"{inv} {inv}",
        # the fit boundary: a leaf at doc base 2^30 with 3000 docs: db = 31, 33 value bits -- a span of 2^33 - 4 is accepted, 2^33 - 3
        # refused.  The predicate has no doc bases and answers for the leaves in order (base 0: db = 12, both fit); with the leaf AT
        # base 0 the boundary is 2^52 - 4 / 2^52 - 3 and the predicate and the entry agree.
        "boundary_span_fits": ok, "boundary_span_plus_one": uns, "boundary_says": "1", "boundary_predicate_answers_for_in_order_bases": ok,
        "boundary_docset_fits": ok, "boundary_docset_plus_one": uns,
        "inorder_boundary_span_fits": "0 0", "inorder_boundary_span_plus_one": f"{uns} {uns}", "inorder_boundary_docset_fits": "0 0",
        "inorder_boundary_docset_plus_one": f"{uns} {uns}",
        # the 32-bit entries over a 64-bit column
        "sorted32_over_64": f"{uns} {uns}", "sorted32_names_the_entry": "1", "terms32_over_64": f"{uns} {uns}", "terms32_says_buckets": "1",
        "docset_sorted32_over_64": f"{uns} {uns}", "docset_terms32_over_64": f"{uns} {uns}", "docset_range32_over_64": f"{uns} {uns}",
        "mask32_over_64": uns, "mask32_names_the_entry": "1",
        # masks from 64-bit columns
        "mask_range": "0 0", "mask_exists": "0", "mask_two_clauses": "0", "mask_null_out_count": ok,
        "mask_seg_null": inv, "mask_clauses_null": inv, "mask_id_zero": inv, "mask_n_zero": inv, "mask_n_five": inv, "mask_kind_in_set": inv,
        "mask_kind_negative": inv, "mask_reserved": inv, "mask_unsealed": state, "mask_invalid_before_unsealed": inv,
        "mask_unsealed_before_unsupported": state, "mask64_column_not_resident": uns, "mask_over_a_32_bit_column": uns, "mask_over_a_multi_column": uns,
        "mask_names_the_32_bit_entry": "1", "mask_invalid_in_clause_1_first": inv, "mask_failed_call_keeps_the_old": "1 1",
        "mask_device_bytes_unchanged": "1", "mask_usable_as_a_filter": "0 0",
    }
    assert got == expect, {k: (got.get(k), v) for k, v in expect.items() if got.get(k) != v} | {k: got[k] for k in got if k not in expect}
