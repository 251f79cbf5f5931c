"""Doc-set requests, the part that needs no device: the structs' sizes, the range rule the kernels compile (nrtgpu_range_accepts)
over the edge values of both kinds, the NumPy reference of the GPU tests (tests/_docset_ref.py) against a brute-force Python loop,
the refusals decided before any device is touched, and -- against tests/mockhip -- every refusal that needs a context, with the
predicates agreeing and the precedence of the statuses."""
import ctypes as C
import itertools
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

from nrtsearch_amd import _lib, api, build

from tests import _docset_ref as ref
from tests import _field_sort_ref as fs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV, UNS, STATE = _lib.NRTGPU_ERR_INVALID_ARG, _lib.NRTGPU_ERR_UNSUPPORTED, _lib.NRTGPU_ERR_STATE


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_struct_sizes(lib):
    assert C.sizeof(_lib.RangeClause) == 16 and _lib.RangeClause.upper_bits.offset == 8 and _lib.RangeClause.reserved.offset == 12
    assert C.sizeof(_lib.DocsetQuery) == 56
    for name, off in (("filter_mask", 0), ("must_not_mask", 4), ("n_more_filters", 8), ("n_more_must_not", 12), ("more_filters", 16),
                      ("more_must_not", 24), ("n_ranges", 32), ("k", 36), ("ranges", 40), ("total_hits_threshold", 48), ("reserved", 52)):
        assert getattr(_lib.DocsetQuery, name).offset == off, name
    assert _lib.NRTGPU_MAX_RANGES == 4
    for sym in ("nrtgpu_search_docset_sorted_batch", "nrtgpu_docset_sorted_supported", "nrtgpu_count_docset_terms_batch",
                "nrtgpu_count_docset_terms_supported", "nrtgpu_range_accepts"):
        assert sym in _lib.ABI_SYMBOLS and getattr(lib, sym) is not None


# ---- the range rule, restated the long way -------------------------------------------------------------------------------------
def _float_compare(a_bits, b_bits):
    """Float.compare on raw bits, the long way."""
    a, b = struct.unpack("<f", struct.pack("<I", a_bits))[0], struct.unpack("<f", struct.pack("<I", b_bits))[0]
    if a < b:
        return -1
    if a > b:
        return 1
    ia = 0x7FC00000 if a != a else a_bits   # equal, or a NaN: floatToIntBits (every NaN collapsed) compared as ints
    ib = 0x7FC00000 if b != b else b_bits
    ia = ia - 2**32 if ia >= 2**31 else ia
    ib = ib - 2**32 if ib >= 2**31 else ib
    return (ia > ib) - (ia < ib)


def _int_compare(a_bits, b_bits):
    a = a_bits - 2**32 if a_bits >= 2**31 else a_bits
    b = b_bits - 2**32 if b_bits >= 2**31 else b_bits
    return (a > b) - (a < b)


def _keeps(kind, lo, hi, v):
    cmp = _int_compare if kind == "int" else _float_compare
    return cmp(lo, v) <= 0 and cmp(v, hi) <= 0


EDGE_BITS = {"int": fs.VALUES["int"].tolist(),
             "float": fs.VALUES["float"].tolist()[:-1] + [0x7FC00000, 0x7F800001, 0xFFFFFFFF]}   # NaN with three payloads


@pytest.mark.parametrize("kind", ["int", "float"])
def test_range_accepts_is_the_restated_compare_over_all_edge_triples(lib, kind):
    bits = EDGE_BITS[kind]
    empty = kept = 0
    for lo, hi, v in itertools.product(bits, repeat=3):
        exp = _keeps(kind, lo, hi, v)
        assert api.range_accepts(kind, lo, hi, v) is exp, (kind, hex(lo), hex(hi), hex(v))
        assert bool(ref.range_keeps(kind, lo, hi, [v])[0]) is exp, "the reference of the GPU tests disagrees with the long way"
        cmp = _int_compare if kind == "int" else _float_compare
        empty += int(cmp(lo, hi) > 0)
        kept += int(exp)
        if cmp(lo, hi) > 0:
            assert not exp   # an empty range keeps nothing
    assert empty > 0 and kept > 0
    if kind == "float":
        nz, pz, inf, ninf, nan = 0x80000000, 0x00000000, 0x7F800000, 0xFF800000, 0x7FC00000
        assert api.range_accepts("float", pz, pz, pz) and not api.range_accepts("float", pz, pz, nz)       # -0.0 < +0.0
        assert api.range_accepts("float", nz, pz, nz) and not api.range_accepts("float", pz, nz, pz)
        assert not api.range_accepts("float", ninf, inf, nan) and api.range_accepts("float", nan, nan, 0xFFC00001)
        assert api.range_accepts("float", ninf, nan, inf)
    else:
        assert api.range_accepts("int", 0x80000000, 0x7FFFFFFF, 0xFFFFFFFF) and not api.range_accepts("int", 0, 0x7FFFFFFF, 0xFFFFFFFF)


def test_range_accepts_refusals(lib):
    out = C.c_int32(7)
    for kind in (2, -1):
        assert lib.nrtgpu_range_accepts(kind, 0, 0, 0, C.byref(out)) == INV and len(lib.nrtgpu_last_error()) > 10
    assert lib.nrtgpu_range_accepts(0, 0, 0, 0, None) == INV
    assert lib.nrtgpu_range_accepts(1, 0, 0, 0, C.byref(out)) == 0 and out.value == 1


# ---- the reference against a brute-force loop ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    """200 docs in leaves of 130, 50 and 20; columns on 80 % of leaf 0, all of leaf 1, absent from leaf 2; two masks."""
    corpus = fs.make_corpus([130, 50, 20], {ref.ALL: 1.0}, seed=11, delete_fraction=0.05)
    rng = np.random.default_rng(12)
    cols = {}
    for name, kind in (("int", "int"), ("float", "float"), ("int2", "int")):
        d0 = np.nonzero(rng.random(130) < 0.8)[0].astype(np.int32)
        cols[name] = [(d0, rng.choice(fs.VALUES[kind], size=len(d0))), (None, rng.choice(fs.VALUES[kind], size=50)), None]
    masks = {mid: [ref.pack(rng.random(s.max_doc) < dens) for s in corpus.segments] for mid, dens in ((5, 0.7), (6, 0.2))}
    return corpus, cols, masks


def _brute_hits(corpus, filters, must_nots, ranges):
    """[(leaf, doc)] by a Python loop over every doc."""
    hits = []
    for si, seg in enumerate(corpus.segments):
        tables = []
        for kind, columns, lo, hi in ranges:
            col = {}
            if columns[si] is not None:
                cd, cv = columns[si]
                col = {int(d): int(v) for d, v in zip(range(seg.max_doc) if cd is None else cd.tolist(), np.asarray(cv).tolist())}
            tables.append((kind, col, lo, hi))
        for doc in range(seg.max_doc):
            bit = lambda words: (int(words[doc >> 6]) >> (doc & 63)) & 1   # noqa: E731
            if seg.live_bits is not None and not bit(seg.live_bits):
                continue
            if any(not bit(m[si]) for m in filters) or any(bit(m[si]) for m in must_nots):
                continue
            if all(doc in col and _keeps(kind, lo, hi, col[doc]) for kind, col, lo, hi in tables):
                hits.append((si, doc))
    return hits


def test_the_reference_agrees_with_a_brute_force_loop(small):
    """Checks tests/_docset_ref.py ALONE (it passes without the feature): the hit set, then one sorted page and one count map."""
    corpus, cols, masks = small
    I, F = fs.VALUES["int"].tolist(), fs.VALUES["float"].tolist()
    range_sets = [
        [], [("int", cols["int"], I[1], I[3])], [("float", cols["float"], F[2], F[5])], [("int", cols["int"], I[3], I[1])],
        [("int", cols["int"], I[0], I[4])], [("float", cols["float"], F[0], F[7])], [("float", cols["float"], F[7], F[7])],
        [("float", cols["float"], F[3], F[3])], [("float", cols["float"], F[0], F[6])],
        [("int", cols["int"], I[1], I[4]), ("float", cols["float"], F[1], F[6]), ("int2", cols["int2"], I[0], I[3]), ("int", cols["int"], I[2], I[4])],
    ]
    range_sets = [[(("int" if k == "int2" else k), c, lo, hi) for k, c, lo, hi in rs] for rs in range_sets]
    checked = nonempty = 0
    for filters, must_nots in (([], []), ([masks[5]], []), ([masks[5]], [masks[6]])):
        for rs in range_sets:
            exp = _brute_hits(corpus, filters, must_nots, rs)
            words = ref.hit_set(corpus, filters, must_nots, rs)
            got = [(si, int(d)) for si, seg in enumerate(corpus.segments) for d in np.nonzero(fs._bits(words[si], seg.max_doc))[0]]
            assert got == exp
            nonempty += int(len(exp) > 0)
            for kind in ("int", "float"):
                docs, bits, total, gte = ref.search(corpus, words, cols[kind], kind, 300, False, fs.KIND_MAX[kind])
                assert total == len(exp) == len(docs) and not gte
                assert sorted(docs.tolist()) == sorted(corpus.segments[si].doc_base + d for si, d in exp)
                keys = fs.order_key(kind, bits)
                assert np.all(np.diff(keys) >= 0) and all(keys[i] < keys[i + 1] or docs[i] < docs[i + 1] for i in range(len(docs) - 1))
                vb, vc, nb, tot, hwv, ovf = ref.count(corpus, words, cols[kind], kind)
                valued = sum(1 for si, d in exp if cols[kind][si] is not None and (cols[kind][si][0] is None or d in set(cols[kind][si][0].tolist())))
                assert (tot, hwv, ovf, int(vc.sum())) == (len(exp), valued, 0, valued) and nb == len(vb)
            checked += 1
    assert checked == 30 and nonempty >= 18


# ---- refusals that need no device ----------------------------------------------------------------------------------------------
def test_null_arguments_are_refused_before_any_device_work(lib):
    d, s, t, fo, to = _lib.DocsetQuery(), _lib.FieldSort(), _lib.TermsCount(0, 16), _lib.FieldDocs(), _lib.TermCounts()
    assert lib.nrtgpu_search_docset_sorted_batch(None, None, None, 0, C.byref(d), C.byref(s), 1, C.byref(fo)) == INV
    assert b"NULL" in lib.nrtgpu_last_error()
    assert lib.nrtgpu_docset_sorted_supported(None, None, 0, C.byref(d), C.byref(s)) == INV
    assert lib.nrtgpu_count_docset_terms_batch(None, None, None, 0, C.byref(d), C.byref(t), 1, C.byref(to)) == INV
    assert lib.nrtgpu_count_docset_terms_supported(None, None, 0, C.byref(d), C.byref(t)) == INV
    assert b"NULL" in lib.nrtgpu_last_error()


def test_the_binding_marshals_and_refuses_what_it_can_see(lib):
    top = api.TopScoreDocCollectorManager(10)
    d = api.DocSetQuery((api.MaskFilter(5), api.MaskFilter(8)), (api.MaskFilter(6),), (api.RangeClause(7, "float", -0.0, np.inf), api.RangeClause(9, "int", -1, 3)))
    ds, keep = api._marshal_docsets([d, api.DocSetQuery()], [top, api.TopScoreDocCollectorManager(3, None, 50)])
    q = ds[0]
    assert (q.filter_mask, q.must_not_mask, q.n_more_filters, q.n_more_must_not, q.n_ranges, q.k, q.total_hits_threshold, q.reserved) == (5, 6, 1, 0, 2, 10, 1000, 0)
    assert q.more_filters[0] == 8 and (q.ranges[0].field_id, q.ranges[0].lower_bits, q.ranges[0].upper_bits, q.ranges[0].reserved) == (7, 0x80000000, 0x7F800000, 0)
    assert (q.ranges[1].field_id, q.ranges[1].lower_bits, q.ranges[1].upper_bits) == (9, 0xFFFFFFFF, 3)
    assert (ds[1].filter_mask, ds[1].n_ranges, ds[1].k, ds[1].total_hits_threshold) == (0, 0, 3, 50) and not ds[1].ranges
    with pytest.raises(ValueError):
        api._marshal_docsets([d], [])
    with pytest.raises(api.UnsupportedQuery):
        api._marshal_docsets([api.DocSetQuery(ranges=(api.RangeClause(7, "long", 0, 1),))], [top])
    with pytest.raises(api.UnsupportedQuery):
        api._marshal_docsets([d], [api.TopScoreDocCollectorManager(10, api.ScoreDoc(3, 1.0))])
    with pytest.raises(ValueError):
        api._docset_sorts([api.SortField(7)], None, 2)
    with pytest.raises(api.UnsupportedQuery):
        api._docset_terms([d], [api.TermsCollector(7, 10, True, "long")], 16, None)
    with pytest.raises(ValueError):
        api._docset_terms([d], [api.TermsCollector(7, 10)], [16, 16], None)


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
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mockhip", "docset_host.py")], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "done" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    got = dict(line.split(" ", 1) for line in r.stdout.strip().split("\n") if " " in line)
    ok, I, U = "0 0 | 0 0", f"{INV} 1 | {INV} 1", f"{UNS} 1 | {UNS} 1"   # sorted | counted: the status (the predicate agreeing), the reason names the query
    expect = {
        "match_all": ok, "masks": ok, "four_ranges": ok, "empty_range": ok, "k_1024": ok, "threshold_int_max": ok, "eight_masks": ok,
        "batch_of_4": "4 0 | 4 0", "diagnostics": "0 1 0", "stats_counted": "1", "plan_items": "1",
        "k_zero": I, "k_1025": I, "threshold_negative": I, "n_ranges_5": I, "n_ranges_negative": I, "ranges_null": I, "clause_reserved": I,
        "query_reserved": I, "mask_negative": I, "n_more_negative": I, "more_null": I, "nine_masks": I, "more_id_zero": I,
        "range_kinds_differ": I, "kinds_differ_text": "1",
        "reverse_2": f"{INV} 1", "has_after_2": f"{INV} 1", "after_doc_negative": f"{INV} 1", "sort_kinds_differ": f"{INV} 1",
        "max_buckets_0": f"{INV} 1", "max_buckets_65537": f"{INV} 1", "capacity_below_max_buckets": str(INV), "null_arrays": str(INV),
        "count_kinds_differ": f"{INV} 1", "batch_of_257_at_65536": f"{INV}/0 1", "names_the_limit": "1",
        "no_column_on_any_leaf": f"{UNS} 1 | {UNS} 1", "range_column_on_no_leaf": U, "mask_not_resident": U, "must_not_mask_not_resident": U,
        "more_mask_not_resident": U,
        "invalid_before_unsupported": I, "invalid_in_query_1_before_unsupported_in_query_0": I,
        "null_docsets": f"{INV} | {INV}", "null_records": f"{INV} | {INV}", "null_out": f"{INV} | {INV}", "null_supported": f"{INV} | {INV}",
        "batch_above_max_batch": f"{INV} | {INV}", "unsealed_leaf": f"{STATE} | {STATE}",
        "flag_no_fixed_point": ok, "flag_packed_postings": ok, "still_answers": ok,
    }
    assert got == expect, {k: (got.get(k), v) for k, v in expect.items() if got.get(k) != v}
