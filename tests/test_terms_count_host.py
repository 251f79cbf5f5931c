"""The terms aggregation (nrtgpu_count_terms_batch) without a GPU: the structs' sizes, the NumPy reference of the GPU tests
(tests/_terms_count_ref.py) against a brute-force Python dict, api.fill_bucket_result against a transcription of the reference's
priority-queue loop, the refusals decided before any device is touched, and -- against the stand-in runtime of tests/mockhip --
what plans and runs and every refusal that needs a context.

test_the_reference_agrees_with_a_brute_force_dict checks the test reference only and passes without the feature; every other
test here needs the new symbols or the new binding."""
import ctypes as C
import heapq
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

from nrtsearch_amd import _lib, api, build

from tests import _field_sort_ref as fs
from tests import _terms_count_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV, UNS = _lib.NRTGPU_ERR_INVALID_ARG, _lib.NRTGPU_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_struct_sizes(lib):
    assert C.sizeof(_lib.TermsCount) == 8 and _lib.TermsCount.max_buckets.offset == 4
    assert C.sizeof(_lib.TermCounts) == 48
    offsets = {n: getattr(_lib.TermCounts, n).offset for n, _ in _lib.TermCounts._fields_}
    assert offsets == {"n_buckets": 0, "capacity": 4, "value_bits": 8, "counts": 16, "total_hits": 24, "hits_with_value": 32, "overflowed": 40,
                       "reserved": 44}
    assert _lib.NRTGPU_MAX_TERM_BUCKETS == 65536
    assert {"nrtgpu_count_terms_batch", "nrtgpu_count_terms_supported"} <= set(_lib.ABI_SYMBOLS)


# ---- the reference against a dict ------------------------------------------------------------------------------------------
def _float_of(bits):
    return struct.unpack("<f", struct.pack("<I", bits))[0]


def _float_compare_key(bits):
    """Float.compare as a sort key, the long way: numeric order, -0.0 below +0.0, NaN (one value) above everything."""
    v = _float_of(bits)
    if v != v:
        return (2, 0.0, 0)
    return (1, v, 0 if bits >> 31 else 1) if v == 0.0 else (1, v, 0)


def _brute(corpus, columns, kind, terms, need, max_buckets):
    table, total = {}, 0
    for si, seg in enumerate(corpus.segments):
        col = {}
        if columns[si] is not None:
            cd, cv = columns[si]
            col = {int(d): int(v) for d, v in zip(range(seg.max_doc) if cd is None else cd.tolist(), np.asarray(cv).tolist())}
        holds = {t: set(seg.postings(t)[0].tolist()) for t in set(terms)}
        for doc in range(seg.max_doc):
            if seg.live_bits is not None and not (int(seg.live_bits[doc >> 6]) >> (doc & 63)) & 1:
                continue
            if sum(1 for t in terms if doc in holds[t]) < max(need, 1):
                continue
            total += 1
            if doc in col:
                b = col[doc]
                if kind == "float" and (b & 0x7FFFFFFF) > 0x7F800000:
                    b = 0x7FC00000   # Float.floatToIntBits
                table[b] = table.get(b, 0) + 1
    if len(table) > max_buckets:
        return [], [], 0, total, -1, 1
    if kind == "int":
        keys = sorted(table, key=lambda b: b - 2**32 if b >= 2**31 else b)
    else:
        keys = sorted(table, key=_float_compare_key)
    return keys, [table[b] for b in keys], len(keys), total, sum(table.values()), 0


@pytest.fixture(scope="module")
def small():
    """200 docs in leaves of 130, 50 and 20; the column on 80 % of leaf 0, all of leaf 1, absent from leaf 2."""
    corpus = fs.make_corpus([130, 50, 20], {1: 0.6, 2: 0.4, 3: 0.3}, seed=11, delete_fraction=0.05)
    rng = np.random.default_rng(12)
    nans = np.array([0x7FC00000, 0x7FC00001, 0xFFC00000, 0x7F800001], dtype=np.uint32)
    cols = {}
    for kind in ("int", "float"):
        pool = np.concatenate([fs.VALUES[kind], nans]) if kind == "float" else fs.VALUES[kind]
        d0 = np.nonzero(rng.random(130) < 0.8)[0].astype(np.int32)
        cols[kind] = [(d0, rng.choice(pool, size=len(d0))), (None, rng.choice(pool, size=50)), None]
    return corpus, cols


@pytest.mark.parametrize("kind", ["int", "float"])
def test_the_reference_agrees_with_a_brute_force_dict(small, kind):
    """(Checks the test reference alone: passes without the feature.)"""
    corpus, cols = small
    checked = overflowed = 0
    for terms, need in (((1,), 1), ((1, 2, 3), 1), ((1, 2, 3), 2), ((1, 2), 2), ((2, 2, 3), 2), ((99,), 1)):
        distinct = _brute(corpus, cols[kind], kind, terms, need, 10**6)[2]
        for max_buckets in (65536, max(distinct, 1), max(distinct - 1, 1), 1):
            exp = _brute(corpus, cols[kind], kind, terms, need, max_buckets)
            bits, counts, n, total, valued, over = ref.count(corpus, cols[kind], kind, terms, need, max_buckets)
            assert (bits.tolist(), counts.tolist(), n, total, valued, over) == exp, (kind, terms, need, max_buckets)
            assert over == int(distinct > max_buckets)
            checked += 1
            overflowed += over
    assert checked == 24 and overflowed >= 5
    if kind == "float":   # the NaN payloads fell in one bucket, the zeros in two
        bits = ref.count(corpus, cols[kind], kind, (1, 2, 3), 1)[0].tolist()
        assert bits.count(0x7FC00000) == 1 and 0x80000000 in bits and 0 in bits and bits[-1] == 0x7FC00000
        assert all((b & 0x7FFFFFFF) <= 0x7F800000 or b == 0x7FC00000 for b in bits)


# ---- fill_bucket_result ---------------------------------------------------------------------------------------------------
def _reference_fill(entries, size, desc):
    """TermsCollectorManager.fillBucketResultByCount (:430-483), line by line, over `entries` in ANY iteration order: a priority
    queue whose head is the worst kept bucket, the decider that replaces the head, otherCounts, the reversed poll order."""
    if not entries or size <= 0:
        return [], 0, 0
    sign = 1 if desc else -1           # the comparator: by count, reversed for ASC
    heap, seq = [], 0                  # (sign * count, insertion number, key, count): the head is the worst kept entry
    other, head = 0, -1
    for key, count in entries:
        if len(heap) < size:
            heapq.heappush(heap, (sign * count, seq, key, count))
            head = heap[0][3]
        elif (count > head) if desc else (count < head):
            worst = heapq.heappop(heap)
            other += worst[3]
            heapq.heappush(heap, (sign * count, seq, key, count))
            head = heap[0][3]
        else:
            other += count
        seq += 1
    buckets = []
    while heap:
        e = heapq.heappop(heap)
        buckets.insert(0, (e[2], e[3]))   # addFirst
    return buckets, len(entries), other


def test_fill_bucket_result_is_the_reference_loop(lib):
    rng = np.random.default_rng(4)
    checked = 0
    for n in (1, 2, 5, 37, 400):
        values = np.sort(rng.choice(100_000, size=n, replace=False)).astype(np.int32)
        counts = rng.permutation(np.arange(1, n + 1)).astype(np.int32) * 3   # distinct counts: no tie anywhere, so none at the cut
        entries = list(zip(values.tolist(), counts.tolist()))
        for size in (0, 1, 3, n - 1, n, n + 5):
            for desc in (True, False):
                for order in (entries, entries[::-1], [entries[i] for i in rng.permutation(n)]):   # the hash map's order is arbitrary
                    exp = _reference_fill(order, size, desc)
                    got = api.fill_bucket_result(values, counts, size, desc)
                    assert (got.buckets, got.total_buckets, got.total_other_counts) == exp, (n, size, desc)
                    checked += 1
    assert checked == 5 * 6 * 2 * 3
    # ties at the cut: the value ascending breaks them (one of the orders the reference may produce)
    got = api.fill_bucket_result(np.array([1, 2, 3, 4], np.int32), np.array([5, 9, 5, 5], np.int32), 2, True)
    assert (got.buckets, got.total_buckets, got.total_other_counts) == ([(2, 9), (1, 5)], 4, 10)
    got = api.fill_bucket_result(np.array([1.5, 2.5], np.float32), np.array([4, 4], np.int32), 1, False)
    assert (got.buckets, got.total_buckets, got.total_other_counts) == ([(1.5, 4)], 2, 4)
    assert api.fill_bucket_result(np.zeros(0, np.int32), np.zeros(0, np.int32), 3) == api.BucketResult([], 0, 0)


# ---- refusals that need no device ------------------------------------------------------------------------------------------
def test_null_arguments_are_refused_before_any_device_work(lib):
    q, t, out = _lib.Bm25Query(), _lib.TermsCount(0, 16), _lib.TermCounts()
    assert lib.nrtgpu_count_terms_batch(None, None, None, 0, C.byref(q), C.byref(t), 1, C.byref(out)) == INV
    assert b"NULL" in lib.nrtgpu_last_error()
    assert lib.nrtgpu_count_terms_supported(None, None, 0, C.byref(q), C.byref(t)) == INV
    assert b"NULL" in lib.nrtgpu_last_error()


def test_the_binding_refuses_what_it_can_see(lib):
    class NoSearcher:
        pass

    with pytest.raises(ValueError):
        api._marshal_terms(NoSearcher(), [api.TermQuery(0, 1)], [], 16, None)
    with pytest.raises(ValueError):
        api._marshal_terms(NoSearcher(), [api.TermQuery(0, 1)], [api.TermsCollector(7, 10)], [16, 16], None)
    with pytest.raises(api.UnsupportedQuery):
        api._marshal_terms(NoSearcher(), [api.TermQuery(0, 1)], [api.TermsCollector(7, 10, True, "long")], 16, None)
    c = api.TermsCollector(7, 10)
    assert (c.field, c.size, c.order_desc, c.kind) == (7, 10, True, "int")
    tc = api.TermCounts(np.array([-0.0], np.float32), np.array([3], np.int32), 5, 3, False)
    assert tc.value_bits.tolist() == [0x80000000]


# ---- against the stand-in runtime -------------------------------------------------------------------------------------------
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
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mockhip", "terms_count_host.py")], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "done" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    got = dict(line.split(" ", 1) for line in r.stdout.strip().split("\n") if " " in line)
    I, U = f"{INV} 1", f"{UNS} 1"   # the status (the predicate agreeing), and the reason names the query
    expect = {
        "supported": "0 0", "supported_must": "0 0", "supported_msm2_with_mask": "0 0", "max_buckets_1": "0 0", "max_buckets_65536": "0 0",
        "the_query_has_after": "0 0", "batch_of_4": "4 0", "diagnostics_items": "0 1", "stats_counted": "1",
        "batch_of_256_at_65536": "0 0", "batch_of_257_at_65536": f"{INV}/0 1", "names_the_limit": "1", "batch_above_max_batch": str(INV),
        "max_buckets_0": I, "max_buckets_negative": I, "max_buckets_65537": I, "capacity_below_max_buckets": str(INV), "null_arrays": str(INV),
        "k_zero": I, "k_2000": U, "no_column_on_any_leaf": U, "dismax": U, "dismax_tie_breaker": U, "must_next_to_should": U,
        "min_competitive_score": U, "mask_not_resident": U, "must_not_mask_not_resident": U, "weights_span_too_many_binades": str(UNS),
        "invalid_before_unsupported": I, "invalid_in_query_1_before_unsupported_in_query_0": I,
        "null_queries": str(INV), "null_terms": str(INV), "null_out": str(INV), "null_supported": str(INV),
        "kinds_differ": I, "kinds_differ_text": "1", "flag_no_fixed_point": str(UNS), "flag_packed_postings": str(UNS), "still_answers": "0 0",
    }
    assert got == expect, {k: (got.get(k), v) for k, v in expect.items() if got.get(k) != v}
