"""The numeric range facet without a device: the structs, the reference against a per-doc loop, nrtgpu_range_cuts /
nrtgpu_range_interval (the very functions the host plans with and the kernels compile) against sorted(set(...)) / bisect, the
roll-up identity, NumericRange.bounds over the constructors' edge cases, the condition the fuzz rounds of the device test must
meet, and -- against tests/mockhip -- every refusal that needs a context, the precedence of the statuses and predicate == entry.
Only test_the_reference_agrees_with_a_per_doc_loop and test_every_fuzz_round_holds_the_three_shapes check the reference alone and
pass without the feature."""
import bisect
import ctypes as C
import os
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest

from nrtsearch_amd import _lib, api, build

from tests import _field_sort_ref as fs
from tests import _range_count_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV, UNS = _lib.NRTGPU_ERR_INVALID_ARG, _lib.NRTGPU_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_struct_sizes_and_symbols(lib):
    assert C.sizeof(_lib.ValueRange) == 16 and C.sizeof(_lib.RangeCount) == 16 and C.sizeof(_lib.RangeCounts) == 32
    assert _lib.RangeCount.ranges.offset == 8 and _lib.RangeCounts.capacity.offset == 8 and _lib.RangeCounts.reserved.offset == 12
    assert _lib.RangeCounts.total_hits.offset == 16 and _lib.RangeCounts.hits_with_value.offset == 24
    assert _lib.NRTGPU_MAX_COUNT_RANGES == 64
    for name in ("nrtgpu_count_ranges_batch", "nrtgpu_count_ranges_supported", "nrtgpu_count_docset_ranges_batch",
                 "nrtgpu_count_docset_ranges_supported", "nrtgpu_range_cuts", "nrtgpu_range_interval"):
        assert hasattr(lib, name) and name in _lib.ABI_SYMBOLS


@pytest.mark.parametrize("kind", ref.KINDS)
def test_the_reference_agrees_with_a_per_doc_loop(kind):
    """Checks tests/_range_count_ref.py alone on a 200-doc index: it passes without the feature."""
    corpus = fs.make_corpus([150, 50], {1: 0.6, 2: 0.3}, seed=3, delete_fraction=0.05)
    rng = np.random.default_rng(4)
    pool = np.array(ref.POOL[kind], dtype=ref.BITS_DTYPE[kind])
    d0 = np.nonzero(rng.random(150) < 0.7)[0].astype(np.int32)
    columns = [(d0, rng.choice(pool, size=len(d0))), None]
    hits = ref.text_hits(corpus, (1, 2), 1)
    value = {int(d): int(b) for d, b in zip(*columns[0])}
    for name, ranges in ref.range_lists(kind):
        expect, total, valued = [0] * len(ranges), 0, 0
        for si, seg in enumerate(corpus.segments):
            for d in range(seg.max_doc):
                live = (int(seg.live_bits[d >> 6]) >> (d & 63)) & 1
                if not (live and any(d in seg.postings(t)[0].tolist() for t in (1, 2))):
                    continue
                total += 1
                if si == 0 and d in value:
                    valued += 1
                    o = ref.order_int(kind, value[d])
                    for i, (lo, hi) in enumerate(ranges):
                        expect[i] += ref.order_int(kind, lo) <= o <= ref.order_int(kind, hi)
        assert ref.count(corpus, hits, columns, kind, ranges) == (expect, total, valued), name
        assert 0 < valued < total


def _greatest_key(kind):
    return ref.order_int(kind, ref.GREATEST[kind])


def _draw_ranges(rnd, kind, key):
    """1..64 ranges: overlapping, nested, identical, touching, single-value, empty, at the kind's least and greatest value, NaN and
    +-0.0 for the float kinds, INT64 values that straddle 2^32 and sit at both ends."""
    sp = ref.sorted_pool(kind)
    extra = {"int": [ref.bits_of("int", v) for v in (-2**31 + 1, 2**31 - 2, 6)],
             "float": [ref.bits_of("float", v) for v in (0.5, -7.25)] + ref.NAN_PAYLOADS["float"],
             "long": [ref.bits_of("long", v) for v in (-2**63 + 1, 2**63 - 2, 2**32 - 2, 2**32 + 1, -2**32)],
             "double": [ref.bits_of("double", v) for v in (2.0, -1e300)] + ref.NAN_PAYLOADS["double"]}[kind]
    vals = sp + extra + [ref.LEAST[kind], ref.GREATEST[kind]]
    out = []
    n = rnd.choice([1, 2, 3, 5, 8, 33, 64])
    while len(out) < n:
        a, b = rnd.choice(vals), rnd.choice(vals)
        shape = rnd.random()
        if shape < 0.1 and out:
            out.append(rnd.choice(out))                       # identical
        elif shape < 0.2 and out:
            out.append((out[-1][1], b))                       # touching (possibly empty)
        elif shape < 0.3:
            out.append((a, a))                                # a single value
        elif shape < 0.4:
            out.append((a, ref.GREATEST[kind]))               # the greatest adds no cut
        elif shape < 0.5:
            out.append((ref.LEAST[kind], b))
        elif shape < 0.9:
            out.append((a, b) if key(a) <= key(b) else (b, a))
        else:
            out.append((a, b))                                # as drawn: half of these are empty
    return out[:n], vals


# a code is the order key plus a constant: what include/nrtgpu.h says of the order-preserving codes, restated on integers
CODE_BIAS = {"int": 2**31, "float": 2**31, "long": 2**63, "double": 2**63}


@pytest.mark.parametrize("kind", ref.KINDS)
def test_cuts_and_intervals_against_sorted_sets_and_bisect(lib, kind):
    """3000 seeded range lists per kind, and on EVERY one of them: the cut list equals sorted(set(lo, hi + 1 unless hi is the
    greatest)) over the non-empty ranges, as codes (key + the kind's bias); the interval of each of 500 random values equals
    bisect_right over those cuts; and the roll-up identity holds -- per-range counts rebuilt from the interval counts of the 500
    values equal the direct counts.  The 500 values are drawn from the list's pool of about twenty distinct ones, so the library
    is asked once per distinct value and bound of a list; the order keys are computed once per value."""
    rnd = random.Random(100 + ref.KINDS.index(kind))
    top, bias, kind_id = _greatest_key(kind), CODE_BIAS[kind], api.ALL_DOC_VALUE_KINDS[kind][0]
    key_of = {}

    def key(bits):
        k = key_of.get(bits)
        if k is None:
            k = key_of[bits] = ref.order_int(kind, bits)
        return k

    saw_empty = saw_greatest = saw_64 = saw_nonzero = 0
    out = C.c_int32(0)
    for case in range(3000):
        ranges, vals = _draw_ranges(rnd, kind, key)
        keys = [(key(lo), key(hi)) for lo, hi in ranges]
        expect = set()
        for lo, hi in keys:
            if lo > hi:
                saw_empty += 1
                continue
            expect.add(lo)
            if hi != top:
                expect.add(hi + 1)
            else:
                saw_greatest += 1
        expect = sorted(expect)
        cuts = api.range_cuts(kind, ranges)
        assert len(cuts) <= 128 and cuts == [e + bias for e in expect], (case, ranges)
        saw_64 += len(ranges) == 64
        arr = (C.c_uint64 * max(len(cuts), 1))(*cuts)
        interval_of = {}

        def interval(bits):   # (api.range_interval with the cut array marshalled once per list, asked once per distinct value)
            got = interval_of.get(bits)
            if got is None:
                assert lib.nrtgpu_range_interval(kind_id, arr, len(cuts), C.c_uint64(bits), C.byref(out)) == 0
                got = interval_of[bits] = out.value
            return got

        probe = [rnd.choice(vals) for _ in range(500)]
        assert api.range_interval(kind, cuts, probe[0]) == interval(probe[0])
        iv = [interval(v) for v in probe]
        pk = [key(v) for v in probe]
        assert iv == [bisect.bisect_right(expect, k) for k in pk], (case, ranges)
        per_interval = [0] * (len(cuts) + 1)
        for i in iv:
            per_interval[i] += 1
        pk.sort()
        for (lo_b, hi_b), (lo, hi) in zip(ranges, keys):
            direct = 0 if lo > hi else bisect.bisect_right(pk, hi) - bisect.bisect_left(pk, lo)
            rolled = 0 if lo > hi else sum(per_interval[interval(lo_b): interval(hi_b) + 1])
            assert rolled == direct, (case, lo_b, hi_b)
            saw_nonzero += direct > 0
    # every list went through every check, so these count the checked lists
    assert saw_empty > 1000 and saw_greatest > 1000 and saw_64 > 300 and saw_nonzero > 10000, (saw_empty, saw_greatest, saw_64, saw_nonzero)


def test_cuts_and_intervals_at_the_named_edges(lib):
    i32, i64, f32, f64 = (lambda v: ref.bits_of("int", v)), (lambda v: ref.bits_of("long", v)), (lambda v: ref.bits_of("float", v)), (lambda v: ref.bits_of("double", v))
    # the greatest value adds no cut, the least is a cut: [MIN, MAX] is ONE cut, and every value lies in interval 1
    assert len(api.range_cuts("int", [(i32(-2**31), i32(2**31 - 1))])) == 1 and len(api.range_cuts("long", [(i64(-2**63), i64(2**63 - 1))])) == 1
    assert len(api.range_cuts("float", [(f32(-np.inf), 0x7FC00000)])) == 1 and len(api.range_cuts("double", [(f64(-np.inf), 0xFFF8000000000123)])) == 1
    cuts = api.range_cuts("long", [(i64(2**32), i64(2**32 + 5))])
    assert [api.range_interval("long", cuts, i64(v)) for v in (5, 2**32 - 1, 2**32, 2**32 + 5, 2**32 + 6, 2**33 + 5)] == [0, 0, 1, 1, 2, 2]
    cuts = api.range_cuts("double", [(f64(0.0), f64(1.5))])
    assert [api.range_interval("double", cuts, b) for b in (f64(-0.0), f64(0.0), f64(1.5), f64(1.5) + 1, 0x7FF0000000000001)] == [0, 1, 1, 2, 2]
    cuts = api.range_cuts("float", [(0x7FC00000, 0xFFC12345)])     # [NaN, NaN]: one cut, at the canonical NaN
    assert len(cuts) == 1 and [api.range_interval("float", cuts, b) for b in (f32(np.inf), 0x7FC00001, 0xFFC12345)] == [0, 1, 1]
    assert api.range_cuts("int", [(i32(5), i32(4))]) == [] and api.range_interval("int", [], i32(7)) == 0 and api.range_cuts("int", []) == []
    # identical and touching ranges share cuts
    assert len(api.range_cuts("int", [(i32(1), i32(5)), (i32(1), i32(5)), (i32(5), i32(9)), (i32(6), i32(9))])) == 4
    out, n = (C.c_uint64 * 128)(), C.c_int32(0)
    vr = (_lib.ValueRange * 1)(_lib.ValueRange(3, 2**32 + 1))
    assert lib.nrtgpu_range_cuts(0, vr, 1, out, C.byref(n)) == INV and lib.nrtgpu_range_cuts(2, vr, 1, out, C.byref(n)) == 0
    assert lib.nrtgpu_range_cuts(4, vr, 1, out, C.byref(n)) == INV and lib.nrtgpu_range_cuts(-1, vr, 1, out, C.byref(n)) == INV
    assert lib.nrtgpu_range_cuts(2, vr, 65, out, C.byref(n)) == INV and lib.nrtgpu_range_cuts(2, None, 1, out, C.byref(n)) == INV
    assert lib.nrtgpu_range_cuts(2, vr, 1, None, C.byref(n)) == INV and lib.nrtgpu_range_cuts(2, vr, 1, out, None) == INV
    assert lib.nrtgpu_range_interval(2, out, 129, C.c_uint64(0), C.byref(n)) == INV and lib.nrtgpu_range_interval(2, None, 1, C.c_uint64(0), C.byref(n)) == INV
    assert lib.nrtgpu_range_interval(1, out, 1, C.c_uint64(2**32), C.byref(n)) == INV and lib.nrtgpu_range_interval(2, out, 1, C.c_uint64(0), None) == INV


def test_numeric_range_bounds_restate_the_constructors():
    NR = api.NumericRange
    assert NR("a", 10, True, 25, False).bounds("int") == (10, 24) and NR("a", 10, False, 25, True).bounds("long") == (11, 25)
    assert NR("a", 7, True, 7, True).bounds("long") == (7, 7)
    assert NR("a", -2**63, True, 2**63 - 1, True).bounds("long") == (-2**63, 2**63 - 1)
    assert NR("a", -2**63, True, 2**63 - 1, True).bounds("int") == (-2**31, 2**31 - 1)     # an INT field's longs, cut to int32
    assert NR("a", 2**40, True, 2**41, True).bounds("int") == (1, 0)                       # no int lies in it: the empty range
    for bad in (NR("a", 2**63 - 1, False, 2**63 - 1, True), NR("a", -2**63, True, -2**63, False), NR("a", 5, True, 4, True),
                NR("a", 5, False, 5, True), NR("a", 5, True, 5, False), NR("a", 4, False, 5, False)):
        with pytest.raises(ValueError):
            bad.bounds("long")
    lo, hi = NR("a", 1, False, 2, False).bounds("double")
    assert (lo, hi) == (float(np.nextafter(1.0, np.inf)), float(np.nextafter(2.0, -np.inf)))
    assert NR("a", 2**63 - 1, True, 2**63 - 1, True).bounds("double") == (2.0**63, 2.0**63)     # the int64 widened, as Java does
    assert NR("a", float("-inf"), True, float("inf"), True).bounds("double") == (float("-inf"), float("inf"))
    for bad in (NR("a", float("nan"), True, 1, True), NR("a", 0, True, float("nan"), True), NR("a", 2, True, 1, True), NR("a", 1, False, 1, True)):
        with pytest.raises(ValueError):
            bad.bounds("double")
    lo, hi = NR("a", 1, False, 2, True).bounds("float")
    assert np.float32(lo) == np.nextafter(np.float32(1), np.float32(np.inf)) and hi == 2.0
    with pytest.raises(api.UnsupportedQuery):
        NR("a", 1, True, 2, True).bounds("short")
    # the marshalled bits
    rc, outs, counts, keep = api._marshal_range_counters([api.RangeCounter(7, "long", (NR("a", -5, True, 2**40, False), (9, 3)))])
    assert (rc[0].field_id, rc[0].n_ranges) == (7, 2) and outs[0].capacity >= 2
    assert (rc[0].ranges[0].lower_bits, rc[0].ranges[0].upper_bits) == (2**64 - 5, 2**40 - 1) and (rc[0].ranges[1].lower_bits, rc[0].ranges[1].upper_bits) == (9, 3)
    with pytest.raises(api.UnsupportedQuery):
        api._marshal_range_counters([api.RangeCounter(7, "short", ())])


def test_every_fuzz_round_holds_the_three_shapes():
    """The condition on the device test's fuzz inputs, held by the reference alone: every round contains a range with count 0, a
    range whose count equals hits_with_value (> 0), and two overlapping ranges that are both non-zero -- for both entries."""
    corpus = ref.fuzz_corpus()
    columns = ref.fuzz_columns(corpus)
    for seed in range(ref.FUZZ_ROUNDS):
        calls = ref.fuzz_round(seed)
        assert {e for e, _ in calls} == {"text", "docset"}
        zero = full = overlap = n_ranges = 0
        kinds = set()
        for entry, reqs in calls:
            for req in reqs:
                kind, _, ranges = req
                kinds.add(kind)
                counts, total, valued = ref.fuzz_expect(corpus, columns, entry, req)
                n_ranges += len(ranges)
                zero += any(c == 0 for c in counts)
                full += valued > 0 and any(c == valued for c in counts)
                keys = [(ref.order_int(kind, lo), ref.order_int(kind, hi)) for lo, hi in ranges]
                overlap += any(counts[i] > 0 and counts[j] > 0 and max(keys[i][0], keys[j][0]) <= min(keys[i][1], keys[j][1]) and keys[i] != keys[j]
                               for i in range(len(ranges)) for j in range(i))
        assert zero >= 4 and full >= 4 and overlap >= 4, (seed, zero, full, overlap)
        assert len(kinds) >= 3 and n_ranges > 30, (seed, kinds, n_ranges)


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
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mockhip", "range_count_host.py")], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "done" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    got = dict(line.split(" ", 1) for line in r.stdout.strip().split("\n") if " " in line)
    inv, uns = str(INV), str(UNS)
    expect = {}
    for tag in ("text", "docset"):
        expect.update({
            f"{tag}_runs_64": "0 0", f"{tag}_runs_32": "0 0", f"{tag}_64_ranges": "0 0",
            f"{tag}_n_ranges_0": f"{inv} {inv}", f"{tag}_n_ranges_65": f"{inv} {inv}", f"{tag}_n_ranges_says": "1", f"{tag}_ranges_null": f"{inv} {inv}",
            f"{tag}_high_word_over_32": f"{inv} {inv}", f"{tag}_high_word_over_64_is_a_value": "0 0",
            # what only the entry can judge: its output
            f"{tag}_capacity_short": inv, f"{tag}_counts_null": inv, f"{tag}_reserved_1": inv,
            f"{tag}_num_hits_0": f"{inv} {inv}", f"{tag}_kinds_differ": f"{inv} {inv}",
            f"{tag}_no_column": f"{uns} {uns}", f"{tag}_no_column_says": "1", f"{tag}_multi_column": f"{uns} {uns}", f"{tag}_multi_says": "1",
            f"{tag}_mixed_widths": uns, f"{tag}_mixed_says": "1", f"{tag}_mixed_widths_other_order": uns, f"{tag}_each_width_alone": "0 0 0 0",
            f"{tag}_mask_not_resident": f"{uns} {uns}",
            f"{tag}_invalid_in_query_1_before_unsupported_in_query_0": inv, f"{tag}_high_word_in_query_1_before_multi_in_query_0": inv,
            f"{tag}_invalid_in_query_1_before_mixed_widths": inv, f"{tag}_multi_before_no_mask": f"{uns} {uns}",
        })
    expect.update({
        "text_dismax": f"{uns} {uns}", "text_must_next_to_should": f"{uns} {uns}", "text_min_competitive": f"{uns} {uns}",
        "text_num_hits_2000": f"{uns} {uns}", "text_has_after_is_not_read": "0 0",
        "docset_k_0": f"{inv} {inv}", "docset_range_32_beside_a_64_count": "0 0", "docset_range_over_a_64_bit_column": f"{uns} {uns}",
        "null_arguments": " ".join([inv] * 7),
        # the text entry refuses both flags, an invalid argument first; the doc-set entry runs under both, at either width
        "text_no_fixed_point": f"{uns} {uns}", "text_no_fixed_point_says": "1", "text_no_fixed_point_invalid_first": f"{inv} {inv}",
        "text_packed_postings": f"{uns} {uns}", "text_packed_postings_says": "1", "text_packed_postings_invalid_first": f"{inv} {inv}",
        "docset_no_fixed_point": "0 0 0 0", "docset_packed_postings": "0 0 0 0",
    })
    assert got == expect, {k: (got.get(k), v) for k, v in expect.items() if got.get(k) != v} | {k: got[k] for k in got if k not in expect}
