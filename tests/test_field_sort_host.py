"""Sort by field, the part that needs no context: the structs' sizes, the key coding the kernel compiles
(nrtgpu_sort_value_code) over the edge values of both kinds, the NumPy reference of the GPU tests (tests/_field_sort_ref.py)
against a brute-force Python sorted(), and the refusals that are decided before any device is touched."""
import ctypes as C
import functools
import math
import struct

import numpy as np
import pytest

from nrtsearch_amd import _lib, api, build

from tests import _field_sort_ref as ref


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_struct_sizes(lib):
    assert C.sizeof(_lib.FieldSort) == 24
    assert C.sizeof(_lib.FieldDocs) == C.sizeof(_lib.TopDocs) == 40
    for name in ("n_hits", "capacity", "docs", "total_hits", "total_hits_is_lower_bound"):
        assert getattr(_lib.FieldDocs, name).offset == getattr(_lib.TopDocs, name).offset
    assert _lib.FieldDocs.value_bits.offset == _lib.TopDocs.scores.offset
    assert _lib.FieldSort.after_bits.offset == 20 and _lib.FieldSort.missing_bits.offset == 8


def _decode(kind, reverse, high):
    """The value bits a key's high word stands for, written out independently of the library."""
    code = high if reverse else (~high) & 0xFFFFFFFF
    if kind == "int":
        return code ^ 0x80000000
    return code & 0x7FFFFFFF if code & 0x80000000 else (~code) & 0xFFFFFFFF


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("reverse", [False, True])
def test_the_code_is_strictly_monotone_and_decodes(lib, kind, reverse):
    bits = ref.VALUES[kind].tolist()   # ascending in the kind's order
    highs = [api.sort_value_code(kind, reverse, b) for b in bits]
    for a, b in zip(highs, highs[1:]):
        # a larger key ranks earlier: ascending sorts want the smaller value's key larger, descending the larger value's
        assert (a < b) if reverse else (a > b), (kind, reverse, highs)
    for b, h in zip(bits, highs):
        assert _decode(kind, reverse, h) == b, (kind, reverse, hex(b), hex(h))
    # with the docid in the low word no key is 0
    assert all(((h << 32) | (0xFFFFFFFF - d)) != 0 for h in highs for d in (0, 2**31 - 1))


@pytest.mark.parametrize("reverse", [False, True])
def test_every_nan_is_the_canonical_one_and_the_largest(lib, reverse):
    canonical = api.sort_value_code("float", reverse, 0x7FC00000)
    for payload in (0x7FC00001, 0x7F800001, 0x7FFFFFFF, 0xFFC00000, 0xFF800001, 0xFFFFFFFF):
        assert api.sort_value_code("float", reverse, payload) == canonical, hex(payload)
    inf = api.sort_value_code("float", reverse, ref.bits_of("float", math.inf))
    assert (canonical > inf) if reverse else (canonical < inf)
    assert _decode("float", reverse, canonical) == 0x7FC00000


def test_the_code_orders_random_values_like_the_reference_order(lib):
    rng = np.random.default_rng(3)
    for kind in ("int", "float"):
        bits = np.concatenate([rng.integers(0, 2**32, size=500, dtype=np.uint64).astype(np.uint32), ref.VALUES[kind]])
        keys = ref.order_key(kind, bits)
        asc = np.array([api.sort_value_code(kind, False, int(b)) for b in bits], dtype=np.int64)
        desc = np.array([api.sort_value_code(kind, True, int(b)) for b in bits], dtype=np.int64)
        o = np.argsort(keys, kind="stable")
        assert np.all(np.diff(desc[o]) >= 0) and np.all(np.diff(asc[o]) <= 0)
        assert np.array_equal(np.diff(desc[o]) == 0, np.diff(keys[o]) == 0)   # equal codes exactly where the values are equal


def _float_compare(a_bits, b_bits):
    """Float.compare on raw bits, the long way."""
    a, b = struct.unpack("<f", struct.pack("<I", a_bits))[0], struct.unpack("<f", struct.pack("<I", b_bits))[0]
    if a < b:
        return -1
    if a > b:
        return 1
    # equal, or a NaN: Float.compare orders floatToIntBits (every NaN collapsed to 0x7fc00000) as ints
    ia = 0x7FC00000 if a != a else a_bits
    ib = 0x7FC00000 if b != b else b_bits
    ia = ia - 2**32 if ia >= 2**31 else ia
    ib = ib - 2**32 if ib >= 2**31 else ib
    return (ia > ib) - (ia < ib)


def _int_compare(a_bits, b_bits):
    a = a_bits - 2**32 if a_bits >= 2**31 else a_bits
    b = b_bits - 2**32 if b_bits >= 2**31 else b_bits
    return (a > b) - (a < b)


@pytest.fixture(scope="module")
def small():
    """200 docs in leaves of 130, 50 and 20; the column on 80 % of leaf 0, all of leaf 1, absent from leaf 2."""
    corpus = ref.make_corpus([130, 50, 20], {1: 0.6, 2: 0.4, 3: 0.3}, seed=11, delete_fraction=0.05)
    rng = np.random.default_rng(12)
    cols = {}
    for kind in ("int", "float"):
        d0 = np.nonzero(rng.random(130) < 0.8)[0].astype(np.int32)
        cols[kind] = [(d0, rng.choice(ref.VALUES[kind], size=len(d0))), (None, rng.choice(ref.VALUES[kind], size=50)), None]
    return corpus, cols


def _brute(corpus, columns, kind, terms, need, k, reverse, missing_bits, after, must_all=False):
    cmp_v = _int_compare if kind == "int" else _float_compare
    hits = []
    for si, seg in enumerate(corpus.segments):
        col = {}
        if columns[si] is not None:
            cd, cv = columns[si]
            col = {int(d): int(v) for d, v in zip(range(seg.max_doc) if cd is None else cd.tolist(), np.asarray(cv).tolist())}
        holds = {t: set(seg.postings(t)[0].tolist()) for t in set(terms)}
        for doc in range(seg.max_doc):
            if seg.live_bits is not None and not (int(seg.live_bits[doc >> 6]) >> (doc & 63)) & 1:
                continue
            n = sum(1 for t in terms if doc in holds[t])
            if n < max(need, 1):
                continue
            hits.append((col.get(doc, missing_bits), seg.doc_base + doc))

    def cmp(x, y):
        c = cmp_v(x[0], y[0])
        c = -c if reverse else c
        return c if c else (x[1] > y[1]) - (x[1] < y[1])

    ordered = sorted(hits, key=functools.cmp_to_key(cmp))
    total = len(ordered)
    if after is not None:
        ordered = [h for h in ordered if cmp(h, (after[1], after[0])) > 0]
    return ordered[:k], total


@pytest.mark.parametrize("kind", ["int", "float"])
def test_the_reference_agrees_with_a_brute_force_sort(lib, small, kind):
    corpus, cols = small
    columns = cols[kind]
    checked = 0
    for terms, need in (((1,), 1), ((1, 2, 3), 1), ((1, 2, 3), 2), ((1, 2), 2), ((2, 2, 3), 2), ((99,), 1)):
        for reverse in (False, True):
            for missing in (ref.KIND_MIN[kind], ref.KIND_MAX[kind], int(ref.VALUES[kind][2])):
                for k in (1, 7, 300):
                    exp, total = _brute(corpus, columns, kind, terms, need, k, reverse, missing, None)
                    docs, bits, tot, gte = ref.search(corpus, columns, kind, terms, k, reverse, missing, need)
                    assert docs.tolist() == [d for _, d in exp] and tot == total and not gte
                    assert bits.tolist() == ref.canonical_bits(kind, [v for v, _ in exp]).tolist()
                    checked += 1
                # pages of 7 behind the cursor
                page1, _ = _brute(corpus, columns, kind, terms, need, 7, reverse, missing, None)
                if len(page1) == 7:
                    after = (page1[-1][1], page1[-1][0])
                    exp, total = _brute(corpus, columns, kind, terms, need, 7, reverse, missing, after)
                    docs, bits, tot, _ = ref.search(corpus, columns, kind, terms, 7, reverse, missing, need, after=after)
                    assert docs.tolist() == [d for _, d in exp] and tot == total
    assert checked >= 100


def test_the_reference_relation_follows_the_slices(lib, small):
    corpus, cols = small
    info = {}
    # one slice per leaf: leaf 0 alone passes max(threshold 20, k 10)
    docs, _, total, gte = ref.search(corpus, cols["int"], "int", (1,), 10, total_hits_threshold=20, slicing=(100, 1, 1), info=info)
    assert len(info["slice_hits"]) == 3 and max(info["slice_hits"]) > 20 and gte and total == sum(info["slice_hits"])
    assert not ref.search(corpus, cols["int"], "int", (1,), 10, total_hits_threshold=max(info["slice_hits"]), slicing=(100, 1, 1))[3]
    # k hits must have been returned: a page of 300 is not full
    assert not ref.search(corpus, cols["int"], "int", (1,), 300, total_hits_threshold=20, slicing=(100, 1, 1))[3]


# ---- refusals that need no device ----------------------------------------------------------------------------------------
def test_sort_value_code_refusals(lib):
    out = C.c_uint32(0)
    for kind, reverse in ((2, 0), (-1, 0), (0, 2), (1, -1)):
        assert lib.nrtgpu_sort_value_code(kind, reverse, 0, C.byref(out)) == _lib.NRTGPU_ERR_INVALID_ARG
        assert len(lib.nrtgpu_last_error()) > 10
    assert lib.nrtgpu_sort_value_code(0, 0, 0, None) == _lib.NRTGPU_ERR_INVALID_ARG
    assert lib.nrtgpu_sort_value_code(1, 1, 0, C.byref(out)) == _lib.NRTGPU_OK


def test_null_arguments_are_refused_before_any_device_work(lib):
    v = np.zeros(4, dtype=np.int32)
    assert lib.nrtgpu_segment_add_doc_values(None, 0, 0, 4, None, v.ctypes.data) == _lib.NRTGPU_ERR_INVALID_ARG
    q, s, out = _lib.Bm25Query(), _lib.FieldSort(), _lib.FieldDocs()
    assert lib.nrtgpu_search_sorted_batch(None, None, None, 0, C.byref(q), C.byref(s), 1, C.byref(out)) == _lib.NRTGPU_ERR_INVALID_ARG
    assert lib.nrtgpu_sorted_supported(None, None, 0, C.byref(q), C.byref(s)) == _lib.NRTGPU_ERR_INVALID_ARG
    assert b"NULL" in lib.nrtgpu_last_error()


def test_the_binding_refuses_what_it_can_see(lib):
    seg = api.GpuSegment.__new__(api.GpuSegment)   # (no context: the checks below come before the library is called)
    seg._h = None
    with pytest.raises(TypeError):
        seg.add_doc_values(7, "int", np.zeros(4, dtype=np.float32))
    with pytest.raises(TypeError):
        seg.add_doc_values(7, "float", np.zeros(4, dtype=np.float64))
    with pytest.raises(ValueError):
        seg.add_doc_values(7, "int", np.zeros(4, dtype=np.int32), np.arange(3))
    with pytest.raises(KeyError):
        seg.add_doc_values(7, "long", np.zeros(4, dtype=np.int64))
    assert api._value_bits("float", -0.0) == 0x80000000 and api._value_bits("int", -1) == 0xFFFFFFFF
    assert api.TopFieldDocs(np.zeros(1, np.int32), np.array([-0.0], np.float32), 1, False).value_bits.tolist() == [0x80000000]
