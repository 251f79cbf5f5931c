"""The terms aggregation over 64-bit columns (nrtgpu_count_terms64_batch, nrtgpu_count_docset_terms64_batch) where no device is
needed: the layout of the output struct and the exported symbols, tests/_terms_count64_ref.py against a per-doc loop,
nrtgpu_terms_home_slots64 -- its refusals, its ranges and how the hash spreads values that differ in one half only -- and the
condition every round of the device fuzz (tests/test_terms_count64_gpu.py) must meet, checked on the reference alone.  No context is
created here: every refusal that needs one is checked in the GPU file."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest

from nrtsearch_amd import _lib, api, build

from tests import _field_sort64_ref as f64
from tests import _field_sort_ref as fs
from tests import _terms_count64_cases as cases
from tests import _terms_count64_ref as ref

FUZZ_BASE, FUZZ_ROUNDS = 9100, 20   # (tests/test_terms_count64_gpu.py runs the same rounds)
NEW_SYMBOLS = ("nrtgpu_count_terms64_batch", "nrtgpu_count_terms64_supported", "nrtgpu_count_docset_terms64_batch",
               "nrtgpu_count_docset_terms64_supported", "nrtgpu_terms_home_slots64")


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_the_output_struct_and_the_symbols(lib):
    t = _lib.TermCounts64
    assert C.sizeof(t) == 48
    assert [(n, getattr(t, n).offset) for n, _ in t._fields_] == [("n_buckets", 0), ("capacity", 4), ("value_bits", 8), ("counts", 16), ("total_hits", 24),
                                                                 ("hits_with_value", 32), ("overflowed", 40), ("reserved", 44)]
    assert t.value_bits.size == 8 and C.sizeof(C.c_uint64) == 8
    for name in NEW_SYMBOLS:
        assert name in _lib.ABI_SYMBOLS and hasattr(lib, name), name
    assert _lib.NRTGPU_TERMS64_LDS_SLOTS == 8192 and _lib.NRTGPU_TERMS64_MAX_CALL_SLOTS == 2**28 // 12
    for name in ("count_terms64_batch", "count_terms64_supported", "count_docset_terms64_batch", "count_docset_terms64_supported", "terms_home_slots64",
                 "TermCounts64"):
        assert hasattr(api, name), name


@pytest.mark.parametrize("kind", ["long", "double"])
def test_the_reference_agrees_with_a_per_doc_loop(kind):
    """(This one passes without the feature: it checks the reference, not the library.)  200 docs in two leaves with deletes, a third
    leaf without the column, docs without a value."""
    corpus = fs.make_corpus([120, 80, 30], {1: 0.6, 2: 0.4}, seed=3, delete_fraction=0.1)
    rng = np.random.default_rng(4)
    pool = cases.POOLS[(kind, "edge")]
    d0 = np.nonzero(rng.random(120) < 0.7)[0].astype(np.int32)
    columns = [(d0, rng.choice(pool, size=len(d0))), (None, rng.choice(pool, size=80)), None]
    for clauses, need in (((1,), 1), ((1, 2), 2), ((1, 2), 1)):
        hits = ref.text_hits(corpus, clauses, need)
        table, total = {}, 0
        for si, seg in enumerate(corpus.segments):
            ok = fs._bits(hits[si], seg.max_doc)
            value = {}
            if columns[si] is not None:
                docs = range(seg.max_doc) if columns[si][0] is None else columns[si][0].tolist()
                value = dict(zip(docs, columns[si][1].tolist()))
            for d in range(seg.max_doc):
                if not ok[d]:
                    continue
                total += 1
                if d in value:
                    b = value[d]
                    if kind == "double" and (b & (2**63 - 1)) > 0x7FF0000000000000:
                        b = f64.CANONICAL_NAN
                    table[b] = table.get(b, 0) + 1
        keys = sorted(table, key=lambda b: f64.order_int(kind, b))
        bits, counts, n, tot, with_value, overflowed = ref.count(corpus, hits, columns, kind)
        assert (bits.tolist(), counts.tolist(), n, tot, with_value, overflowed) == (keys, [table[b] for b in keys], len(keys), total, sum(table.values()), 0)
        assert n >= 2 and total > with_value > 0
        assert ref.unvalued_hits(corpus, hits, columns) == total - with_value
        over = ref.count(corpus, hits, columns, kind, n - 1)
        assert (len(over[0]), len(over[1]), over[2], over[3], over[4], over[5]) == (0, 0, 0, total, -1, 1)
        assert ref.count(corpus, hits, columns, kind, n)[5] == 0
    if kind == "double":   # the zeros are two buckets, the NaNs one, last
        bits = ref.count(corpus, ref.text_hits(corpus, (1, 2), 1), columns, kind)[0].tolist()
        assert bits[-1] == f64.CANONICAL_NAN and bits.count(f64.CANONICAL_NAN) == 1 and bits.index(0x8000000000000000) + 1 == bits.index(0)


def test_home_slots_refusals_and_ranges(lib):
    lds, tab = C.c_uint32(7), C.c_uint32(7)
    inv = _lib.NRTGPU_ERR_INVALID_ARG
    for kind in (-1, 0, 1, 4):
        assert lib.nrtgpu_terms_home_slots64(kind, 5, 16, C.byref(lds), C.byref(tab)) == inv and b"kind" in lib.nrtgpu_last_error()
    for b in (0, -1, 65537):
        assert lib.nrtgpu_terms_home_slots64(2, 5, b, C.byref(lds), C.byref(tab)) == inv and b"max_buckets" in lib.nrtgpu_last_error()
    assert lib.nrtgpu_terms_home_slots64(2, 5, 16, None, C.byref(tab)) == inv
    assert lib.nrtgpu_terms_home_slots64(3, 5, 16, C.byref(lds), None) == inv
    with pytest.raises(KeyError):
        api.terms_home_slots64("int", 5, 16)
    rng = np.random.default_rng(6)
    values = np.concatenate([rng.integers(0, 2**64, size=300, dtype=np.uint64), cases.LONG_EDGE, cases.POOLS[("double", "edge")]])
    for b in (1, 2, 3, 4, 5, 8, 9, 1000, 4096, 4097, 65535, 65536):
        slots = 2
        while slots < 2 * b:
            slots *= 2
        for kind in ("long", "double"):
            for v in values[:: 7 if b > 9 else 1].tolist():
                l, t = api.terms_home_slots64(kind, v, b)
                assert 0 <= l < _lib.NRTGPU_TERMS64_LDS_SLOTS and 0 <= t < slots, (kind, v, b, l, t)
    # every NaN is one value; the zeros are two
    assert len({api.terms_home_slots64("double", v, 4096) for v in cases.NANS}) == 1
    assert api.terms_home_slots64("double", 0, 4096) != api.terms_home_slots64("double", 0x8000000000000000, 4096)


def test_the_hash_reads_both_halves_of_a_value():
    """4096 longs that agree in their low 32 bits, and 4096 that agree in their high word: the distinct home slots in the workgroup's
    table are at least half of what a uniform draw gives, m (1 - (1 - 1/m)^n).  A hash that reads half of the code yields one slot."""
    m, n = _lib.NRTGPU_TERMS64_LDS_SLOTS, 4096
    uniform = m * (1.0 - (1.0 - 1.0 / m) ** n)
    for name, values in (("high halves differ", [(j << 32) + 5 for j in range(n)]), ("low halves differ", [(5 << 32) + j for j in range(n)])):
        for max_buckets, slots in ((4096, 8192), (65536, 131072)):
            lds = {api.terms_home_slots64("long", v, max_buckets)[0] for v in values}
            tab = {api.terms_home_slots64("long", v, max_buckets)[1] for v in values}
            assert len(lds) >= uniform / 2, f"{name}: {len(lds)} distinct LDS home slots, a uniform draw gives {uniform:.0f}"
            assert len(tab) >= slots * (1.0 - (1.0 - 1.0 / slots) ** n) / 2, f"{name}: {len(tab)} distinct home slots in a table of {slots}"
    assert math.isclose(uniform, 3223.45, abs_tol=0.01)


def test_index_a_is_what_the_device_tests_assume():
    ix = cases.index_a()
    assert ix.sizes == [2500, 700, 300] and all(seg.live_bits is not None for seg in ix.corpus.segments)
    for key, cols in ix.columns.items():
        assert cols[0][0] is None and cols[1][0] is not None and 0.7 < len(cols[1][0]) / 700 < 0.9 and cols[2] is None
    every = cases.Req(("long", "many"), 65536, docset=True)
    assert ix.distinct(every) > 600 and ix.distinct(dataclasses.replace(every, column=("double", "many"))) > 600
    assert ix.expected(dataclasses.replace(every, column=("long", "edge")))[0].tolist() == cases.LONG_EDGE.tolist()
    assert ix.expected(dataclasses.replace(every, column=("double", "edge")))[0].tolist() == cases.DOUBLE_EDGE.tolist() + [f64.CANONICAL_NAN]
    assert ix.unvalued(every) > 300


@pytest.mark.parametrize("round_", range(FUZZ_ROUNDS))
def test_every_fuzz_round_holds_its_condition(round_):
    """Over the 20 seeds every round holds at least one overflowed query, one exact query with >= 2 buckets, and one hit without a
    value; and both forms and both kinds."""
    ix, batches = cases.fuzz_round(FUZZ_BASE, round_)
    assert 1 <= len(ix.sizes) <= 3 and all(1 <= n <= 3000 for n in ix.sizes)
    reqs = [r for b in batches for r in b]
    assert all(1 <= len(b) <= 16 for b in batches)
    exp = [ix.expected(r) for r in reqs]
    assert any(e[5] == 1 for e in exp), "no overflowed query"
    assert any(e[5] == 0 and e[2] >= 2 for e in exp), "no exact query with two buckets"
    assert any(ix.unvalued(r) > 0 for r in reqs), "no hit without a value"
    assert {r.docset for r in reqs} == {False, True} and {r.column[0] for r in reqs} == {"long", "double"}
