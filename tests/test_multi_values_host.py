"""Multi-valued doc value columns, the part that needs no device and no context: the NumPy reference of the GPU tests
(tests/_multi_values_ref.py) against a brute-force dict / loop, and the new entry's refusal of a NULL segment.

test_the_reference_equals_a_brute_force_loop checks the REFERENCE alone: it reads nothing of the library and passes without the
feature.  test_the_entry_refuses_a_null_segment needs the symbol and fails without it.  No public struct changed."""
import struct

import numpy as np
import pytest

from nrtsearch_amd import _lib, build

from tests import _docset_ref as dsr
from tests import _field_sort_ref as fs
from tests import _multi_values_ref as mref

NAN_PAYLOADS = [0x7FC00000, 0x7FC00001, 0xFFC12345]
POOL = {"int": np.array([fs.INT32_MIN, -1, 0, 1, 7, fs.INT32_MAX], dtype=np.int32).view(np.uint32),
        "float": np.concatenate([np.array([-np.inf, -1.5, -0.0, 0.0, 1e-45, 3.25, np.inf], dtype=np.float32).view(np.uint32),
                                 np.array(NAN_PAYLOADS, dtype=np.uint32)])}


def _value(kind, bits):
    """The Java value of the bits as a sortable Python key: ints by value; floats by Float.compare (NaN above +inf, -0.0 < +0.0)."""
    if kind == "int":
        return bits - 2**32 if bits >= 2**31 else bits
    f = struct.unpack("<f", struct.pack("<I", bits))[0]
    if f != f:
        return (2, 0.0, 0)
    return (1, f, 0 if bits >> 31 else 1) if f == 0.0 else (1, f, 0)


def _column(rng, n_docs, pool):
    per_doc = rng.integers(0, 4, size=n_docs)
    per_doc[17] = 70
    docs = np.repeat(np.arange(n_docs, dtype=np.int32), per_doc)
    vals = rng.choice(pool, size=len(docs)).astype(np.uint32)
    at = int(np.searchsorted(docs, 5))
    if per_doc[5] == 3:
        vals[at: at + 3] = pool[0]   # the same value three times in one doc
    return docs, vals


@pytest.mark.parametrize("kind", ["int", "float"])
def test_the_reference_equals_a_brute_force_loop(kind):
    corpus = fs.make_corpus([150, 50], {1: 1.0, 2: 0.4}, seed=12, delete_fraction=0.05)
    rng = np.random.default_rng(3)
    columns = [_column(rng, 150, POOL[kind]), None]
    hits = mref.text_hits(corpus, (2,), 1)
    # ---- counting: a dict over the value instances of the live docs that hold term 2
    table, total = {}, 0
    for si, seg in enumerate(corpus.segments):
        live = fs._bits(seg.live_bits, seg.max_doc)
        matched = set(seg.postings(2)[0].tolist())
        for d in range(seg.max_doc):
            if not live[d] or d not in matched:
                continue
            total += 1
            if columns[si] is None:
                continue
            for vd, vb in zip(*columns[si]):
                if int(vd) == d:
                    b = int(vb)
                    if kind == "float" and (b & 0x7FFFFFFF) > 0x7F800000:
                        b = 0x7FC00000
                    table[b] = table.get(b, 0) + 1
    order = sorted(table, key=lambda b: _value(kind, b))
    bits, counts, n, tot, valued, over = mref.count(corpus, hits, columns, kind)
    assert (bits.tolist(), counts.tolist(), n, tot, valued, over) == (order, [table[b] for b in order], len(order), total, sum(table.values()), 0)
    assert valued > tot > 0 and n == (6 if kind == "int" else 8)   # more instances than hits; the three NaN payloads are one bucket
    assert mref.count(corpus, hits, columns, kind, n - 1)[2:] == (0, total, -1, 1) and mref.count(corpus, hits, columns, kind, n)[5] == 0
    # ---- "any value in range": a loop over every doc's values
    for lo, hi in [(lo, hi) for lo in POOL[kind] for hi in POOL[kind]]:
        exp = []
        for si, seg in enumerate(corpus.segments):
            keep = np.zeros(seg.max_doc, dtype=bool)
            if columns[si] is not None:
                for vd, vb in zip(*columns[si]):
                    if _value(kind, int(lo)) <= _value(kind, int(vb)) <= _value(kind, int(hi)):
                        keep[int(vd)] = True
            exp.append(dsr.pack(keep))
        got = mref.any_in_range(corpus, kind, columns, int(lo), int(hi))
        assert all(np.array_equal(g, e) for g, e in zip(got, exp)), (lo, hi)
        assert not got[1].any()   # the leaf without the column keeps nothing


def test_the_entry_refuses_a_null_segment():
    build.build()
    lib = _lib.load()
    assert "nrtgpu_segment_add_doc_values_multi" in _lib.ABI_SYMBOLS
    docs, vals = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.uint32)
    assert lib.nrtgpu_segment_add_doc_values_multi(None, 7, _lib.NRTGPU_DOCVALUES_INT32, 1, docs.ctypes.data, vals.ctypes.data) == _lib.NRTGPU_ERR_INVALID_ARG
    assert lib.nrtgpu_segment_add_doc_values_multi(None, 7, _lib.NRTGPU_DOCVALUES_INT32, 0, None, None) == _lib.NRTGPU_ERR_INVALID_ARG
