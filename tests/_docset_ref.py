"""A NumPy reference of the doc-set requests (nrtgpu_search_docset_sorted_batch, nrtgpu_count_docset_terms_batch), independent of
the library's coding of the values.

  hit set   liveDocs AND every filter mask AND no must_not mask AND every range clause.  A range clause keeps a doc iff the doc
            HAS a value in the clause's column and lower <= value <= upper, with Integer.compare / Float.compare WRITTEN OUT on
            numpy integers (_field_sort_ref.order_key: -0.0 < +0.0, every NaN equal and above +inf); a doc without a value, or in
            a leaf without the column, fails; lower > upper keeps nothing
  then      tests/_field_sort_ref.py's ordering, paging and relation, and tests/_terms_count_ref.py's counting, over that set:
            both take the set as their `accept` words, under a clause that every doc matches (term ALL of the corpora here)

Columns are the other references' (per leaf None, or (docs or None = every doc, value bits uint32))."""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from tests import _field_sort_ref as fs
from tests import _terms_count_ref as tcr

ALL = 1   # the term the corpora of these tests index in every doc (density 1.0)


def pack(ok: np.ndarray) -> np.ndarray:
    """bool[max_doc] -> uint64 words"""
    padded = np.zeros(((len(ok) + 63) // 64) * 64, dtype=bool)
    padded[: len(ok)] = ok
    return np.packbits(padded.reshape(-1, 64), axis=1, bitorder="little").view(np.uint64).reshape(-1)


def range_keeps(kind: str, lower_bits: int, upper_bits: int, value_bits) -> np.ndarray:
    """The range rule on values that exist: lower <= value <= upper in the kind's order."""
    v = fs.order_key(kind, value_bits)
    lo, hi = int(fs.order_key(kind, [lower_bits])[0]), int(fs.order_key(kind, [upper_bits])[0])
    return (v >= lo) & (v <= hi)


def hit_set(corpus, filters: Sequence[Sequence[np.ndarray]] = (), must_nots: Sequence[Sequence[np.ndarray]] = (),
            ranges: Sequence[Tuple[str, Sequence, int, int]] = (), live=None):
    """-> per leaf the hit set as uint64 words.  filters / must_nots: per mask its words per leaf; ranges: (kind, columns per leaf,
    lower bits, upper bits); live[leaf]: other liveDocs words replacing the leaf's."""
    out = []
    for si, seg in enumerate(corpus.segments):
        ok = np.ones(seg.max_doc, dtype=bool)
        lv = live[si] if live is not None and live[si] is not None else seg.live_bits
        if lv is not None:
            ok &= fs._bits(lv, seg.max_doc)
        for m in filters:
            ok &= fs._bits(m[si], seg.max_doc)
        for m in must_nots:
            ok &= ~fs._bits(m[si], seg.max_doc)
        for kind, columns, lo, hi in ranges:
            keep = np.zeros(seg.max_doc, dtype=bool)
            if columns[si] is not None:
                cd, cv = columns[si]
                idx = np.arange(seg.max_doc) if cd is None else np.asarray(cd)
                keep[idx] = range_keeps(kind, lo, hi, np.asarray(cv, dtype=np.uint32))
            ok &= keep
        out.append(pack(ok))
    return out


def search(corpus, hits, columns, kind: str, k: int, reverse: bool = False, missing_bits: int = 0, **kw):
    """_field_sort_ref.search over the hit set -> (docs, value_bits, total_hits, relation_gte)"""
    return fs.search(corpus, columns, kind, (ALL,), k, reverse, missing_bits, 1, accept=hits, **kw)


def count(corpus, hits, columns, kind: str, max_buckets: int = 65536):
    """_terms_count_ref.count over the hit set -> (value_bits, counts, n_buckets, total_hits, hits_with_value, overflowed)"""
    return tcr.count(corpus, columns, kind, (ALL,), 1, max_buckets, accept=hits)
