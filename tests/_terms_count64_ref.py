"""A NumPy reference of the terms aggregation over ONE 64-bit doc value column (nrtgpu_count_terms64_batch,
nrtgpu_count_docset_terms64_batch: LONG / DATE_TIME as int64, DOUBLE as float64), independent of the library's coding of the values
and of its count tables.

  hits      per leaf uint64 words: a text query's (text_hits: tests/_field_sort_ref.py's matching -- all clauses SHOULD: docs matched
            by at least max(1, min_should_match) clauses, all clauses MUST: by all of them, inside the accept set) or a doc set's
            (tests/_docset_ref.py: hit_set -- liveDocs AND every filter AND no must_not AND every 32-bit range clause)
  buckets   numpy.unique over the uint64 value bits of the hits that HAVE a value, every NaN first made 0x7FF8000000000000 (doubles
            are bucketed by Double.doubleToLongBits: -0.0 and +0.0 are two buckets); a hit without a value, or in a leaf without
            the column, adds to no bucket but counts in total_hits
  order     ascending Long.compare / Double.compare, written out on integers (tests/_field_sort64_ref.py: order_key)
  overflow  more than max_buckets distinct values: no buckets, hits_with_value -1, total_hits exact (tests/_terms_count_ref.py: count)
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np

from tests import _field_sort64_ref as f64
from tests import _field_sort_ref as fs
from tests import _multi_values_ref as mref

text_hits = mref.text_hits   # (corpus, term_ids, need, accept=, live=) -> per leaf uint64 words


def count(corpus, hits, columns: Sequence[Optional[Tuple[Optional[np.ndarray], np.ndarray]]], kind: str, max_buckets: int = 65536):
    """-> (value_bits uint64 ascending in the kind's order, counts int32, n_buckets, total_hits, hits_with_value, overflowed).
    hits[leaf]: uint64 words; columns[leaf]: None (the leaf lacks the column) or (docs or None = every doc, value bits uint64)."""
    total, valued = 0, []
    for si, seg in enumerate(corpus.segments):
        ok = fs._bits(hits[si], seg.max_doc)
        total += int(ok.sum())
        if columns[si] is None:
            continue
        cd, cv = columns[si]
        has = np.zeros(seg.max_doc, dtype=bool)
        vals = np.zeros(seg.max_doc, dtype=np.uint64)
        idx = np.arange(seg.max_doc) if cd is None else np.asarray(cd)
        has[idx] = True
        vals[idx] = np.asarray(cv, dtype=np.uint64)
        valued.append(vals[ok & has])
    bits = f64.canonical_bits(kind, np.concatenate(valued) if valued else np.zeros(0, np.uint64))
    ub, uc = np.unique(bits, return_counts=True)
    if len(ub) > int(max_buckets):
        return np.zeros(0, np.uint64), np.zeros(0, np.int32), 0, total, -1, 1
    order = np.argsort(f64.order_key(kind, ub), kind="stable")
    return ub[order].astype(np.uint64), uc[order].astype(np.int32), int(len(ub)), total, int(uc.sum()), 0


def distinct(corpus, hits, columns, kind: str) -> int:
    """the distinct values among the valued hits"""
    return count(corpus, hits, columns, kind)[2]


def unvalued_hits(corpus, hits, columns) -> int:
    """the hits without a value (a doc that lacks one, a leaf that lacks the column)"""
    n = 0
    for si, seg in enumerate(corpus.segments):
        ok = fs._bits(hits[si], seg.max_doc)
        if columns[si] is None:
            n += int(ok.sum())
        elif columns[si][0] is not None:
            has = np.zeros(seg.max_doc, dtype=bool)
            has[np.asarray(columns[si][0])] = True
            n += int((ok & ~has).sum())
    return n
