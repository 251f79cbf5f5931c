"""A NumPy reference of the terms aggregation (nrtgpu_count_terms_batch): a query's hits counted per distinct value of ONE int or
float doc value column, independent of the library's coding of the values.

  hits      tests/_field_sort_ref.py's matching: all clauses SHOULD: docs matched by at least max(1, min_should_match) clauses
            (duplicate clauses count each); all clauses MUST: by all of them; inside the accept set
  buckets   numpy.unique over the value bits of the hits that HAVE a value, every NaN first made 0x7FC00000 (floats are bucketed
            by Float.floatToIntBits: -0.0 and +0.0 are two buckets); a hit without a value, or in a leaf without the column, adds
            to no bucket but counts in total_hits
  order     ascending Integer.compare / Float.compare, written out on integers (_field_sort_ref.order_key)
  overflow  more than max_buckets distinct values: no buckets, hits_with_value -1, total_hits exact
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np

from tests import _field_sort_ref as fs


def count(corpus, columns: Sequence[Optional[Tuple[Optional[np.ndarray], np.ndarray]]], kind: str, term_ids: Sequence[int], need: int = 1,
          max_buckets: int = 65536, accept=None, live=None):
    """-> (value_bits uint32 ascending in the kind's order, counts int32, n_buckets, total_hits, hits_with_value, overflowed).
    columns[leaf]: None (the leaf lacks the column) or (docs or None = every doc, value bits uint32); accept[leaf] / live[leaf]:
    the accept set / other liveDocs words replacing the leaf's liveDocs."""
    counts = fs.clause_counts(corpus, term_ids)
    total, valued = 0, []
    for si, seg in enumerate(corpus.segments):
        ok = counts[si] >= max(int(need), 1)
        if accept is not None and accept[si] is not None:
            ok = ok & fs._bits(accept[si], seg.max_doc)
        elif live is not None and live[si] is not None:
            ok = ok & fs._bits(live[si], seg.max_doc)
        elif seg.live_bits is not None:
            ok = ok & fs._bits(seg.live_bits, seg.max_doc)
        total += int(ok.sum())
        if columns[si] is None:
            continue
        cd, cv = columns[si]
        has = np.zeros(seg.max_doc, dtype=bool)
        vals = np.zeros(seg.max_doc, dtype=np.uint32)
        idx = np.arange(seg.max_doc) if cd is None else np.asarray(cd)
        has[idx] = True
        vals[idx] = np.asarray(cv, dtype=np.uint32)
        valued.append(vals[ok & has])
    bits = fs.canonical_bits(kind, np.concatenate(valued) if valued else np.zeros(0, np.uint32))
    ub, uc = np.unique(bits, return_counts=True)
    if len(ub) > int(max_buckets):
        return np.zeros(0, np.uint32), np.zeros(0, np.int32), 0, total, -1, 1
    order = np.argsort(fs.order_key(kind, ub), kind="stable")
    return ub[order].astype(np.uint32), uc[order].astype(np.int32), int(len(ub)), total, int(uc.sum()), 0
