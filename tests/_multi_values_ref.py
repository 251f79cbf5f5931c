"""A NumPy reference of the readers of MULTI-VALUED doc value columns (nrtgpu_segment_add_doc_values_multi), working from the
uploaded (value_docs, values) arrays and independent of the library's coding of the values.

  column    per leaf None (the leaf lacks the column) or (value_docs int32 non-decreasing, value bits uint32): value i belongs to
            leaf doc value_docs[i]; a doc listed c times has c values, duplicates included
  counting  every value instance of every hit adds 1 to its value's bucket (the reference's for (i < docValues.size())
            countsMap.addTo(docValues.get(i), 1)): a loop over the hits' value instances, the bits canonicalised as
            tests/_terms_count_ref.py does (every NaN 0x7FC00000; -0.0 and +0.0 two buckets); total_hits counts hits,
            hits_with_value the value INSTANCES counted
  range     a doc passes iff ANY of its values lies in [lower, upper] under tests/_docset_ref.py's long-hand compare; a doc with
            no value, or in a leaf without the column, fails
  hit sets  tests/_field_sort_ref.py's clause counts (text queries) and tests/_docset_ref.py's hit_set (doc sets), as uint64 words
            per leaf; a multi-valued range clause enters hit_set as one more filter (any_in_range)
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np

from tests import _docset_ref as dsr
from tests import _field_sort_ref as fs

Column = Sequence[Optional[Tuple[np.ndarray, np.ndarray]]]


def text_hits(corpus, term_ids: Sequence[int], need: int = 1, accept=None, live=None):
    """-> per leaf the hits of a text query as uint64 words (tests/_field_sort_ref.py's matching)."""
    counts = fs.clause_counts(corpus, term_ids)
    out = []
    for si, seg in enumerate(corpus.segments):
        ok = counts[si] >= max(int(need), 1)
        if accept is not None and accept[si] is not None:
            ok = ok & fs._bits(accept[si], seg.max_doc)
        elif live is not None and live[si] is not None:
            ok = ok & fs._bits(live[si], seg.max_doc)
        elif seg.live_bits is not None:
            ok = ok & fs._bits(seg.live_bits, seg.max_doc)
        out.append(dsr.pack(ok))
    return out


def any_in_range(corpus, kind: str, columns: Column, lower_bits: int, upper_bits: int):
    """-> per leaf, as uint64 words, the docs with SOME value in the range."""
    out = []
    for si, seg in enumerate(corpus.segments):
        keep = np.zeros(seg.max_doc, dtype=bool)
        if columns[si] is not None:
            vd, vb = columns[si]
            vd, vb = np.asarray(vd, dtype=np.int64), np.asarray(vb, dtype=np.uint32)
            if len(vd):
                keep[vd[dsr.range_keeps(kind, lower_bits, upper_bits, vb)]] = True
        out.append(dsr.pack(keep))
    return out


def count(corpus, hits, columns: Column, kind: str, max_buckets: int = 65536):
    """-> (value_bits uint32 ascending in the kind's order, counts int32, n_buckets, total_hits, hits_with_value, overflowed);
    hits: per leaf uint64 words."""
    total, instances = 0, []
    for si, seg in enumerate(corpus.segments):
        ok = fs._bits(hits[si], seg.max_doc)
        total += int(ok.sum())
        if columns[si] is None:
            continue
        vd, vb = columns[si]
        vd, vb = np.asarray(vd, dtype=np.int64), np.asarray(vb, dtype=np.uint32)
        instances.append(vb[ok[vd]] if len(vd) else vb)
    bits = fs.canonical_bits(kind, np.concatenate(instances) if instances else np.zeros(0, np.uint32))
    ub, uc = np.unique(bits, return_counts=True)
    if len(ub) > int(max_buckets):
        return np.zeros(0, np.uint32), np.zeros(0, np.int32), 0, total, -1, 1
    order = np.argsort(fs.order_key(kind, ub), kind="stable")
    return ub[order].astype(np.uint32), uc[order].astype(np.int32), int(len(ub)), total, int(uc.sum()), 0
