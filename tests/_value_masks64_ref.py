"""A NumPy / Python reference of filter masks built from 64-bit doc value columns (nrtgpu_segment_set_mask_from_values64): the docs
of one leaf that pass EVERY clause, with Long.compare / Double.compare written out on Python integers
(tests/_field_sort64_ref.py: order_int), not through the library's coding.

  range    the doc has a value with lower <= value <= upper, both inclusive, in the kind's order (doubles: -0.0 < +0.0, every
           NaN equal and above +inf); lower > upper matches nothing
  exists   the doc has a value (a NaN is one)
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np

from tests import _field_sort64_ref as ref


def passes(max_doc: int, column: Optional[Tuple[Optional[np.ndarray], np.ndarray]], kind: str, clause) -> np.ndarray:
    """bool[max_doc] for one clause: ("range", lower_bits, upper_bits) or ("exists",); column: (docs or None, value bits uint64)."""
    has = np.zeros(max_doc, dtype=bool)
    keys = np.zeros(max_doc, dtype=np.int64)
    cd, cv = column
    idx = np.arange(max_doc) if cd is None else np.asarray(cd)
    has[idx] = True
    keys[idx] = ref.order_key(kind, cv)
    if clause[0] == "exists":
        return has
    lo, hi = ref.order_int(kind, clause[1]), ref.order_int(kind, clause[2])
    return has & (keys >= lo) & (keys <= hi) if lo <= hi else np.zeros(max_doc, dtype=bool)


def words(ok: np.ndarray) -> np.ndarray:
    """The (max_doc + 63) / 64 uint64 words of a doc set (bits at or beyond max_doc 0)."""
    padded = np.zeros(((len(ok) + 63) // 64) * 64, dtype=bool)
    padded[: len(ok)] = ok
    return np.packbits(padded.reshape(-1, 64), axis=1, bitorder="little").view(np.uint64).reshape(-1)


def mask(max_doc: int, clauses: Sequence[Tuple]) -> np.ndarray:
    """clauses: (column, kind, clause) each -> the words of the docs that pass every one."""
    ok = np.ones(max_doc, dtype=bool)
    for column, kind, clause in clauses:
        ok &= passes(max_doc, column, kind, clause)
    return words(ok)
