"""A NumPy reference of the masks nrtgpu_segment_set_mask_from_values builds from doc value columns, per leaf and independent of
the library's coding of the values: the order is Integer.compare / Float.compare written out on numpy integers
(tests/_field_sort_ref.py: order_key -- -0.0 < +0.0, every NaN equal and above +inf), identity in a set is equality of those keys
(how IntPoint / FloatPoint.newSetQuery compare encoded points: -0.0 and +0.0 two members, every NaN one).

  column   ("single", docs or None = every doc, value bits uint32[n])     one value per listed doc (ascending docids)
           ("multi", value_docs int32 non-decreasing, value bits uint32)  value i belongs to doc value_docs[i]
  clause   ("range", kind, lower bits, upper bits)   a value with lower <= value <= upper; lower > upper keeps nothing
           ("exists",)                               a value (a NaN is one)
           ("in_set", kind, bits uint32[m])          a value equal to a listed one (any order, duplicates allowed)
  a doc passes a clause iff SOME value of it passes; a doc without a value fails every clause; the mask is the docs that pass
  EVERY clause, as uint64 words with the bits at and beyond max_doc 0.  liveDocs are ignored: the mask does not hold them."""
from __future__ import annotations

from typing import Sequence, Tuple

import numpy as np

from tests import _docset_ref as dsr
from tests import _field_sort_ref as fs


def value_docs_of(max_doc: int, column) -> Tuple[np.ndarray, np.ndarray]:
    """-> (doc of every value instance int64, its bits uint32), either arity"""
    arity, docs, bits = column
    bits = np.asarray(bits, dtype=np.uint32).reshape(-1)
    if arity == "single" and docs is None:
        docs = np.arange(max_doc)
    return np.asarray(docs, dtype=np.int64).reshape(-1), bits


def values_pass(clause, bits: np.ndarray) -> np.ndarray:
    """bool per value: the clause's test of values that exist"""
    if clause[0] == "exists":
        return np.ones(len(bits), dtype=bool)
    if clause[0] == "range":
        _, kind, lo, hi = clause
        return dsr.range_keeps(kind, lo, hi, bits)
    _, kind, listed = clause
    return np.isin(fs.order_key(kind, bits), fs.order_key(kind, np.asarray(listed, dtype=np.uint32)))


def clause_docs(max_doc: int, column, clause) -> np.ndarray:
    """bool[max_doc]: the docs with SOME value that passes"""
    docs, bits = value_docs_of(max_doc, column)
    keep = np.zeros(max_doc, dtype=bool)
    if len(docs):
        keep[docs[values_pass(clause, bits)]] = True
    return keep


def mask_words(max_doc: int, clauses: Sequence[tuple]) -> Tuple[np.ndarray, int]:
    """clauses: [(column, clause)] -> (the uint64 words of the docs that pass every one, their number)"""
    ok = np.ones(max_doc, dtype=bool)
    for column, clause in clauses:
        ok &= clause_docs(max_doc, column, clause)
    return dsr.pack(ok), int(ok.sum())
