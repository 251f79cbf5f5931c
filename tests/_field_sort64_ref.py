"""A NumPy / Python reference of sorted searches over ONE 64-bit doc value column (LONG / DATE_TIME as int64, DOUBLE as float64),
independent of the library's coding of the values and of its packed keys: the order is Long.compare / Double.compare written out
on Python / NumPy integers, which docs match is counted from the corpus postings (tests/_field_sort_ref.py: clause_counts) or
taken from a doc set's accept words and 32-bit range clauses, the relation follows the per-slice rule over api.slices.

  value     the doc's column value; a doc without one, or in a leaf without the column, takes the sort's missing value; every NaN
            is reported as 0x7FF8000000000000, a NaN missing value included
  order     value ascending (reverse: descending), equal values by global docid ascending in both directions
  page      the first k hits strictly behind the cursor (after value, after doc); total_hits counts the hits of every page
  relation  GREATER_THAN_OR_EQUAL_TO iff some slice holds more than max(total_hits_threshold, k) hits and k hits were returned
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from nrtsearch_amd import api

from tests import _field_sort_ref as fs

INT64_MIN, INT64_MAX = -2**63, 2**63 - 1
U64 = 2**64
CANONICAL_NAN = 0x7FF8000000000000
DTYPES = {"long": np.int64, "double": np.float64}


def bits_of(kind: str, value) -> int:
    return int(np.array([value], dtype=DTYPES[kind]).view(np.uint64)[0])


def value_of(kind: str, bits: int):
    """The Python value of 64 value bits (what api.SortField64.missing / api.FieldDoc.value take)."""
    v = np.array([bits], dtype=np.uint64).view(DTYPES[kind])[0]
    return int(v) if kind == "long" else float(v)


def order_int(kind: str, bits: int) -> int:
    """A Python int that orders like Long.compare (kind "long") / Double.compare (kind "double": -0.0 < +0.0, every NaN equal and
    above +inf) of the value with these 64 bits."""
    b = int(bits) & (U64 - 1)
    if kind == "long":
        return b - U64 if b >= 2**63 else b
    mag = b & (2**63 - 1)
    if mag > 0x7FF0000000000000:
        return CANONICAL_NAN
    return -mag - 1 if b >= 2**63 else mag


def order_key(kind: str, bits) -> np.ndarray:
    """order_int over an array, as int64 (every key fits)."""
    b = np.asarray(bits, dtype=np.uint64)
    if kind == "long":
        return b.view(np.int64) if b.flags.c_contiguous else np.ascontiguousarray(b).view(np.int64)
    mag = (b & np.uint64(2**63 - 1)).astype(np.int64)
    nan = mag > 0x7FF0000000000000
    neg = (b >= np.uint64(2**63)) & ~nan
    return np.where(nan, np.int64(CANONICAL_NAN), np.where(neg, -mag - 1, mag))


def canonical_bits(kind: str, bits) -> np.ndarray:
    """The bits a hit reports for a value: the value's own, every NaN as 0x7FF8000000000000."""
    b = np.asarray(bits, dtype=np.uint64).copy()
    if kind == "double":
        b[(b & np.uint64(2**63 - 1)) > np.uint64(0x7FF0000000000000)] = np.uint64(CANONICAL_NAN)
    return b


def text_hits(corpus, term_ids: Sequence[int], need: int = 1, accept=None, live=None) -> List[np.ndarray]:
    """Per leaf bool[max_doc]: the docs a text query hits (tests/_field_sort_ref.py: search's matching)."""
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
        out.append(ok)
    return out


def docset_hits(corpus, filters=(), must_nots=(), ranges32=()) -> List[np.ndarray]:
    """Per leaf bool[max_doc]: liveDocs AND every filter AND no must_not AND every 32-bit range clause.
    filters / must_nots: per mask a list of per-leaf words; ranges32: (columns, kind, lower_bits, upper_bits) with columns as in
    _field_sort_ref.search."""
    out = []
    for si, seg in enumerate(corpus.segments):
        ok = np.ones(seg.max_doc, dtype=bool) if seg.live_bits is None else fs._bits(seg.live_bits, seg.max_doc)
        for m in filters:
            ok = ok & fs._bits(m[si], seg.max_doc)
        for m in must_nots:
            ok = ok & ~fs._bits(m[si], seg.max_doc)
        for columns, kind, lo, hi in ranges32:
            has = np.zeros(seg.max_doc, dtype=bool)
            vals = np.zeros(seg.max_doc, dtype=np.uint32)
            if columns[si] is not None:
                cd, cv = columns[si]
                idx = np.arange(seg.max_doc) if cd is None else np.asarray(cd)
                has[idx] = True
                vals[idx] = np.asarray(cv, dtype=np.uint32)
            k = fs.order_key(kind, vals)
            ok = ok & has & (k >= int(fs.order_key(kind, [lo])[0])) & (k <= int(fs.order_key(kind, [hi])[0]))
        out.append(ok)
    return out


def search(corpus, hits: Sequence[np.ndarray], columns: Sequence[Optional[Tuple[Optional[np.ndarray], np.ndarray]]], kind: str, k: int,
           reverse: bool = False, missing_bits: int = 0, after: Optional[Tuple[int, int]] = None, total_hits_threshold: int = 1000,
           slicing: Tuple[int, int, int] = (250_000, 5, 1), doc_bases: Optional[Sequence[int]] = None, info: Optional[dict] = None):
    """-> (docs int32, value_bits uint64, total_hits, relation_gte).  hits[leaf]: bool per doc; columns[leaf]: None (the leaf
    lacks the column) or (docs or None = every doc, value bits uint64); after: (global doc, value bits)."""
    all_docs, all_bits, per_leaf = [], [], []
    missing_bits = int(canonical_bits(kind, [missing_bits])[0])   # (every NaN a sort reports is canonical, the missing value included)
    for si, seg in enumerate(corpus.segments):
        vals = np.full(seg.max_doc, missing_bits, dtype=np.uint64)
        if columns[si] is not None:
            cd, cv = columns[si]
            vals[np.arange(seg.max_doc) if cd is None else np.asarray(cd)] = canonical_bits(kind, np.asarray(cv, dtype=np.uint64))
        d = np.nonzero(hits[si])[0]
        all_docs.append(d.astype(np.int64) + (seg.doc_base if doc_bases is None else int(doc_bases[si])))
        all_bits.append(vals[d])
        per_leaf.append(len(d))
    docs = np.concatenate(all_docs)
    bits = np.concatenate(all_bits)
    keys = order_key(kind, bits)
    signed = ~keys if reverse else keys   # (~k = -k - 1 reverses the order without overflowing at INT64_MIN)
    order = np.lexsort((docs, signed))
    docs, bits, signed = docs[order], bits[order], signed[order]
    total = len(docs)
    if after is not None:
        ak = np.int64(order_int(kind, after[1]))
        ak = ~ak if reverse else ak
        behind = (signed > ak) | ((signed == ak) & (docs > int(after[0])))
        docs, bits = docs[behind], bits[behind]
    docs, bits = docs[:k], bits[:k]
    if slicing[0] == 0:
        groups = [list(range(len(corpus.segments)))]
    else:
        groups, _ = api.slices([s.max_doc for s in corpus.segments], [fs.live_count(s) for s in corpus.segments], slicing[2], slicing[0], slicing[1])
    slice_hits = [sum(per_leaf[si] for si in g) for g in groups]
    gte = any(h > max(int(total_hits_threshold), int(k)) for h in slice_hits) and len(docs) == k
    if info is not None:
        info["slice_hits"] = slice_hits
    return docs.astype(np.int32), bits.astype(np.uint64), int(total), bool(gte)


def upload(ctx, corpus, kind: str, columns, field: int = 0, column_field: int = 7, doc_bases: Optional[Sequence[int]] = None, more=None):
    """The corpus's leaves on the device, each with its 64-bit column (None: without) under column_field -> [api.GpuSegment].
    more(g, si): further uploads before the seal."""
    leaves = []
    for si, (seg, col) in enumerate(zip(corpus.segments, columns)):
        g = api.GpuSegment(ctx, seg.max_doc, seg.doc_base if doc_bases is None else int(doc_bases[si]))
        g.add_field_norms(field, seg.norms)
        g.add_terms(field, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
        if col is not None:
            g.add_doc_values64(column_field, kind, np.asarray(col[1], dtype=np.uint64), col[0])
        if more is not None:
            more(g, si)
        g.seal()
        if seg.live_bits is not None:
            g.set_live_docs(seg.live_bits)
        leaves.append(g)
    return leaves
