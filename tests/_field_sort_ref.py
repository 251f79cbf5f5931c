"""A NumPy reference of sorted searches (Sort(field) over ONE int or float doc value column, Lucene's implicit docid tie break),
independent of the library's coding of the values: which docs match is counted from the corpus postings, the order is
Integer.compare / Float.compare restated on numpy integers, and the relation follows the per-slice rule over api.slices.

  hits      all clauses SHOULD: docs matched by at least max(1, min_should_match) clauses (duplicate clauses count each);
            all clauses MUST: by all of them; inside the accept set (liveDocs & FILTER & ~MUST_NOT)
  value     the doc's column value; a doc without one, or in a leaf without the column, takes the sort's missing value
  order     value ascending (reverse: descending), equal values by global docid ascending in both directions
  page      the first k hits strictly behind the cursor (after value, after doc); total_hits counts the hits of every page
  relation  GREATER_THAN_OR_EQUAL_TO iff some slice holds more than max(total_hits_threshold, k) hits and k hits were returned

Also the small corpora the tests of this route share (leaves of chosen sizes; synth.build_corpus cuts tiered sizes only)."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from nrtsearch_amd import api, synth

INT32_MIN, INT32_MAX = -2**31, 2**31 - 1
# the values the columns of the tests draw from, in ascending order (float: Float.compare's), as bits below
INT_VALUES = np.array([INT32_MIN, -1, 0, 1, INT32_MAX], dtype=np.int32)
FLOAT_VALUES = np.array([-np.inf, -1.5, -0.0, 0.0, 1e-45, 3.25, np.inf, np.nan], dtype=np.float32)
VALUES = {"int": INT_VALUES.view(np.uint32), "float": FLOAT_VALUES.view(np.uint32)}
KIND_MIN = {"int": int(np.array([INT32_MIN], np.int32).view(np.uint32)[0]), "float": int(np.array([-np.inf], np.float32).view(np.uint32)[0])}
KIND_MAX = {"int": int(np.array([INT32_MAX], np.int32).view(np.uint32)[0]), "float": int(np.array([np.nan], np.float32).view(np.uint32)[0])}


def bits_of(kind: str, value) -> int:
    return int(np.array([value], dtype=np.int32 if kind == "int" else np.float32).view(np.uint32)[0])


def value_of(kind: str, bits: int):
    """The Python value of 32 value bits (what api.SortField.missing / api.FieldDoc.value take)."""
    v = np.array([bits], dtype=np.uint32).view(np.int32 if kind == "int" else np.float32)[0]
    return int(v) if kind == "int" else float(v)


def order_key(kind: str, bits) -> np.ndarray:
    """int64 keys that order like Integer.compare (kind "int") / Float.compare (kind "float": -0.0 < +0.0, every NaN equal and
    above +inf) of the values with these bits."""
    b = np.asarray(bits, dtype=np.uint32).astype(np.int64)
    if kind == "int":
        return np.where(b >= 2**31, b - 2**32, b)
    mag = b & 0x7FFFFFFF
    nan = mag > 0x7F800000
    neg = (b >= 2**31) & ~nan
    return np.where(nan, np.int64(0x7FC00000), np.where(neg, -mag - 1, mag))


def canonical_bits(kind: str, bits) -> np.ndarray:
    """The bits a hit reports for a value: the value's own, every NaN as 0x7FC00000."""
    b = np.asarray(bits, dtype=np.uint32).copy()
    if kind == "float":
        b[(b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)] = np.uint32(0x7FC00000)
    return b


def _bits(words: np.ndarray, n: int) -> np.ndarray:
    w = np.ascontiguousarray(words, dtype=np.uint64)
    return np.unpackbits(w.view(np.uint8), bitorder="little")[:n].astype(bool)


_count_memo: dict = {}


def clause_counts(corpus, term_ids: Sequence[int]) -> List[np.ndarray]:
    """Per leaf int32[max_doc]: the clauses of term_ids (duplicates count each) that match the doc.  Computed once per
    (corpus, clauses) and shared; callers must not write into the arrays."""
    key = (id(corpus), tuple(int(t) for t in term_ids))
    got = _count_memo.get(key)
    if got is not None and got[0] is corpus:
        return got[1]
    out = []
    for seg in corpus.segments:
        c = np.zeros(seg.max_doc, dtype=np.int32)
        for t in term_ids:
            d, _ = seg.postings(int(t))
            c[d] += 1   # (a term holds a doc once)
        c.setflags(write=False)
        out.append(c)
    _count_memo[key] = (corpus, out)
    return out


def live_count(seg) -> int:
    return seg.max_doc if seg.live_bits is None else int(_bits(seg.live_bits, seg.max_doc).sum())


def search(corpus, columns: Sequence[Optional[Tuple[Optional[np.ndarray], np.ndarray]]], kind: str, term_ids: Sequence[int], k: int,
           reverse: bool = False, missing_bits: int = 0, need: int = 1, after: Optional[Tuple[int, int]] = None,
           total_hits_threshold: int = 1000, accept: Optional[Sequence[Optional[np.ndarray]]] = None, live=None,
           slicing: Tuple[int, int, int] = (250_000, 5, 1), info: Optional[dict] = None):
    """-> (docs int32, value_bits uint32, total_hits, relation_gte).
    columns[leaf]: None (the leaf lacks the column) or (docs or None = every doc, value bits uint32); need: the clauses a hit
    matches at least; after: (global doc, value bits) of the previous page's last hit; accept[leaf] / live[leaf]: the accept
    set / other liveDocs words replacing the leaf's liveDocs; slicing: (slice_max_docs, slice_max_segments, virtual_shards)."""
    counts = clause_counts(corpus, term_ids)
    all_docs, all_bits, per_leaf = [], [], []
    for si, seg in enumerate(corpus.segments):
        ok = counts[si] >= max(int(need), 1)
        if accept is not None and accept[si] is not None:
            ok = ok & _bits(accept[si], seg.max_doc)
        elif live is not None and live[si] is not None:
            ok = ok & _bits(live[si], seg.max_doc)
        elif seg.live_bits is not None:
            ok = ok & _bits(seg.live_bits, seg.max_doc)
        vals = np.full(seg.max_doc, missing_bits, dtype=np.uint32)
        if columns[si] is not None:
            cd, cv = columns[si]
            vals[np.arange(seg.max_doc) if cd is None else np.asarray(cd)] = np.asarray(cv, dtype=np.uint32)
        d = np.nonzero(ok)[0]
        all_docs.append(d.astype(np.int64) + seg.doc_base)
        all_bits.append(vals[d])
        per_leaf.append(len(d))
    docs = np.concatenate(all_docs)
    bits = canonical_bits(kind, np.concatenate(all_bits))
    keys = order_key(kind, bits)
    signed = -keys if reverse else keys
    order = np.lexsort((docs, signed))   # by value in the sort's direction, then docid ascending
    docs, bits, signed = docs[order], bits[order], signed[order]
    total = len(docs)
    if after is not None:
        ak = int(order_key(kind, [after[1]])[0])
        ak = -ak if reverse else ak
        behind = (signed > ak) | ((signed == ak) & (docs > int(after[0])))
        docs, bits = docs[behind], bits[behind]
    docs, bits = docs[:k], bits[:k]
    if slicing[0] == 0:
        groups = [list(range(len(corpus.segments)))]
    else:
        groups, _ = api.slices([s.max_doc for s in corpus.segments], [live_count(s) for s in corpus.segments], slicing[2], slicing[0], slicing[1])
    slice_hits = [sum(per_leaf[si] for si in g) for g in groups]
    gte = any(h > max(int(total_hits_threshold), int(k)) for h in slice_hits) and len(docs) == k
    if info is not None:
        info["slice_hits"] = slice_hits
    return docs.astype(np.int32), bits.astype(np.uint32), int(total), bool(gte)


# ---- corpora with leaves of chosen sizes ---------------------------------------------------------------------------------
def make_corpus(sizes: Sequence[int], term_density: Dict[int, float], seed: int = 5, delete_fraction: float = 0.0):
    """A synth.Corpus whose leaves have exactly `sizes` docs; term t occurs in each doc independently with term_density[t]
    (1.0: in every doc); freqs 1..4 with one freq of 20 per leaf and term (the kernels' escape code)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    terms = sorted(int(t) for t in term_density)
    segments, doc_freq, base, total_len = [], {t: 0 for t in terms}, 0, 0
    for size in sizes:
        lens = np.clip(np.rint(np.exp(rng.normal(np.log(80.0), 0.6, size=size))), 4, 4000).astype(np.int32)
        total_len += int(lens.sum())
        offs, d_all, f_all = [0], [], []
        for t in terms:
            p = float(term_density[t])
            d = np.arange(size, dtype=np.int32) if p >= 1.0 else np.nonzero(rng.random(size) < p)[0].astype(np.int32)
            f = rng.integers(1, 5, size=len(d)).astype(np.int32)
            if len(f):
                f[len(f) // 2] = 20
            doc_freq[t] += len(d)
            d_all.append(d)
            f_all.append(f)
            offs.append(offs[-1] + len(d))
        live = None
        if delete_fraction > 0.0:
            alive = rng.random(size) >= delete_fraction
            padded = np.zeros(((size + 63) // 64) * 64, dtype=bool)
            padded[:size] = alive
            live = np.packbits(padded.reshape(-1, 64), axis=1, bitorder="little").view(np.uint64).reshape(-1)
        segments.append(synth.SegmentData(max_doc=int(size), doc_base=base, norms=synth.int_to_byte4(lens),
                                          term_ids=np.array(terms, np.int64), offsets=np.array(offs, np.int64),
                                          docids=np.concatenate(d_all).astype(np.int32), freqs=np.concatenate(f_all).astype(np.int32),
                                          live_bits=live))
        base += int(size)
    n = int(sum(sizes))
    return synth.Corpus(n_docs=n, doc_count=n, sum_total_term_freq=total_len, segments=segments, doc_freq=doc_freq)


def upload(ctx, corpus, kind: str, columns, field: int = 0, column_field: int = 7):
    """The corpus's leaves on the device, each with its column (None: without) under column_field -> [api.GpuSegment]."""
    leaves = []
    for seg, col in zip(corpus.segments, columns):
        g = api.GpuSegment(ctx, seg.max_doc, seg.doc_base)
        g.add_field_norms(field, seg.norms)
        g.add_terms(field, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
        if col is not None:
            g.add_doc_values(column_field, kind, np.asarray(col[1], dtype=np.uint32), col[0])
        g.seal()
        if seg.live_bits is not None:
            g.set_live_docs(seg.live_bits)
        leaves.append(g)
    return leaves
