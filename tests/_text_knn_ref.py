"""A NumPy reference of searches whose request carries a `query` AND `knn` clauses (nrtgpu_search_text_knn_batch), built ON
the oracle without changing it: the oracle's host helpers give the BM25 statistics, its exact vector search the knn lists, its
Collector (LazyQueueTopScoreDocCollector) collects per slice, its topdocs_merge reduces.

The reference resolves every knn query to a doc-and-score query over its top k and ORs those into the main query as further
SHOULD clauses of one BooleanQuery (SearchRequestProcessor.java:267-296).  Per leaf:

  text      the float64 sum of the matching text clauses' float32 BM25 scores (inner_scores of _function_score_ref.py without
            the final cast) and the matched bits; they count only inside the accept set (liveDocs & FILTER & ~MUST_NOT)
  knn_sum   the float64 sum, in list order, of float32(score * boost) over the lists that hold the doc
  FLAT      text and lists: float32(text + knn_sum)      NESTED: float32(float64(float32(text)) + knn_sum)
            text only: float32(text)                     lists only: float32(knn_sum)
  hits      (text matches and accepted) or (listed and live in its leaf)

-- then one Collector per slice (oracle.corpus_slices), each visiting its leaves in docBase order, and TopDocs.merge.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from nrtsearch_amd import synth

f32, f64 = np.float32, np.float64
_text_memo: dict = {}


def _bits(words: np.ndarray, n: int) -> np.ndarray:
    """bool[n]: bit d of the 64-bit words."""
    w = np.ascontiguousarray(words, dtype=np.uint64)
    return np.unpackbits(w.view(np.uint8), bitorder="little")[:n].astype(bool)


def words_of(flags: np.ndarray) -> np.ndarray:
    """bool[n] -> 64-bit words."""
    n = len(flags)
    padded = np.zeros(((n + 63) // 64) * 64, dtype=bool)
    padded[:n] = flags
    return np.packbits(padded.reshape(-1, 64), axis=1, bitorder="little").view(np.uint64).reshape(-1)


def make_corpus(sizes: Sequence[int], ranks: Sequence[int], delete_fraction: float = 0.0, seed: int = 1234,
                without: Sequence[Tuple[int, int]] = ()) -> synth.Corpus:
    """synth.build_corpus with the leaves' sizes given.  without: (leaf, term) pairs whose postings are left out of that leaf."""
    ranks = sorted(set(int(r) for r in ranks))
    n_docs = int(sum(sizes))
    lens, postings_of = synth.corpus_variant_arrays(n_docs, "iid", seed)
    norms_all = synth.int_to_byte4(lens)
    bases = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    rng = np.random.Generator(np.random.PCG64(seed + 99))
    per_term = {r: postings_of(r) for r in ranks}
    doc_freq = {r: 0 for r in ranks}
    segments = []
    for s, size in enumerate(sizes):
        docs, freqs, counts = [], [], []
        for r in ranks:
            d, f = per_term[r]
            lo, hi = np.searchsorted(d, [bases[s], bases[s + 1]])
            if (s, r) in without:
                hi = lo
            docs.append((d[lo:hi] - bases[s]).astype(np.int32))
            freqs.append(f[lo:hi])
            counts.append(int(hi - lo))
            doc_freq[r] += int(hi - lo)
        live = None
        if delete_fraction > 0.0:
            alive = rng.random(size) >= delete_fraction
            if alive.all():
                alive[size // 2] = False
            live = words_of(alive)
        segments.append(synth.SegmentData(max_doc=int(size), doc_base=int(bases[s]), norms=norms_all[bases[s]: bases[s] + size].copy(),
                                          term_ids=np.asarray(ranks, dtype=np.int64),
                                          offsets=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64),
                                          docids=np.ascontiguousarray(np.concatenate(docs), dtype=np.int32),
                                          freqs=np.ascontiguousarray(np.concatenate(freqs), dtype=np.int32), live_bits=live))
    return synth.Corpus(n_docs=n_docs, doc_count=n_docs, sum_total_term_freq=int(lens.astype(np.int64).sum()), segments=segments,
                        doc_freq=doc_freq)


def text_sums(oracle, corpus, term_ids: Sequence[int], boosts: Optional[Sequence[float]] = None):
    """Per leaf (matched bool[max_doc], sum float64[max_doc]) of the SHOULD disjunction over term_ids: the clause scores added in
    float64, no final cast.  Computed once per (corpus, clauses) and shared; callers must not write into the arrays."""
    key = (id(corpus), tuple(int(t) for t in term_ids), None if boosts is None else tuple(float(b) for b in boosts))
    got = _text_memo.get(key)
    if got is not None and got[0] is corpus:
        return got[1]
    weights, cache = oracle.bm25_query_stats(corpus, term_ids, boosts)
    leaves = []
    for seg in corpus.segments:
        acc = np.zeros(seg.max_doc, dtype=f64)
        matched = np.zeros(seg.max_doc, dtype=bool)
        for i, t in enumerate(term_ids):
            d, fr = seg.postings(int(t))
            if len(d) == 0:
                continue
            w = f32(weights[i])
            ninv = cache[np.asarray(seg.norms)[d].astype(np.int64)].astype(f32)
            prod = (fr.astype(f32) * ninv).astype(f32)          # BM25Similarity SimScorer.score: one rounding per operation
            den = (f32(1.0) + prod).astype(f32)
            quo = (w / den).astype(f32)
            sc = (w - quo).astype(f32)
            np.add.at(acc, d, sc.astype(f64))
            matched[d] = True
        acc.setflags(write=False)
        matched.setflags(write=False)
        leaves.append((matched, acc))
    _text_memo[key] = (corpus, leaves)
    return leaves


def combine(text: np.ndarray, text_ok: np.ndarray, knn_sum: np.ndarray, listed: np.ndarray, nested: bool) -> np.ndarray:
    """float32[n]: the score of every doc by the four cases above (docs that are no hit: whatever)."""
    text = np.asarray(text, dtype=f64)
    knn_sum = np.asarray(knn_sum, dtype=f64)
    both = (text.astype(f32).astype(f64) + knn_sum).astype(f32) if nested else (text + knn_sum).astype(f32)
    return np.where(text_ok & listed, both, np.where(text_ok, text.astype(f32), knn_sum.astype(f32))).astype(f32)


def clause_values(scores, boost: float) -> np.ndarray:
    """float32(score * boost): one float multiply."""
    return (np.asarray(scores, dtype=f32) * f32(boost)).astype(f32)


def knn_sums(corpus, lists: Sequence[Tuple[Sequence[int], Sequence[float], float]]):
    """Per leaf (listed bool[max_doc], knn_sum float64[max_doc]); lists: (global docids, scores, boost) in the request's order."""
    out = []
    for seg in corpus.segments:
        ks = np.zeros(seg.max_doc, dtype=f64)
        listed = np.zeros(seg.max_doc, dtype=bool)
        for docs, scores, boost in lists:
            docs = np.asarray(docs, dtype=np.int64)
            vals = clause_values(scores, boost)
            here = (docs >= seg.doc_base) & (docs < seg.doc_base + seg.max_doc)
            local = docs[here] - seg.doc_base
            ks[local] = ks[local] + vals[here].astype(f64)    # (no doc twice in one list)
            listed[local] = True
        out.append((listed, ks))
    return out


def search(oracle, corpus, term_ids: Sequence[int], k: int, lists=(), nested: bool = False,
           accept: Optional[Sequence[Optional[np.ndarray]]] = None, boosts: Optional[Sequence[float]] = None,
           after: Optional[Tuple[int, float]] = None, total_hits_threshold: int = 1000, slicing="default", info: Optional[dict] = None):
    """-> (docs, scores, total_hits, relation_gte), the shape of oracle.search_bm25.
    accept[leaf]: the text query's accept set (liveDocs & FILTER & ~MUST_NOT) as 64-bit words; None: the leaf's liveDocs.
    info["kinds"]: how many listed docs match the text ("text"), do not ("no_text"), lie outside the accept set but are live
    ("outside"), are deleted ("deleted"); info["hits"]: the hits."""
    if slicing == "default":
        slicing = oracle.DEFAULT_SLICING
    leaves = text_sums(oracle, corpus, term_ids, boosts)
    ksums = knn_sums(corpus, lists)
    groups = oracle.corpus_slices(corpus, slicing)
    kinds = {"text": 0, "no_text": 0, "outside": 0, "deleted": 0}
    out_lists, total, gte = [], 0, False
    for g in groups:
        col = oracle.Collector(k, after, total_hits_threshold)
        for si in g:
            seg = corpus.segments[si]
            matched, text = leaves[si]
            listed, ks = ksums[si]
            live = _bits(seg.live_bits, seg.max_doc) if seg.live_bits is not None else np.ones(seg.max_doc, dtype=bool)
            acc = _bits(accept[si], seg.max_doc) & live if accept is not None and accept[si] is not None else live
            text_ok = matched & acc
            listed_live = listed & live
            hit = text_ok | listed_live
            final = combine(text, text_ok, ks, listed_live, nested)
            kinds["text"] += int((listed_live & text_ok).sum())
            kinds["no_text"] += int((listed_live & acc & ~matched).sum())
            kinds["outside"] += int((listed_live & ~acc).sum())
            kinds["deleted"] += int((listed & ~live).sum())
            col.set_leaf(seg.doc_base)
            docs = np.nonzero(hit)[0]
            for d, s in zip(docs.tolist(), final[docs].tolist()):
                col.collect(d, s)
        d, s, t, ge = col.topdocs()
        col.close()
        out_lists.append((d, s))
        total += t
        gte = gte or ge
    docs, scores = oracle.topdocs_merge(k, out_lists)
    if info is not None:
        info["kinds"] = kinds
    return docs, scores, int(total), bool(gte)


def leaf_vectors(corpus, dim: int = 8, seed: int = 777) -> List[np.ndarray]:
    """Small synthetic vectors, one row per doc of every leaf."""
    return [synth.make_vectors(seg.max_doc, dim, seed + si) for si, seg in enumerate(corpus.segments)]


def knn_list(oracle, corpus, vectors: Sequence[np.ndarray], sim: int, query: np.ndarray, k: int, boost: float = 1.0,
             accept: Optional[Sequence[Optional[np.ndarray]]] = None) -> Tuple[np.ndarray, np.ndarray]:
    """What a knn search returns for one query: the k best live (accepted) docs of all leaves by oracle.knn_exact, scores with the
    boost applied, ranked (score desc, doc asc)."""
    per_leaf = []
    for si, seg in enumerate(corpus.segments):
        words = accept[si] if accept is not None and accept[si] is not None else seg.live_bits
        kk = min(k, seg.max_doc)
        d, s, n = oracle.knn_exact(sim, query[None, :], vectors[si], kk, live_words=words, doc_base=seg.doc_base, boost=boost)
        per_leaf.append((d[0, : n[0]], s[0, : n[0]]))
    return oracle.topdocs_merge(k, per_leaf)
