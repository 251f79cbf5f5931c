"""A NumPy reference of function-score searches over multi-match queries (include/nrtgpu.h:
nrtgpu_search_function_score_multi_match_batch), built ON the two existing references without touching them:

  tests/_multi_match_ref.py     leaf_finals: per leaf (inner float32[max_doc], inner_hit bool[max_doc]) of the two-level query
  tests/_function_score_ref.py  final_scores: (final, hit) of the docs handed to it, from their inner scores and function sets

Per doc: (inner, inner_hit) by the multi-match rule; a doc with not inner_hit, or outside the accept set, is no hit at all; for the
others (final, hit) by the function-score rule -- then one oracle.Collector per slice (oracle.corpus_slices), each visiting its
leaves in docBase order, and oracle.topdocs_merge.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from tests import _function_score_ref as fs_ref
from tests import _multi_match_ref as mm_ref

f32, f64 = np.float32, np.float64


def value(shape: str, group_of: Sequence[int], scores: np.ndarray, matched: np.ndarray, operator, msm, tie_breaker: float,
          member: Sequence[Optional[np.ndarray]], weights: Sequence[float], score_mode: str, boost_mode: str, min_score: float = 0.0,
          min_excluded: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """The per-doc rule.  scores float32[C, n], matched bool[C, n], member[i] bool[n] or None -> (final float32[n], is_hit bool[n]);
    final is only meaningful where is_hit."""
    inner, inner_hit = mm_ref.combine(shape, group_of, scores, matched, operator, msm, tie_breaker)
    final, hit = fs_ref.final_scores(inner, member, weights, score_mode, boost_mode, min_score, min_excluded)
    return final, inner_hit & hit


def search(oracle, fields: Sequence, groups, shape: str, k: int, operator: str = "should", msm=0, tie_breaker: float = 0.0,
           functions: Sequence[Tuple[int, float]] = (), score_mode: str = "multiply", boost_mode: str = "multiply", min_score: float = 0.0,
           min_excluded: bool = False, masks: Optional[Dict[Tuple[int, int], np.ndarray]] = None, after: Optional[Tuple[int, float]] = None,
           total_hits_threshold: int = 1000, accept: Optional[Sequence[Optional[np.ndarray]]] = None, slicing="default", live=None,
           info: Optional[dict] = None):
    """-> (docs, scores, total_hits, relation_gte), the shape of oracle.search_bm25.
    The multi-match arguments are _multi_match_ref.search's, the function-score arguments _function_score_ref.search's:
    functions: (mask id or 0, weight) in the request's order; masks[(leaf, id)]: the function filter's doc set as 64-bit words."""
    if slicing == "default":
        slicing = oracle.DEFAULT_SLICING
    inner_finals = mm_ref.leaf_finals(oracle, fields, groups, shape, operator, msm, tie_breaker)
    lists, total, gte, slice_hits = [], 0, False, []
    for g in oracle.corpus_slices(fields[0], slicing):
        col = oracle.Collector(k, after, total_hits_threshold)
        n_slice = 0
        for si in g:
            seg = fields[0].segments[si]
            inner, inner_hit = inner_finals[si]
            ok = inner_hit.copy()
            if accept is not None and accept[si] is not None:
                ok &= mm_ref._bits(accept[si], seg.max_doc)
            elif live is not None and live[si] is not None:
                ok &= mm_ref._bits(live[si], seg.max_doc)
            elif seg.live_bits is not None:
                ok &= mm_ref._bits(seg.live_bits, seg.max_doc)
            docs = np.nonzero(ok)[0]                                  # the accepted inner hits
            member = [None if mid == 0 else mm_ref._bits(masks[(si, mid)], seg.max_doc)[docs] for mid, _ in functions]
            final, hit = fs_ref.final_scores(inner[docs], member, [w for _, w in functions], score_mode, boost_mode, min_score, min_excluded)
            col.set_leaf(seg.doc_base)
            for d, s in zip(docs[hit].tolist(), final[hit].tolist()):
                col.collect(d, s)
            n_slice += int(hit.sum())
        d, s, t, ge = col.topdocs()
        col.close()
        lists.append((d, s))
        total += t
        gte = gte or ge
        slice_hits.append(n_slice)
    docs, scores = oracle.topdocs_merge(k, lists)
    if info is not None:
        info["slice_hits"] = slice_hits
    return docs, scores, int(total), bool(gte)


_mask_memo: dict = {}


def function_masks(fields) -> Dict[Tuple[int, int], np.ndarray]:
    """The function filters' doc sets on the test index of _multi_match_ref.build_index: masks[(leaf, id)] for ids 7 (40 % of the docs)
    and 9 (10 %) -- the masks tests/test_multi_match_gpu.py sets.  Built once; read-only."""
    got = _mask_memo.get(id(fields))
    if got is not None and got[0] is fields:
        return got[1]
    from nrtsearch_amd import synth
    masks = {(si, mid): synth.random_mask(seg.max_doc, dens, 10 * mid + si) for si, seg in enumerate(fields[0].segments)
             for mid, dens in ((7, 0.4), (9, 0.1))}
    _mask_memo[id(fields)] = (fields, masks)
    return masks


def to_query(api, groups, shape: str, operator: str = "should", msm=0, tie_breaker: float = 0.0, functions: Sequence[Tuple[int, float]] = (),
             score_mode: str = "multiply", boost_mode: str = "multiply", min_score: float = 0.0, min_excluded: bool = False, filter=(), must_not=()):
    """The same query as the mirror's objects: a FunctionScoreQuery whose inner query is a MultiMatchQuery."""
    inner = mm_ref.to_query(api, groups, shape, operator, msm, tie_breaker, filter, must_not)
    return api.FunctionScoreQuery(inner, tuple(api.WeightFunction(float(w), int(m)) for m, w in functions), score_mode, boost_mode,
                                  float(min_score), bool(min_excluded))
