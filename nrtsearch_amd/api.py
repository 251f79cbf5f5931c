"""Host-side mirror of the reference's operator surface for the accelerated path.

Names and argument meaning follow Lucene / nrtsearch so the parity tests read like the reference's
own tests:

  reference                                                         here
  ---------------------------------------------------------------   ---------------------------
  org.apache.lucene.search.TermQuery / BoostQuery / BooleanQuery     TermQuery / BoostQuery / BooleanQuery
  BM25Similarity.scorer(boost, collectionStats, termStats)           BM25Similarity.scorer
  TopScoreDocCollectorManager(numHits, after, totalHitsThreshold)    TopScoreDocCollectorManager
     (S/search/collectors/RelevanceCollector.java:63-68)
  IndexSearcher.search(Query, CollectorManager)                      GpuIndexSearcher.search
     (S/handler/SearchHandler.java:1412-1413)
  TopDocs / TotalHits.Relation                                       TopDocs

Everything numeric happens behind the C ABI (include/nrtgpu.h) on the GPU; this module only
marshals.  It has no CPU implementation of the query path.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import os
import threading
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib
from ._lib import NrtGpuError  # noqa: F401  (re-export)

INT_MAX = 2**31 - 1
TOTAL_HITS_THRESHOLD = 1000  # S/search/SearchRequestProcessor.java:102


# ---- queries (only the shapes eligible for the device route) ------------------------
EXCHANGE_ALLGATHER, EXCHANGE_ALLTOALL = 0, 1   # nrtgpu.h: NRTGPU_EXCHANGE_*
EXCHANGE_NO_SPECULATION = 0x100               # ... or-ed into dist_search_batch's mode: no shard-level guesses


@dataclasses.dataclass(frozen=True)
class TermQuery:
    field: int
    term: int  # injective 64-bit id of the term (the Java shim hashes the BytesRef)


@dataclasses.dataclass(frozen=True)
class BoostQuery:
    query: TermQuery
    boost: float


@dataclasses.dataclass(frozen=True)
class MaskFilter:
    """A non-scoring clause whose per-leaf doc set is resident as a mask (GpuSegment.set_mask): what a
    FILTER / MUST_NOT clause is once LRUQueryCache holds its DocIdSet."""

    mask_id: int


@dataclasses.dataclass(frozen=True)
class BooleanQuery:
    """SHOULD disjunction of term clauses, optionally narrowed by one FILTER and one MUST_NOT clause
    (S/query/QueryNodeMapper.java:257-283)."""

    should: Tuple[Union[TermQuery, BoostQuery], ...] = ()
    minimum_number_should_match: int = 0
    filter: Tuple[MaskFilter, ...] = ()
    must_not: Tuple[MaskFilter, ...] = ()
    must: Tuple[Union[TermQuery, BoostQuery], ...] = ()   # MatchQuery with operator MUST (QueryNodeMapper.java:369-373)


@dataclasses.dataclass(frozen=True)
class DisjunctionMaxQuery:
    """DisjunctionMaxQuery over (boosted) term queries (S/query/QueryNodeMapper.java:350-358): a doc scores its best
    disjunct plus tie_breaker_multiplier x the others (0..1)."""

    disjuncts: Tuple[Union[TermQuery, BoostQuery], ...] = ()
    tie_breaker_multiplier: float = 0.0


Query = Union[TermQuery, BoostQuery, BooleanQuery, DisjunctionMaxQuery]


@dataclasses.dataclass(frozen=True)
class WeightFunction:
    """One FilterFunction of a MultiFunctionScoreQuery that is a plain weight (S/query/multifunction/WeightFilterFunction.java):
    docs in the function's filter -- a resident mask, 0 = no filter query: every doc -- get `weight`.  The request's weight 0
    means 1 (FilterFunction.java:83): the caller maps it."""

    weight: float
    mask_id: int = 0


@dataclasses.dataclass(frozen=True)
class FunctionScoreQuery:
    """MultiFunctionScoreQuery with weight functions over a BM25 disjunction (S/query/multifunction/MultiFunctionScoreQuery.java):
    score_mode "multiply" / "sum" combines the matching functions' weights, boost_mode "multiply" / "sum" / "replace" combines
    that with the inner score; min_score / min_excluded drop docs whose final score fails the test.
    `inner` may also be a MultiMatchQuery: GpuIndexSearcher.search_function_score_multi_match_batch runs that form."""

    inner: Union[Query, "MultiMatchQuery"]
    functions: Tuple[WeightFunction, ...] = ()
    score_mode: str = "multiply"
    boost_mode: str = "multiply"
    min_score: float = 0.0
    min_excluded: bool = False


@dataclasses.dataclass(frozen=True, eq=False)
class KnnClause:
    """One resolved knn clause of a request that also carries a `query` (nrtgpu_doc_scores): the global docids and vector scores
    a knn search returned, ORed into the text query as a SHOULD clause worth (float)(score * boost) per doc
    (S/search/SearchRequestProcessor.java:267-296).  boost 1.0 when the scores carry the boost already."""

    docs: np.ndarray
    scores: np.ndarray
    boost: float = 1.0


SCORE_MODES = {"multiply": 0, "sum": 1}                  # nrtgpu_function_score.score_mode
BOOST_MODES = {"multiply": 0, "sum": 1, "replace": 2}    # ... .boost_mode


@dataclasses.dataclass(frozen=True)
class MultiMatchQuery:
    """The two-level queries of the reference's multiMatchQuery (S/query/QueryNodeMapper.java:429-528) over term clauses:
    shape "cross_fields": a BooleanQuery with one clause per group (a token), each group the DisjunctionMaxQuery of the token's
    per-field term queries (MatchCrossFieldsQuery / BlendedTermQuery); operator "should" with minimum_number_should_match, or "must".
    shape "best_fields": a DisjunctionMaxQuery with one disjunct per group (a field), each group a BooleanQuery of the field's term
    clauses; operator "should" with a minimum per group (an int for all groups, or a tuple), or "must".
    tie_breaker_multiplier belongs to the DisjunctionMax level.  Field boosts ride in BoostQuery clauses."""

    shape: str
    groups: Tuple[Tuple[Union[TermQuery, BoostQuery], ...], ...]
    operator: str = "should"
    minimum_number_should_match: Union[int, Tuple[int, ...]] = 0
    tie_breaker_multiplier: float = 0.0
    filter: Tuple[MaskFilter, ...] = ()
    must_not: Tuple[MaskFilter, ...] = ()


GROUP_SHAPES = {"cross_fields": _lib.NRTGPU_GROUPS_SUM_OF_MAX, "best_fields": _lib.NRTGPU_GROUPS_MAX_OF_SUM}   # nrtgpu_clause_groups.shape


DOC_VALUE_KINDS = {"int": (_lib.NRTGPU_DOCVALUES_INT32, np.dtype(np.int32)), "float": (_lib.NRTGPU_DOCVALUES_FLOAT32, np.dtype(np.float32))}


def _value_bits(kind: str, value) -> int:
    """The 32 bits of a doc value of the kind (an int32 / a float32)."""
    return int(np.array([value], dtype=DOC_VALUE_KINDS[kind][1]).view(np.uint32)[0])


# 64-bit columns (GpuSegment.add_doc_values64): LONG / DATE_TIME (epoch millis) and DOUBLE doc values
DOC_VALUE_KINDS64 = {"long": (_lib.NRTGPU_DOCVALUES_INT64, np.dtype(np.int64)), "double": (_lib.NRTGPU_DOCVALUES_FLOAT64, np.dtype(np.float64))}


def _value_bits64(kind: str, value) -> int:
    """The 64 bits of a doc value of the kind (an int64 / a float64)."""
    return int(np.array([value], dtype=DOC_VALUE_KINDS64[kind][1]).view(np.uint64)[0])


@dataclasses.dataclass(frozen=True)
class SortField:
    """SortField(field, Type.INT / Type.FLOAT, reverse) over a doc value column (GpuSegment.add_doc_values), with
    SortField.setMissingValue: `missing` is the value a doc without one sorts AS, whatever `reverse` is (NumberFieldDef.java:275-276
    passes MAX_VALUE / +inf for missingLast: the caller does that mapping)."""

    field: int
    kind: str = "int"
    reverse: bool = False
    missing: Union[int, float] = 0


@dataclasses.dataclass
class FieldDoc:
    """A hit of a sorted search as a searchAfter cursor: its global docid and the value it sorted as."""

    doc: int
    value: Union[int, float]


@dataclasses.dataclass
class TopFieldDocs:
    docs: np.ndarray            # int32 global docids, in the sort's order
    values: np.ndarray          # int32 / float32: the value each hit sorted as (the missing value for a doc without one)
    total_hits: int
    relation_gte: bool          # True == TotalHits.Relation.GREATER_THAN_OR_EQUAL_TO

    @property
    def value_bits(self) -> np.ndarray:
        return self.values.view(np.uint32)


class UnsupportedQuery(Exception):
    """The rewritten query is not eligible for the device route: run the CPU (Lucene) path."""


@dataclasses.dataclass
class ScoreDoc:
    doc: int
    score: float


@dataclasses.dataclass
class TopScoreDocCollectorManager:
    num_hits: int
    after: Optional[ScoreDoc] = None
    total_hits_threshold: int = TOTAL_HITS_THRESHOLD
    # Scorable.setMinCompetitiveScore fed from outside this searcher (other shards of the same search)
    min_competitive_score: float = 0.0


@dataclasses.dataclass
class TopDocs:
    docs: np.ndarray            # int32 global docids
    scores: np.ndarray          # float32
    total_hits: int
    relation_gte: bool          # True == TotalHits.Relation.GREATER_THAN_OR_EQUAL_TO


_OUT_ARRAYS = threading.local()


def _int8_rows(a, what: str) -> np.ndarray:
    """int8[n, dim], contiguous.  Anything but int8 is a TypeError: a cast would wrap -129 to 127 without a word."""
    a = np.asarray(a)
    if a.dtype != np.int8:
        raise TypeError(f"{what} of a byte vector field must be int8, got {a.dtype}")
    return np.ascontiguousarray(np.atleast_2d(a))


# the scalar fields of an array of nrtgpu_topdocs as numpy sees them: a call's capacities go in and its counts come out in one statement each
_TOPDOCS_SCALARS = np.dtype({"names": ["n_hits", "capacity", "total_hits", "total_hits_is_lower_bound"], "formats": ["<i4", "<i4", "<i8", "<i4"],
                             "offsets": [getattr(_lib.TopDocs, n).offset for n in ("n_hits", "capacity", "total_hits", "total_hits_is_lower_bound")],
                             "itemsize": C.sizeof(_lib.TopDocs)})


class _Outputs:
    """What a call that returns nq lists of up to `width` hits writes into: an array of nrtgpu_topdocs whose docs / scores pointers
    address the rows of two numpy arrays.  What it hands out (lists, topdocs) is a copy: the holder is used again."""

    def __init__(self, nq: int, width: int):
        self.outs = (_lib.TopDocs * nq)()
        self.docs = np.zeros((nq, width), dtype=np.int32)
        self.scores = np.zeros((nq, width), dtype=np.float32)
        self.outs._rows = (self.docs, self.scores)   # (what the pointers address lives as long as the array: _topdocs_outputs' callers keep only that)
        self.scalars = np.frombuffer(self.outs, dtype=_TOPDOCS_SCALARS)
        d0, s0 = self.docs.ctypes.data, self.scores.ctypes.data
        for qi in range(nq):
            self.outs[qi].docs = C.cast(d0 + qi * width * 4, C.POINTER(C.c_int32))
            self.outs[qi].scores = C.cast(s0 + qi * width * 4, C.POINTER(C.c_float))

    def begin(self, caps) -> "_Outputs":
        """Before a call: the capacity the library is told per query (one int for all, or one each; the entries differ in what they
        pass, and the library refuses some values on purpose), no hits yet."""
        self.scalars["capacity"] = caps
        self.scalars["n_hits"] = 0
        self.scalars["total_hits"] = 0
        return self

    def lists(self, none_if_negative: bool = False) -> list:
        """The call's answers as TopDocs: ONE copy of each array, a row's hits as a view of it; none_if_negative: None for a query the
        call left with total_hits < 0 (a dist search delivers only this rank's slice of the batch)."""
        dc, sc = self.docs.copy(), self.scores.copy()
        counts = (self.scalars[name].tolist() for name in ("n_hits", "total_hits", "total_hits_is_lower_bound"))
        return [None if none_if_negative and total < 0 else TopDocs(dc[qi, :m], sc[qi, :m], total, bool(lower))
                for qi, (m, total, lower) in enumerate(zip(*counts))]

    def topdocs(self, qi: int) -> TopDocs:
        o = self.outs[qi]
        return TopDocs(self.docs[qi, : o.n_hits].copy(), self.scores[qi, : o.n_hits].copy(), int(o.total_hits),
                       bool(o.total_hits_is_lower_bound))


def _outputs(nq: int, width: int, caps=None) -> _Outputs:
    """The calling thread's holder of that shape, begun (caps: _Outputs.begin; None = the width).  Built once per thread and shape and
    used again -- 2 x nq pointer objects through numpy's ctypes bridge cost 0.3 ms at 64 queries, a tenth of an exact vector search's
    pass."""
    cache = getattr(_OUT_ARRAYS, "by_shape", None)
    if cache is None:
        cache = _OUT_ARRAYS.by_shape = {}
    h = cache.get((nq, width))
    if h is None:
        if len(cache) >= 8:
            cache.clear()
        h = cache[(nq, width)] = _Outputs(nq, width)
    return h.begin(width if caps is None else caps)


def _text_outputs(n: int, managers) -> _Outputs:
    """The outputs of a text entry: max(num_hits, 1) hits per query."""
    caps = [max(int(mgr.num_hits), 1) for mgr in managers]
    return _outputs(n, max(caps, default=1), caps)


def _topdocs_outputs(nq: int, k: int):
    """(outs, docs, scores) of _outputs(nq, k), capacity k in every element: for a caller that makes the library call itself."""
    h = _outputs(nq, k)
    return h.outs, h.docs, h.scores


def _supported(rc: int) -> bool:
    """An eligibility predicate's answer: NRTGPU_OK -> True, NRTGPU_ERR_UNSUPPORTED -> False, anything else is an error."""
    if rc == _lib.NRTGPU_ERR_UNSUPPORTED:
        return False
    _lib.check(rc)
    return True


def _float_queries(queries, similarity: str, one: bool = False) -> np.ndarray:
    """float32[nq, dim] (one: float32[dim]), contiguous; unit-normalised for "normalized_cosine", which is then a dot product
    (VectorFieldDef.java:568-573).  The norm of ONE query is numpy's vector norm, the norms of a batch its reduction along the rows:
    the two may round differently, so a query may reach a single-query entry and a batch entry with other bits."""
    q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1) if one else np.ascontiguousarray(np.atleast_2d(queries), dtype=np.float32)
    if similarity == "normalized_cosine":
        norm = np.linalg.norm(q) if one else np.linalg.norm(q, axis=1, keepdims=True)
        q = np.ascontiguousarray(q / norm.astype(np.float32), dtype=np.float32)
    return q


def _request_arrays(nq: int, ks, boosts, filters, min_scores):
    """[ks, boosts, masks, min_scores] of a `*_requests` entry: one value per query each, None where the caller gave none."""
    ks = np.ascontiguousarray(ks, dtype=np.int32).reshape(-1)
    boosts = None if boosts is None else np.ascontiguousarray(boosts, dtype=np.float32).reshape(-1)
    masks = None if filters is None else np.array([int(f.mask_id) if f is not None else 0 for f in filters], dtype=np.int32)
    min_scores = None if min_scores is None else np.ascontiguousarray(min_scores, dtype=np.float32).reshape(-1)
    for name, a in (("ks", ks), ("boosts", boosts), ("filters", masks), ("min_scores", min_scores)):
        if a is not None and a.shape[0] != nq:
            raise ValueError(f"{name}: {a.shape[0]} values for {nq} queries")
    return [ks, boosts, masks, min_scores]


# ---- statistics / similarity ---------------------------------------------------------------------
@dataclasses.dataclass
class CollectionStatistics:
    doc_count: int
    sum_total_term_freq: int


class IndexStatistics:
    """Index-global statistics the searcher reads from the top-level reader."""

    def __init__(self):
        self.fields: Dict[int, CollectionStatistics] = {}
        self.doc_freq: Dict[Tuple[int, int], int] = {}

    @classmethod
    def from_corpus(cls, corpus, field: int = 0) -> "IndexStatistics":
        st = cls()
        st.fields[field] = CollectionStatistics(corpus.doc_count, corpus.sum_total_term_freq)
        for t, df in corpus.doc_freq.items():
            st.doc_freq[(field, int(t))] = int(df)
        return st


class BM25Similarity:
    """Default similarity of the reference (S/similarity/SimilarityCreator.java:33,41)."""

    def __init__(self, k1: float = 1.2, b: float = 0.75):
        self.k1, self.b = float(k1), float(b)

    def idf(self, doc_freq: int, doc_count: int) -> np.float32:
        return np.float32(_lib.load().nrtgpu_bm25_idf(int(doc_count), int(doc_freq)))

    def avgdl(self, cs: CollectionStatistics) -> np.float32:
        return np.float32(_lib.load().nrtgpu_bm25_avgdl(int(cs.sum_total_term_freq), int(cs.doc_count)))

    def norm_cache(self, cs: CollectionStatistics) -> np.ndarray:
        out = np.zeros(256, dtype=np.float32)
        _lib.load().nrtgpu_bm25_norm_cache(C.c_float(float(self.avgdl(cs))), C.c_float(self.k1), C.c_float(self.b),
                                          out.ctypes.data)
        return out

    def scorer(self, boost: float, cs: CollectionStatistics, doc_freq: int) -> Tuple[np.float32, np.ndarray]:
        """-> (weight = boost * idf, normInverse cache[256])."""
        idf = self.idf(doc_freq, cs.doc_count)
        return np.float32(np.float32(boost) * idf), self.norm_cache(cs)


# ---- device context / segment store --------------------------------------------------------------
class GpuContext:
    def __init__(self, device_id: int = 0, max_batch: int = 1024, target_items: int = 0,
                 collect_timing: bool = False, flags: int = 0, host_threads: int = 0, lookup_budget_pct: int = 0):
        L = _lib.load()
        if os.environ.get("NRTGPU_PACKED_POSTINGS", "") not in ("", "0"):   # run anything (the whole test suite) on the packed layout
            flags |= _lib.NRTGPU_FLAG_PACKED_POSTINGS
        self.flags = flags
        if lookup_budget_pct == 0 and os.environ.get("NRTGPU_TEST_LOOKUP_BUDGET_PCT"):   # run anything on another lookup budget (tests, A/B scripts)
            lookup_budget_pct = int(os.environ["NRTGPU_TEST_LOOKUP_BUDGET_PCT"])
        cfg = _lib.Config(device_id, max_batch, target_items, int(collect_timing), flags, host_threads, int(lookup_budget_pct), 0)
        h = C.c_void_p()
        _lib.check(L.nrtgpu_create(C.byref(cfg), C.byref(h)))
        self._h = h
        self.max_batch = max_batch

    def set_slicing(self, slice_max_docs: int = 250_000, slice_max_segments: int = 5, virtual_shards: int = 1) -> None:
        """MyIndexSearcher.SlicingParams of the searcher this context serves (TotalHits.relation is decided per slice)."""
        _lib.check(_lib.load().nrtgpu_set_slicing(self._h, int(slice_max_docs), int(slice_max_segments), int(virtual_shards)))

    @staticmethod
    def dist_unique_id() -> bytes:
        """An ncclUniqueId (128 bytes) for dist_init: made on one rank, handed to the others by the deployment."""
        buf = C.create_string_buffer(128)
        _lib.check(_lib.load().nrtgpu_dist_unique_id(buf))
        return bytes(buf.raw)

    def dist_init(self, world: int, rank: int, unique_id: bytes) -> None:
        """Joins the RCCL communicator of a `world`-GPU search (one process per GPU): the collective lives in the library."""
        _lib.check(_lib.load().nrtgpu_dist_init(self._h, int(world), int(rank), C.c_char_p(unique_id)))

    def dist_close(self) -> None:
        _lib.load().nrtgpu_dist_close(self._h)

    def exchange_open(self, shm_name: str, world: int, rank: int) -> None:
        """Cross-GPU bound exchange (include/nrtgpu.h); synchronise the ranks once before the first search."""
        _lib.check(_lib.load().nrtgpu_exchange_open(self._h, shm_name.encode(), int(world), int(rank)))

    def exchange_close(self) -> None:
        _lib.load().nrtgpu_exchange_close(self._h)

    def stats(self) -> dict:
        st = _lib.Stats()
        _lib.check(_lib.load().nrtgpu_get_stats(self._h, C.byref(st)))
        return {n: getattr(st, n) for n, _ in _lib.Stats._fields_}

    def scan_profile(self) -> dict:
        out = np.zeros(16, dtype=np.float64)
        _lib.check(_lib.load().nrtgpu_get_scan_profile(self._h, out.ctypes.data))
        # counters of wave 0 of every item, summed over the items since reset_stats (NRTGPU_FLAG_PROFILE)
        names = ["prologue_cycles", "rendezvous_wait_cycles", "rendezvous_cycles", "walk_cycles", "epilogue_cycles",
                 "rendezvous", "compactions", "subtiles", "rz_select_cycles", "sparse_subtiles", "rz_keep_cycles",
                 "rz_publish_append_cycles", "candidate_subtiles", "maybe_subtiles", "last_wave_finish_cycles",
                 "first_wave_finish_cycles"]
        return dict(zip(names, out.tolist()))

    def maxscore_profile(self) -> dict:
        out = np.zeros(16, dtype=np.float64)
        _lib.check(_lib.load().nrtgpu_get_maxscore_profile(self._h, out.ctypes.data))
        names = ["windows", "compactions", "chunks", "postings_streamed", "postings_surviving", "docs_evaluated", "lookups",
                 "candidates", "prologue_cycles", "item_cycles", "waves_meeting_cycles", "waves_idle_cycles", "waves_part_prologue_cycles",
                 "waves_walk_cycles", "last_wave_out_cycles", "epilogue_cycles"]
        return dict(zip(names, out.tolist()))

    def maxscore_meetings(self) -> dict:
        """The MaxScore route's meetings since reset_stats (nrtgpu_debug_maxscore_meetings; development library, NRTGPU_FLAG_PROFILE)."""
        out = np.zeros(4, dtype=np.int64)
        _lib.check(_lib.load().nrtgpu_debug_maxscore_meetings(self._h, out.ctypes.data))
        res = dict(zip(["meetings", "overflow_meetings", "compactions", "wave_estimates"], (int(x) for x in out)))
        g = np.zeros(1, dtype=np.int64)   # (guesses that raised theta in a meeting: nrtgpu_debug_maxscore_meeting_guesses)
        _lib.check(_lib.load().nrtgpu_debug_maxscore_meeting_guesses(self._h, g.ctypes.data))
        res["meeting_guesses"] = int(g[0])
        return res

    @staticmethod
    def set_thread_deadline(seconds_from_now: Optional[float]) -> None:
        """The calling thread's deadline for the search calls it makes from now on (nrtgpu_set_thread_deadline_ns): None = no deadline."""
        L = _lib.load()
        L.nrtgpu_set_thread_deadline_ns(0 if seconds_from_now is None else int(L.nrtgpu_monotonic_ns() + seconds_from_now * 1e9))

    @staticmethod
    def last_diagnostics() -> dict:
        """What the calling thread's last completed search call cost (nrtgpu_last_diagnostics)."""
        d = _lib.Diagnostics()
        _lib.check(_lib.load().nrtgpu_last_diagnostics(C.byref(d)))
        return {n: getattr(d, n) for n, _ in _lib.Diagnostics._fields_ if n != "reserved"}

    def reset_stats(self) -> None:
        _lib.load().nrtgpu_reset_stats(self._h)

    def maxscore_item_walls(self):
        """(walls[n_slots, 8] = start, end (100 MHz ticks), item, windows, round begin, CU, round, workgroup; n_items) of the last
        instrumented MaxScore launch (nrtgpu_get_maxscore_item_walls): rows >= the call's items are helper sessions."""
        L = _lib.load()
        n_items = C.c_int64(0)
        n = int(L.nrtgpu_get_maxscore_item_walls(self._h, None, 0, C.byref(n_items)))
        out = np.zeros((max(n, 0), 8), dtype=np.uint64)
        if n > 0:
            L.nrtgpu_get_maxscore_item_walls(self._h, out.ctypes.data, n, C.byref(n_items))
        return out, int(n_items.value)

    @staticmethod
    def set_thread_slices(slice_of_leaf: Optional[Sequence[int]]) -> None:
        """Partial residency (nrtgpu_set_thread_slices): the calling thread's next searches run over a SUBSET of the searcher's leaves
        and count their hits by the whole searcher's slices -- slice_of_leaf[i] = the slice of the call's i-th leaf; None clears."""
        if slice_of_leaf is None:
            _lib.check(_lib.load().nrtgpu_set_thread_slices(None, 0))
        else:
            a = np.ascontiguousarray(slice_of_leaf, dtype=np.int32)
            _lib.check(_lib.load().nrtgpu_set_thread_slices(a.ctypes.data, len(a)))

    def set_speculation(self, margin: float) -> None:
        """Speculative thresholds of the MaxScore route (nrtgpu_set_speculation): the guess's safety margin in standard deviations; 0 = off."""
        _lib.check(_lib.load().nrtgpu_set_speculation(self._h, C.c_float(float(margin))))

    def set_knn_gather(self, max_accept_permille: int) -> None:
        """The gather route of the filtered knn requests (nrtgpu_set_knn_gather): knn_search / knn_search_bytes with a filter that accepts
        at most this many thousandths of the field's rows score only the accepted rows; 0 (the default) = never.  Same results."""
        _lib.check(_lib.load().nrtgpu_set_knn_gather(self._h, int(max_accept_permille)))

    def set_shard_share(self, shard_docs: int, index_docs: int) -> None:
        """This context's share of a sharded index (nrtgpu_set_shard_share): the shard-level guesses then count the other shards'
        docs by it instead of assuming equal shards; (0, 0): equal shards."""
        _lib.check(_lib.load().nrtgpu_set_shard_share(self._h, int(shard_docs), int(index_docs)))

    def spec_counters(self) -> dict:
        """Speculative thresholds of the MaxScore route (nrtgpu_stats.spec_*): queries run under them since nrtgpu_set_speculation,
        queries run again, whether the library has switched them off for this context."""
        st = self.stats()
        return {"queries": int(st["spec_queries"]), "reruns": int(st["spec_reruns"]), "switched_off": bool(st["spec_disabled"]),
                "scattered": bool(st["spec_scattered"])}

    def debug_live_segments(self) -> int:
        """Segment handles of this context (uploads and forks) not freed yet (nrtgpu_debug_live_segments)."""
        return int(_lib.load().nrtgpu_debug_live_segments(self._h))

    def debug_hold_coalescers(self, hold: bool) -> None:
        """Test hook (nrtgpu_debug_hold_coalescers): while held, coalescer leaders leave only with a full batch / panel."""
        _lib.check(_lib.load().nrtgpu_debug_hold_coalescers(self._h, 1 if hold else 0))

    def debug_coalescer_pending(self, which: int) -> int:
        """Requests parked in a coalescer: 0 = nrtgpu_search_bm25_coalesced, 1 = nrtgpu_knn_exact_coalesced, 2 = nrtgpu_knn_search_coalesced,
        3 = nrtgpu_knn_search_bytes_coalesced, 4 = nrtgpu_knn_exact_bytes_coalesced."""
        return int(_lib.load().nrtgpu_debug_coalescer_pending(self._h, int(which)))

    def debug_dist_inject(self, step: int = -1, failed_query: int = -1) -> None:
        """Test hook (nrtgpu_debug_dist_inject): the next one-call dist search on this context fails `step`, and / or counts
        `failed_query`'s speculative guess as failed."""
        _lib.check(_lib.load().nrtgpu_debug_dist_inject(self._h, int(step), int(failed_query)))

    def close(self) -> None:
        if getattr(self, "_h", None):
            _lib.load().nrtgpu_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GpuSegment:
    """HBM-resident columnar replica of one immutable segment."""

    def __init__(self, ctx: GpuContext, max_doc: int, doc_base: int = 0):
        self.ctx, self.max_doc, self.doc_base = ctx, int(max_doc), int(doc_base)
        h = C.c_void_p()
        _lib.check(_lib.load().nrtgpu_segment_begin(ctx._h, self.max_doc, 0, C.byref(h)))
        self._h = h

    @classmethod
    def from_data(cls, ctx: GpuContext, seg, field: int = 0, omit_norms: bool = False,
                  omit_freqs: bool = False) -> "GpuSegment":
        """Upload a synth.SegmentData (what the Java side reads through PostingsEnum / norms)."""
        g = cls(ctx, seg.max_doc, seg.doc_base)
        g.add_field_norms(field, None if omit_norms else seg.norms)
        g.add_terms(field, seg.term_ids, seg.offsets, seg.docids, None if omit_freqs else seg.freqs)
        g.seal()
        if seg.live_bits is not None:
            g.set_live_docs(seg.live_bits)
        return g

    def add_field_norms(self, field: int, norms: Optional[np.ndarray]) -> None:
        p = None
        if norms is not None:
            norms = np.ascontiguousarray(norms, dtype=np.uint8)
            assert norms.shape[0] == self.max_doc
            p = norms.ctypes.data
        _lib.check(_lib.load().nrtgpu_segment_add_field_norms(self._h, int(field), p))

    def add_terms(self, field: int, term_ids, offsets, docids, freqs) -> None:
        term_ids = np.ascontiguousarray(term_ids, dtype=np.int64)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        docids = np.ascontiguousarray(docids, dtype=np.int32)
        fp = None
        if freqs is not None:
            freqs = np.ascontiguousarray(freqs, dtype=np.int32)
            fp = freqs.ctypes.data
        _lib.check(_lib.load().nrtgpu_segment_add_terms(self._h, int(field), len(term_ids), term_ids.ctypes.data,
                                                        offsets.ctypes.data, docids.ctypes.data, fp))

    def add_vectors(self, field: int, vectors: np.ndarray, ord_to_doc: Optional[np.ndarray] = None) -> None:
        vectors = np.ascontiguousarray(vectors, dtype=np.float32)
        op = None
        if ord_to_doc is not None:
            ord_to_doc = np.ascontiguousarray(ord_to_doc, dtype=np.int32)
            op = ord_to_doc.ctypes.data
        _lib.check(_lib.load().nrtgpu_segment_add_vectors(self._h, int(field), vectors.shape[1], vectors.shape[0],
                                                          op, vectors.ctypes.data))

    def add_byte_vectors(self, field: int, vectors: np.ndarray, ord_to_doc: Optional[np.ndarray] = None) -> None:
        """The rows of a byte (int8) vector field: int8[n, dim] (nrtgpu_segment_add_byte_vectors).  No silent cast."""
        vectors = _int8_rows(vectors, "vectors")
        op = None
        if ord_to_doc is not None:
            ord_to_doc = np.ascontiguousarray(ord_to_doc, dtype=np.int32)
            op = ord_to_doc.ctypes.data
        _lib.check(_lib.load().nrtgpu_segment_add_byte_vectors(self._h, int(field), vectors.shape[1], vectors.shape[0],
                                                               op, vectors.ctypes.data))

    def add_doc_values(self, field: int, kind: str, values: np.ndarray, docs: Optional[np.ndarray] = None) -> None:
        """A per-doc value column of the field (nrtgpu_segment_add_doc_values): kind "int" (int32) or "float" (float32), one value
        per listed doc (docs: ascending leaf docids; None: one value per doc of the segment).  No silent cast: the array's dtype
        must be the kind's, or uint32 for the kind's raw bits."""
        values = np.ascontiguousarray(values).reshape(-1)
        if values.dtype not in (DOC_VALUE_KINDS[kind][1], np.dtype(np.uint32)):
            raise TypeError(f"doc values of kind {kind!r} must be {DOC_VALUE_KINDS[kind][1]} (or uint32 bits), got {values.dtype}")
        dp = None
        if docs is not None:
            docs = np.ascontiguousarray(docs, dtype=np.int32).reshape(-1)
            if docs.shape[0] != values.shape[0]:
                raise ValueError(f"{docs.shape[0]} docs, {values.shape[0]} values")
            dp = docs.ctypes.data
        _lib.check(_lib.load().nrtgpu_segment_add_doc_values(self._h, int(field), DOC_VALUE_KINDS[kind][0], values.shape[0], dp,
                                                             values.ctypes.data if values.shape[0] else None))

    def add_doc_values64(self, field: int, kind: str, values: np.ndarray, docs: Optional[np.ndarray] = None) -> None:
        """A per-doc column of 64-bit values (nrtgpu_segment_add_doc_values64): kind "long" (int64: LONG, DATE_TIME as epoch
        millis) or "double" (float64); add_doc_values' contract otherwise.  No silent cast: the array's dtype must be the kind's,
        or uint64 for the kind's raw bits."""
        values = np.ascontiguousarray(values).reshape(-1)
        if values.dtype not in (DOC_VALUE_KINDS64[kind][1], np.dtype(np.uint64)):
            raise TypeError(f"doc values of kind {kind!r} must be {DOC_VALUE_KINDS64[kind][1]} (or uint64 bits), got {values.dtype}")
        dp = None
        if docs is not None:
            docs = np.ascontiguousarray(docs, dtype=np.int32).reshape(-1)
            if docs.shape[0] != values.shape[0]:
                raise ValueError(f"{docs.shape[0]} docs, {values.shape[0]} values")
            dp = docs.ctypes.data
        _lib.check(_lib.load().nrtgpu_segment_add_doc_values64(self._h, int(field), DOC_VALUE_KINDS64[kind][0], values.shape[0], dp,
                                                               values.ctypes.data if values.shape[0] else None))

    def add_doc_values_multi(self, field: int, kind: str, values: np.ndarray, value_docs: np.ndarray) -> None:
        """A multi-valued value column of the field (nrtgpu_segment_add_doc_values_multi): values[i] belongs to leaf doc
        value_docs[i] (non-decreasing; a doc listed c times has c values, duplicates count each; a doc not listed has none).
        Terms counts and doc-set range clauses read it as they read a single-valued column; a sort refuses it.  No silent cast,
        as in add_doc_values."""
        values = np.ascontiguousarray(values).reshape(-1)
        if values.dtype not in (DOC_VALUE_KINDS[kind][1], np.dtype(np.uint32)):
            raise TypeError(f"doc values of kind {kind!r} must be {DOC_VALUE_KINDS[kind][1]} (or uint32 bits), got {values.dtype}")
        value_docs = np.ascontiguousarray(value_docs, dtype=np.int32).reshape(-1)
        if value_docs.shape[0] != values.shape[0]:
            raise ValueError(f"{value_docs.shape[0]} value_docs, {values.shape[0]} values")
        n = values.shape[0]
        _lib.check(_lib.load().nrtgpu_segment_add_doc_values_multi(self._h, int(field), DOC_VALUE_KINDS[kind][0], n,
                                                                   value_docs.ctypes.data if n else None, values.ctypes.data if n else None))

    def seal(self) -> None:
        _lib.check(_lib.load().nrtgpu_segment_seal(self._h))

    def set_live_docs(self, bits: Optional[np.ndarray]) -> None:
        if bits is None:
            _lib.check(_lib.load().nrtgpu_segment_set_live_docs(self._h, None, 0))
            return
        bits = np.ascontiguousarray(bits, dtype=np.uint64)
        _lib.check(_lib.load().nrtgpu_segment_set_live_docs(self._h, bits.ctypes.data, len(bits)))

    def fork(self, live_bits: Optional[np.ndarray]) -> "GpuSegment":
        """A new reader version of this sealed segment: shares its data, carries its own liveDocs (nrtgpu_segment_fork)."""
        g = GpuSegment.__new__(GpuSegment)
        g.ctx, g.max_doc, g.doc_base = self.ctx, self.max_doc, self.doc_base
        h = C.c_void_p()
        if live_bits is None:
            _lib.check(_lib.load().nrtgpu_segment_fork(self._h, None, 0, C.byref(h)))
        else:
            live_bits = np.ascontiguousarray(live_bits, dtype=np.uint64)
            _lib.check(_lib.load().nrtgpu_segment_fork(self._h, live_bits.ctypes.data, len(live_bits), C.byref(h)))
        g._h = h
        return g

    def set_mask(self, mask_id: int, bits: Optional[np.ndarray]) -> None:
        """Doc set of a non-scoring clause (uint64 words, bit d = doc d matches); None drops it."""
        if bits is None:
            _lib.check(_lib.load().nrtgpu_segment_set_mask(self._h, int(mask_id), None, 0))
            return
        bits = np.ascontiguousarray(bits, dtype=np.uint64)
        _lib.check(_lib.load().nrtgpu_segment_set_mask(self._h, int(mask_id), bits.ctypes.data, len(bits)))

    def set_mask_from_values(self, mask_id: int, clauses: Sequence["ValueClause"]) -> int:
        """The mask of the docs that pass EVERY clause, built on the device from the segment's resident doc value columns
        (nrtgpu_segment_set_mask_from_values) and registered under mask_id as set_mask registers one -> the number of its docs.
        liveDocs are not part of it."""
        vc, keep = _marshal_value_clauses(clauses)
        count = C.c_int64(0)
        _lib.check(_lib.load().nrtgpu_segment_set_mask_from_values(self._h, int(mask_id), vc, len(clauses), C.byref(count)))
        del keep
        return int(count.value)

    def set_mask_from_values64(self, mask_id: int, clauses: Sequence["ValueClause64"]) -> int:
        """set_mask_from_values over 64-bit columns (nrtgpu_segment_set_mask_from_values64): range and exists clauses -> the number
        of docs of the registered mask."""
        n = len(clauses)
        if not 1 <= n <= _lib.NRTGPU_MAX_RANGES:
            raise ValueError(f"{n} clauses: 1..{_lib.NRTGPU_MAX_RANGES}")
        vc = (_lib.ValueClause64 * n)()
        for i, c in enumerate(clauses):
            if c.clause not in ("range", "exists"):
                raise UnsupportedQuery(f"a 64-bit value clause {c.clause!r}")
            vc[i] = _lib.ValueClause64(_VALUE_CLAUSE_KINDS[c.clause], int(c.field), int(c.lower_bits), int(c.upper_bits), 0)
        count = C.c_int64(0)
        _lib.check(_lib.load().nrtgpu_segment_set_mask_from_values64(self._h, int(mask_id), vc, n, C.byref(count)))
        return int(count.value)

    def get_mask(self, mask_id: int) -> np.ndarray:
        """The uint64 words of a registered mask, however it was set (nrtgpu_segment_get_mask)."""
        bits = np.zeros((self.max_doc + 63) // 64, dtype=np.uint64)
        _lib.check(_lib.load().nrtgpu_segment_get_mask(self._h, int(mask_id), bits.ctypes.data, len(bits)))
        return bits

    @property
    def device_bytes(self) -> int:
        return int(_lib.load().nrtgpu_segment_device_bytes(self._h))

    def debug_term_lookup(self, field: int, term_id: int) -> Tuple[int, int, int]:
        """Test hook of the development library (nrtgpu_debug_term_lookup): (kind, log2 docs per lookup cell, bytes) of the doc ->
        posting lookup structure the seal gave the term: kind 0 none, 1 records per 32 docs, 2 lookup cells."""
        kind, shift, nbytes = C.c_int32(-1), C.c_int32(-1), C.c_int64(-1)
        _lib.check(_lib.load().nrtgpu_debug_term_lookup(self._h, int(field), int(term_id), C.byref(kind), C.byref(shift), C.byref(nbytes)))
        return int(kind.value), int(shift.value), int(nbytes.value)

    def release(self) -> None:
        if getattr(self, "_h", None):
            _lib.load().nrtgpu_segment_release(self._h)
            self._h = None


# ---- searcher ------------------------------------------------------------------------------------
def _unsupported(msg: str):
    raise UnsupportedQuery(msg)


def _flatten(query: Query) -> Tuple[List[Tuple[int, int, float, int]], int, List[int], List[int], int, float]:
    """Eligibility predicate of SURVEY 8b on the rewritten query -> [(field, term, boost, occur: 0 SHOULD / 1 MUST)], msm,
    filter mask ids, must_not mask ids (any number of FILTER / MUST_NOT clauses: the library combines their masks at plan
    time), disjunction_max (1: best clause + tie breaker x the others instead of the sum), tie breaker."""
    def one(q, occur: int = 0) -> Tuple[int, int, float, int]:
        if isinstance(q, TermQuery):
            return (q.field, q.term, 1.0, occur)
        if isinstance(q, BoostQuery) and isinstance(q.query, TermQuery):
            return (q.query.field, q.query.term, float(q.boost), occur)
        raise UnsupportedQuery(f"clause {q!r} is not a (boosted) TermQuery")

    def dismax(q: DisjunctionMaxQuery):
        if not 0.0 <= q.tie_breaker_multiplier <= 1.0:
            raise UnsupportedQuery("DisjunctionMaxQuery with a tie breaker outside [0, 1]")
        if not q.disjuncts:
            raise UnsupportedQuery("empty DisjunctionMaxQuery")
        return [one(c) for c in q.disjuncts]

    def masks(q: BooleanQuery) -> Tuple[List[int], List[int]]:
        if any(not isinstance(c, MaskFilter) or c.mask_id <= 0 for c in q.filter + q.must_not):
            raise UnsupportedQuery("FILTER / MUST_NOT clauses must be resident masks")
        if len(q.filter) > _lib.NRTGPU_MAX_MASKS or len(q.must_not) > _lib.NRTGPU_MAX_MASKS:
            raise UnsupportedQuery(f"more than {_lib.NRTGPU_MAX_MASKS} FILTER or MUST_NOT clauses")
        return [c.mask_id for c in q.filter], [c.mask_id for c in q.must_not]

    if isinstance(query, DisjunctionMaxQuery):
        return dismax(query), 0, [], [], 1, float(query.tie_breaker_multiplier)
    if isinstance(query, BooleanQuery) and len(query.must) == 1 and isinstance(query.must[0], DisjunctionMaxQuery):
        # "+dismax #filter -must_not": one scoring clause, the masks add nothing to the score
        if query.should:
            raise UnsupportedQuery("a DisjunctionMaxQuery next to SHOULD clauses")
        f, mn = masks(query)
        return dismax(query.must[0]), 0, f, mn, 1, float(query.must[0].tie_breaker_multiplier)
    if isinstance(query, BooleanQuery):
        f, mn = masks(query)
        if query.must:
            # a conjunction of term clauses matches the docs all of them match and sums all their scores
            # (ConjunctionScorer: double sum, one cast): the disjunction with minimumNumberShouldMatch = n
            if query.should:
                # ReqOptSumScorer returns (float)required + (float)optional -- two separately rounded sums added in float
                # [Lucene-recall]: the clauses carry their occur, the kernel a second accumulator (plan.h: kMsSecReqOpt)
                if query.minimum_number_should_match > 0:   # (Lucene then scores the SHOULD part as one more required scorer)
                    raise UnsupportedQuery("MUST clauses next to minimumNumberShouldMatch > 0")
                return [one(c, 1) for c in query.must] + [one(c, 0) for c in query.should], 0, f, mn, 0, 0.0
            return [one(c) for c in query.must], len(query.must), f, mn, 0, 0.0
        if not query.should:
            raise UnsupportedQuery("empty BooleanQuery")
        if query.filter and query.minimum_number_should_match < 1:
            # with a FILTER clause Lucene makes the SHOULD clauses optional: filter-only docs would be hits of score 0
            raise UnsupportedQuery("FILTER with minimumNumberShouldMatch = 0")
        return [one(c) for c in query.should], query.minimum_number_should_match, f, mn, 0, 0.0
    return [one(query)], 0, [], [], 0, 0.0


class _Marshalled:
    """Keeps the ctypes arrays of a batch alive for the duration of the call."""

    def __init__(self, n: int):
        self.queries = (_lib.Bm25Query * n)()
        self.keep: list = []


class GpuIndexSearcher:
    """IndexSearcher over GPU-resident leaves: search(query, collectorManager) -> TopDocs."""

    def __init__(self, ctx: GpuContext, leaves: Sequence[GpuSegment], stats: IndexStatistics,
                 similarity: Optional[BM25Similarity] = None):
        self.ctx, self.leaves, self.stats = ctx, list(leaves), stats
        self.similarity = similarity or BM25Similarity()
        n = len(self.leaves)
        self._segs = (C.c_void_p * max(n, 1))(*[l._h for l in self.leaves])
        self._bases = (C.c_int32 * max(n, 1))(*[l.doc_base for l in self.leaves])
        self._cache_memo: Dict[int, np.ndarray] = {}

    def _norm_cache(self, field: int) -> np.ndarray:
        c = self._cache_memo.get(field)
        if c is None:
            c = self.similarity.norm_cache(self.stats.fields[field])
            self._cache_memo[field] = c
        return c

    def _marshal(self, queries: Sequence[Query], managers: Sequence[TopScoreDocCollectorManager]) -> _Marshalled:
        m = _Marshalled(len(queries))
        for qi, (query, mgr) in enumerate(zip(queries, managers)):
            clauses, msm, filters, must_nots, dis_max, tie_breaker = _flatten(query)
            fields: List[int] = []
            terms = (_lib.Term * len(clauses))()
            for ti, (field, term, boost, occur) in enumerate(clauses):
                if field not in self.stats.fields:
                    raise UnsupportedQuery(f"no statistics for field {field}")
                if field not in fields:
                    fields.append(field)
                df = self.stats.doc_freq.get((field, term), 0)
                cs = self.stats.fields[field]
                w = np.float32(np.float32(boost) * self.similarity.idf(df, cs.doc_count)) if df > 0 else np.float32(0)
                terms[ti] = _lib.Term(field, fields.index(field), term, float(w), int(occur))
            cache = np.concatenate([self._norm_cache(f) for f in fields]).astype(np.float32)
            m.keep += [terms, cache]
            q = m.queries[qi]
            q.n_terms = len(clauses)
            q.terms = terms
            q.n_caches = len(fields)
            q.norm_cache = cache.ctypes.data_as(C.POINTER(C.c_float))
            q.k = int(mgr.num_hits)
            q.total_hits_threshold = int(mgr.total_hits_threshold)
            q.has_after = int(mgr.after is not None)
            q.after_doc = int(mgr.after.doc) if mgr.after is not None else 0
            q.after_score = float(mgr.after.score) if mgr.after is not None else 0.0
            q.min_should_match = int(msm)
            q.min_competitive_score = float(mgr.min_competitive_score)
            q.filter_mask = int(filters[0]) if filters else 0
            q.must_not_mask = int(must_nots[0]) if must_nots else 0
            q.disjunction_max = int(dis_max)
            q.tie_breaker = float(np.float32(tie_breaker))
            for ids, n_name, p_name in ((filters[1:], "n_more_filters", "more_filters"), (must_nots[1:], "n_more_must_not", "more_must_not")):
                if ids:   # further FILTER / MUST_NOT clauses: the library ANDs / AND-NOTs their masks at plan time
                    arr = (C.c_int32 * len(ids))(*[int(x) for x in ids])
                    m.keep.append(arr)
                    setattr(q, n_name, len(ids))
                    setattr(q, p_name, arr)
        return m

    def _run_text(self, entry: str, m: _Marshalled, managers: Sequence[TopScoreDocCollectorManager], *records) -> List[TopDocs]:
        """A text route's batch entry: entry(ctx, segs, bases, n_segs, queries, *the route's records per query, n, outs)."""
        n = len(m.queries)
        h = _text_outputs(n, managers)
        _lib.check(getattr(_lib.load(), entry)(self.ctx._h, self._segs, self._bases, len(self.leaves), m.queries, *records, n, h.outs))
        return h.lists()

    def search_batch(self, queries: Sequence[Query], managers: Sequence[TopScoreDocCollectorManager]) -> List[TopDocs]:
        return self._run_text("nrtgpu_search_bm25_batch", self._marshal(queries, managers), managers)

    def search(self, query: Query, manager: TopScoreDocCollectorManager) -> TopDocs:
        return self.search_batch([query], [manager])[0]

    def _marshal_function_scores(self, queries: Sequence[FunctionScoreQuery], m: _Marshalled):
        """nrtgpu_function_score per query; the ctypes arrays stay alive in m.keep."""
        fs = (_lib.FunctionScore * len(queries))()
        for qi, query in enumerate(queries):
            if query.score_mode not in SCORE_MODES or query.boost_mode not in BOOST_MODES:
                raise UnsupportedQuery(f"score_mode {query.score_mode!r} / boost_mode {query.boost_mode!r}")
            funcs = (_lib.ScoreFunction * max(len(query.functions), 1))()
            for i, f in enumerate(query.functions):
                funcs[i] = _lib.ScoreFunction(int(f.mask_id), float(np.float32(f.weight)))
            m.keep.append(funcs)
            fs[qi].n_functions = len(query.functions)
            fs[qi].functions = funcs
            fs[qi].score_mode = SCORE_MODES[query.score_mode]
            fs[qi].boost_mode = BOOST_MODES[query.boost_mode]
            fs[qi].min_score = float(np.float32(query.min_score))
            fs[qi].min_excluded = int(bool(query.min_excluded))
        m.keep.append(fs)
        return fs

    def search_function_score_batch(self, queries: Sequence[FunctionScoreQuery],
                                    managers: Sequence[TopScoreDocCollectorManager]) -> List[TopDocs]:
        """MultiFunctionScoreQuery searches (nrtgpu_search_function_score_batch): every live doc matching the inner query is
        scored, total_hits is exact."""
        m = self._marshal([q.inner for q in queries], managers)
        return self._run_text("nrtgpu_search_function_score_batch", m, managers, self._marshal_function_scores(queries, m))

    def function_score_supported(self, query: FunctionScoreQuery, manager: TopScoreDocCollectorManager) -> bool:
        """The eligibility predicate alone (nrtgpu_function_score_supported)."""
        m = self._marshal([query.inner], [manager])
        fs = self._marshal_function_scores([query], m)
        return _supported(_lib.load().nrtgpu_function_score_supported(self.ctx._h, self._segs, len(self.leaves), m.queries, fs))

    def _marshal_knn_clauses(self, knn_clauses: Sequence[Sequence[KnnClause]], m: _Marshalled):
        """nrtgpu_knn_clauses per query; the form by BooleanQuery.rewrite's rule: a text query with FILTER / MUST_NOT clauses is no
        pure disjunction and stays ONE clause (NESTED), anything else this route takes is inlined (FLAT)."""
        kc = (_lib.KnnClauses * len(knn_clauses))()
        for qi, clauses in enumerate(knn_clauses):
            lists = (_lib.DocScores * max(len(clauses), 1))()
            for li, c in enumerate(clauses):
                docs = np.ascontiguousarray(c.docs, dtype=np.int32).reshape(-1)
                scores = np.ascontiguousarray(c.scores, dtype=np.float32).reshape(-1)
                if docs.shape[0] != scores.shape[0]:
                    raise ValueError(f"query {qi} knn clause {li}: {docs.shape[0]} docs, {scores.shape[0]} scores")
                m.keep += [docs, scores]
                lists[li] = _lib.DocScores(docs.ctypes.data_as(C.POINTER(C.c_int32)), scores.ctypes.data_as(C.POINTER(C.c_float)),
                                           docs.shape[0], float(np.float32(c.boost)))
            m.keep.append(lists)
            q = m.queries[qi]
            kc[qi].lists = lists
            kc[qi].n_lists = len(clauses)
            kc[qi].text_nested = int(q.filter_mask != 0 or q.must_not_mask != 0 or q.n_more_filters != 0 or q.n_more_must_not != 0)
        m.keep.append(kc)
        return kc

    def search_text_knn_batch(self, queries: Sequence[Query], knn_clauses: Sequence[Sequence[KnnClause]],
                              managers: Sequence[TopScoreDocCollectorManager]) -> List[TopDocs]:
        """Requests with `query` AND `knn` (nrtgpu_search_text_knn_batch): knn_clauses[i], the resolved knn lists of request i, are
        further SHOULD clauses beside queries[i] in one BooleanQuery.  Every hit is scored, total_hits is exact."""
        if len(knn_clauses) != len(queries):
            raise ValueError(f"{len(knn_clauses)} knn clause lists for {len(queries)} queries")
        m = self._marshal(queries, managers)
        return self._run_text("nrtgpu_search_text_knn_batch", m, managers, self._marshal_knn_clauses(knn_clauses, m))

    def text_knn_supported(self, query: Query, knn_clauses: Sequence[KnnClause], manager: TopScoreDocCollectorManager) -> bool:
        """The eligibility predicate alone (nrtgpu_text_knn_supported)."""
        m = self._marshal([query], [manager])
        kc = self._marshal_knn_clauses([knn_clauses], m)
        return _supported(_lib.load().nrtgpu_text_knn_supported(self.ctx._h, self._segs, len(self.leaves), m.queries, kc))

    def search_with_knn(self, query: Query, manager: TopScoreDocCollectorManager, knn: Sequence[tuple] = ()) -> TopDocs:
        """The request as a caller writes it: `query` and knn = [(field, similarity, vector, k, boost, accept)], accept a MaskFilter
        or None.  The knn clauses are resolved first, in shared passes per (field, similarity) (knn_search_requests; the scores come
        back with the boost applied), and their lists go beside the text query (search_text_knn_batch)."""
        clauses: List[Optional[KnnClause]] = [None] * len(knn)
        groups: Dict[Tuple[int, str, int], List[int]] = {}
        for i, (field, similarity, vector, _k, _boost, _accept) in enumerate(knn):
            groups.setdefault((int(field), similarity, int(np.asarray(vector).reshape(-1).shape[0])), []).append(i)
        for (field, similarity, _dim), idx in groups.items():
            res = self.knn_search_requests(field, similarity, np.stack([np.asarray(knn[i][2], dtype=np.float32).reshape(-1) for i in idx]),
                                           [int(knn[i][3]) for i in idx], boosts=[float(knn[i][4]) for i in idx],
                                           filters=[knn[i][5] for i in idx])
            for i, td in zip(idx, res):
                clauses[i] = KnnClause(td.docs, td.scores, 1.0)
        return self.search_text_knn_batch([query], [clauses], [manager])[0]

    def _marshal_multi_match(self, queries: Sequence[MultiMatchQuery], managers: Sequence[TopScoreDocCollectorManager]):
        """(nrtgpu_bm25_query array holder, nrtgpu_clause_groups array): the clauses of all groups in group order."""
        flat = []
        for query in queries:
            if query.shape not in GROUP_SHAPES or query.operator not in ("should", "must"):
                raise UnsupportedQuery(f"shape {query.shape!r} / operator {query.operator!r}")
            if not query.groups or any(len(g) == 0 for g in query.groups):
                raise UnsupportedQuery("a multi-match query without groups, or with an empty group")
            if len(query.groups) > _lib.NRTGPU_MAX_GROUPS:
                raise UnsupportedQuery(f"more than {_lib.NRTGPU_MAX_GROUPS} groups")
            # (minimumNumberShouldMatch = 1 only lets _flatten take the FILTER clauses; the real minima are set below)
            flat.append(BooleanQuery(tuple(c for g in query.groups for c in g), 1, query.filter, query.must_not))
        m = self._marshal(flat, managers)
        gs = (_lib.ClauseGroups * len(queries))()
        for qi, query in enumerate(queries):
            best = query.shape == "best_fields"
            must = query.operator == "must"
            msm = query.minimum_number_should_match
            of = (C.c_int32 * m.queries[qi].n_terms)(*[gi for gi, g in enumerate(query.groups) for _ in g])
            m.keep.append(of)
            gs[qi].shape = GROUP_SHAPES[query.shape]
            gs[qi].n_groups = len(query.groups)
            gs[qi].group_of_term = of
            gs[qi].tie_breaker = float(np.float32(query.tie_breaker_multiplier))
            gs[qi].group_occur = int(must and not best)
            m.queries[qi].min_should_match = 0
            if best:
                for t in range(m.queries[qi].n_terms):
                    m.queries[qi].terms[t].occur = int(must)
                if not must:
                    per = tuple(msm) if isinstance(msm, (tuple, list)) else (int(msm),) * len(query.groups)
                    if len(per) != len(query.groups):
                        raise UnsupportedQuery("minimum_number_should_match: one entry per group")
                    mins = (C.c_int32 * len(per))(*[int(x) for x in per])
                    m.keep.append(mins)
                    gs[qi].group_min_should_match = mins
            elif not must:
                if isinstance(msm, (tuple, list)):
                    raise UnsupportedQuery("cross_fields takes one minimum_number_should_match")
                m.queries[qi].min_should_match = int(msm)
        m.keep.append(gs)
        return m, gs

    def search_multi_match_batch(self, queries: Sequence[MultiMatchQuery], managers: Sequence[TopScoreDocCollectorManager]) -> List[TopDocs]:
        """Multi-match searches (nrtgpu_search_multi_match_batch): every live doc that is a hit is scored, total_hits is exact."""
        m, gs = self._marshal_multi_match(queries, managers)
        return self._run_text("nrtgpu_search_multi_match_batch", m, managers, gs)

    def multi_match_supported(self, query: MultiMatchQuery, manager: TopScoreDocCollectorManager) -> bool:
        """The eligibility predicate alone (nrtgpu_multi_match_supported)."""
        m, gs = self._marshal_multi_match([query], [manager])
        return _supported(_lib.load().nrtgpu_multi_match_supported(self.ctx._h, self._segs, len(self.leaves), m.queries, gs))

    def _marshal_function_score_multi_match(self, queries: Sequence[FunctionScoreQuery], managers: Sequence[TopScoreDocCollectorManager]):
        """(nrtgpu_bm25_query array holder, nrtgpu_clause_groups array, nrtgpu_function_score array) of function scores whose
        inner query is a MultiMatchQuery."""
        for query in queries:
            if not isinstance(query.inner, MultiMatchQuery):
                raise UnsupportedQuery("the inner query is not a MultiMatchQuery (search_function_score_batch takes flat inner queries)")
        m, gs = self._marshal_multi_match([q.inner for q in queries], managers)
        return m, gs, self._marshal_function_scores(queries, m)

    def search_function_score_multi_match_batch(self, queries: Sequence[FunctionScoreQuery],
                                                managers: Sequence[TopScoreDocCollectorManager]) -> List[TopDocs]:
        """MultiFunctionScoreQuery over MultiMatchQuery searches (nrtgpu_search_function_score_multi_match_batch): every live doc
        that is a hit of the inner query and passes the min_score test is scored, total_hits is exact."""
        m, gs, fs = self._marshal_function_score_multi_match(queries, managers)
        return self._run_text("nrtgpu_search_function_score_multi_match_batch", m, managers, gs, fs)

    def function_score_multi_match_supported(self, query: FunctionScoreQuery, manager: TopScoreDocCollectorManager) -> bool:
        """The eligibility predicate alone (nrtgpu_function_score_multi_match_supported)."""
        m, gs, fs = self._marshal_function_score_multi_match([query], [manager])
        return _supported(_lib.load().nrtgpu_function_score_multi_match_supported(self.ctx._h, self._segs, len(self.leaves), m.queries, gs, fs))

    def debug_walk_rows(self, queries: Sequence[Query], managers: Sequence[TopScoreDocCollectorManager]):
        """Test hook of the development library (nrtgpu_debug_walk_rows): the MaxScore route's walk rows of the batch, as the
        plan expansion writes them on the device (nothing is searched).  -> (begin[n_queries, n_leaves] (-1: none),
        count[n_queries, n_leaves], rows: a structured array with the fields suffix (S_c), ub, weight, fx_scale, flags, u_after and
        the four device addresses)."""
        n, nl = len(queries), len(self.leaves)
        m = self._marshal(queries, managers)
        begin = np.full((n, nl), -1, dtype=np.int32)
        count = np.zeros((n, nl), dtype=np.int32)
        L = _lib.load()
        total = int(L.nrtgpu_debug_walk_rows(self.ctx._h, self._segs, self._bases, nl, m.queries, n, begin.ctypes.data, count.ctypes.data, None, 0))
        if total < 0:
            _lib.check(-total)
        rows = np.zeros(max(total, 1), dtype=WALK_ROW_DTYPE)
        got = int(L.nrtgpu_debug_walk_rows(self.ctx._h, self._segs, self._bases, nl, m.queries, n, begin.ctypes.data, count.ctypes.data,
                                           rows.ctypes.data, total))
        if got < 0:
            _lib.check(-got)
        return begin, count, rows[:total]

    def dist_search_batch(self, queries: Sequence[Query], managers: Sequence[TopScoreDocCollectorManager],
                          mode: int = EXCHANGE_ALLGATHER) -> List[Optional[TopDocs]]:
        """The multi-GPU search through nrtgpu_dist_search_bm25_batch_mode: this rank's leaves, RCCL exchange + merge inside
        the library (GpuContext.dist_init first).  EXCHANGE_ALLGATHER: every rank gets every answer; EXCHANGE_ALLTOALL: this
        rank gets the answers of its slice of the batch, None for the others."""
        n = len(queries)
        m = self._marshal(queries, managers)
        h = _text_outputs(n, managers)
        _lib.check(_lib.load().nrtgpu_dist_search_bm25_batch_mode(self.ctx._h, self._segs, self._bases, len(self.leaves), m.queries, n,
                                                                  int(mode), h.outs))
        return h.lists(none_if_negative=True)

    def dist_knn_exact(self, field: int, similarity: str, queries: np.ndarray, k: int, boost: float = 1.0,
                       mode: int = EXCHANGE_ALLGATHER) -> List[Optional[TopDocs]]:
        """Exact vector search over a row-partitioned field (nrtgpu_dist_knn_exact): this rank's leaves, exchange + merge
        inside the library; every rank passes the same queries."""
        return self._knn_batch("nrtgpu_dist_knn_exact", field, self.SIMILARITY[similarity], _float_queries(queries, similarity), k,
                               C.c_float(boost), int(mode), none_if_negative=True)

    def supported(self, query: Query, manager: TopScoreDocCollectorManager) -> bool:
        """The eligibility predicate alone (nrtgpu_query_supported): would the device route take this query?"""
        m = self._marshal([query], [manager])
        return _supported(_lib.load().nrtgpu_query_supported(self.ctx._h, self._segs, len(self.leaves), m.queries))

    def search_coalesced(self, query: Query, manager: TopScoreDocCollectorManager) -> TopDocs:
        """Blocking single search meant to be called from many threads at once: the library merges
        concurrent callers into device batches (nrtgpu_search_bm25_coalesced)."""
        m = self._marshal([query], [manager])
        h = _text_outputs(1, [manager])
        _lib.check(_lib.load().nrtgpu_search_bm25_coalesced(self.ctx._h, self._segs, self._bases, len(self.leaves), m.queries, h.outs))
        return h.topdocs(0)

    # ---- vectors: ExactFloatVectorQuery / vector rescorer ------------------------------------------
    SIMILARITY = {"cosine": 0, "dot_product": 1, "normalized_cosine": 1, "l2_norm": 2, "max_inner_product": 3}

    def _knn_batch(self, entry: str, field: int, sim: int, queries: np.ndarray, k: int, *tail, none_if_negative: bool = False) -> list:
        """A batch of vector queries with one k through entry(ctx, segs, bases, n_segs, field, sim, queries, nq, dim, k, *tail, outs)."""
        nq, dim = queries.shape
        h = _outputs(nq, int(k))
        _lib.check(getattr(_lib.load(), entry)(self.ctx._h, self._segs, self._bases, len(self.leaves), int(field), sim, queries.ctypes.data,
                                               nq, dim, int(k), *tail, h.outs))
        return h.lists(none_if_negative)

    def _knn_requests(self, entry: str, field: int, sim: int, queries: np.ndarray, ks, boosts, filters, min_scores) -> List[TopDocs]:
        """Vector queries with a k, boost, filter and threshold each through a `*_requests` entry."""
        nq, dim = queries.shape
        ks, *optional = _request_arrays(nq, ks, boosts, filters, min_scores)
        h = _outputs(nq, max(int(ks.max()), 1))
        _lib.check(getattr(_lib.load(), entry)(self.ctx._h, self._segs, self._bases, len(self.leaves), int(field), sim, queries.ctypes.data,
                                               nq, dim, ks.ctypes.data, *(None if a is None else a.ctypes.data for a in optional), h.outs))
        return h.lists()

    def _one_knn_query(self, entry: str, field: int, sim: int, query: np.ndarray, k: int, cap: int, *tail) -> TopDocs:
        """One query vector through a single-query (coalesced) entry; cap: the capacity the entry is told, tail: its scalars between
        k and the output."""
        h = _outputs(1, cap)
        _lib.check(getattr(_lib.load(), entry)(self.ctx._h, self._segs, self._bases, len(self.leaves), int(field), sim, query.ctypes.data,
                                               int(query.shape[0]), int(k), *tail, h.outs))
        return h.topdocs(0)

    def knn_exact(self, field: int, similarity: str, queries: np.ndarray, k: int, boost: float = 1.0) -> List[TopDocs]:
        """Brute-force exact vector search over every doc with a vector (S/query/vector/ExactVectorQuery.java)."""
        return self._knn_batch("nrtgpu_knn_exact", field, self.SIMILARITY[similarity], _float_queries(queries, similarity), k, C.c_float(boost))

    def knn_exact_coalesced(self, field: int, similarity: str, query: np.ndarray, k: int, boost: float = 1.0) -> TopDocs:
        """What a request thread calls with ONE exact vector query: concurrent callers are merged into panels of up to 64 queries
        that share a pass over the rows (nrtgpu_knn_exact_coalesced)."""
        return self._one_knn_query("nrtgpu_knn_exact_coalesced", field, self.SIMILARITY[similarity], _float_queries(query, similarity, one=True),
                                   k, int(k), C.c_float(boost))

    def knn_exact_relation(self, field: int, k: int, total_hits_threshold: int = TOTAL_HITS_THRESHOLD) -> bool:
        """TotalHits.relation of an exact vector query over these leaves by the reference's per-slice rule: True = GREATER_THAN_OR_EQUAL_TO
        (nrtgpu_knn_exact_relation; host only)."""
        rc = _lib.load().nrtgpu_knn_exact_relation(self.ctx._h, self._segs, self._bases, len(self.leaves), int(field), int(k), int(total_hits_threshold))
        if rc < 0:
            _lib.check(rc)
        return bool(rc)

    def knn_search(self, field: int, similarity: str, queries: np.ndarray, k: int, boost: float = 1.0,
                   filter: Optional[MaskFilter] = None, min_score: float = 0.0) -> List[TopDocs]:
        """The `knn` request path (KnnQuery with filter and similarity threshold) answered by exact search."""
        return self._knn_batch("nrtgpu_knn_search", field, self.SIMILARITY[similarity], _float_queries(queries, similarity), k, C.c_float(boost),
                               int(filter.mask_id) if filter else 0, C.c_float(min_score))

    def knn_search_requests(self, field: int, similarity: str, queries: np.ndarray, ks: Sequence[int], boosts: Optional[Sequence[float]] = None,
                            filters: Optional[Sequence[Optional[MaskFilter]]] = None,
                            min_scores: Optional[Sequence[float]] = None) -> List[TopDocs]:
        """`knn` requests with a k, boost, filter and threshold EACH, answered in passes of up to 64 that share one read of the rows
        (nrtgpu_knn_search_requests): query i gets what knn_search gives it alone."""
        return self._knn_requests("nrtgpu_knn_search_requests", field, self.SIMILARITY[similarity], _float_queries(queries, similarity),
                                  ks, boosts, filters, min_scores)

    def knn_search_coalesced(self, field: int, similarity: str, query: np.ndarray, k: int, boost: float = 1.0,
                             filter: Optional[MaskFilter] = None, min_score: float = 0.0) -> TopDocs:
        """What a request thread calls with ONE `knn` request: concurrent callers share panels of up to 64 whatever their k, filter,
        threshold and boost (nrtgpu_knn_search_coalesced)."""
        return self._one_knn_query("nrtgpu_knn_search_coalesced", field, self.SIMILARITY[similarity], _float_queries(query, similarity, one=True),
                                   k, max(int(k), 1), C.c_float(boost), int(filter.mask_id) if filter else 0, C.c_float(min_score))

    # ---- byte (int8) vector fields: ExactByteVectorQuery / NrtKnnByteVectorQuery ---------------------
    BYTE_SIMILARITY = {"cosine": 0, "dot_product": 1, "l2_norm": 2, "max_inner_product": 3}

    def _byte_similarity(self, similarity: str) -> int:
        if similarity not in self.BYTE_SIMILARITY:   # ("normalized_cosine" does not exist for byte fields: VectorFieldDef.java:698-701)
            raise ValueError(f"similarity {similarity!r} is not defined for byte vector fields")
        return self.BYTE_SIMILARITY[similarity]

    def knn_exact_bytes(self, field: int, similarity: str, queries: np.ndarray, k: int, boost: float = 1.0) -> List[TopDocs]:
        """Brute-force exact search over a byte vector field (ExactVectorQuery.ExactByteVectorQuery); queries: int8."""
        return self._knn_batch("nrtgpu_knn_exact_bytes", field, self._byte_similarity(similarity), _int8_rows(queries, "queries"), k, C.c_float(boost))

    def knn_search_bytes(self, field: int, similarity: str, queries: np.ndarray, k: int, boost: float = 1.0,
                         filter: Optional[MaskFilter] = None, min_score: float = 0.0) -> List[TopDocs]:
        """The `knn` request path over a byte vector field (NrtKnnByteVectorQuery with filter and similarity threshold), exact."""
        return self._knn_batch("nrtgpu_knn_search_bytes", field, self._byte_similarity(similarity), _int8_rows(queries, "queries"), k, C.c_float(boost),
                               int(filter.mask_id) if filter else 0, C.c_float(min_score))

    def knn_search_bytes_requests(self, field: int, similarity: str, queries: np.ndarray, ks: Sequence[int],
                                  boosts: Optional[Sequence[float]] = None, filters: Optional[Sequence[Optional[MaskFilter]]] = None,
                                  min_scores: Optional[Sequence[float]] = None) -> List[TopDocs]:
        """`knn` requests over a byte vector field with a k, boost, filter and threshold EACH, answered in passes of up to 64 that share
        one read of the rows (nrtgpu_knn_search_bytes_requests): query i gets what knn_search_bytes gives it alone."""
        return self._knn_requests("nrtgpu_knn_search_bytes_requests", field, self._byte_similarity(similarity), _int8_rows(queries, "queries"),
                                  ks, boosts, filters, min_scores)

    def knn_search_bytes_coalesced(self, field: int, similarity: str, query: np.ndarray, k: int, boost: float = 1.0,
                                   filter: Optional[MaskFilter] = None, min_score: float = 0.0) -> TopDocs:
        """What a request thread calls with ONE `knn` request over a byte vector field: concurrent callers share panels of up to 64
        whatever their k, filter, threshold and boost (nrtgpu_knn_search_bytes_coalesced)."""
        return self._one_knn_query("nrtgpu_knn_search_bytes_coalesced", field, self._byte_similarity(similarity), _int8_rows(query, "query").reshape(-1),
                                   k, max(int(k), 1), C.c_float(boost), int(filter.mask_id) if filter else 0, C.c_float(min_score))

    def knn_exact_bytes_coalesced(self, field: int, similarity: str, query: np.ndarray, k: int, boost: float = 1.0) -> TopDocs:
        """What a request thread calls with ONE exact query over a byte vector field: concurrent callers with one boost are merged into
        panels of up to 64 queries that share a pass over the rows (nrtgpu_knn_exact_bytes_coalesced)."""
        return self._one_knn_query("nrtgpu_knn_exact_bytes_coalesced", field, self._byte_similarity(similarity), _int8_rows(query, "query").reshape(-1),
                                   k, max(int(k), 1), C.c_float(boost))

    def rescore_vectors(self, hits: TopDocs, field: int, similarity: str, query: np.ndarray, window: int,
                        query_weight: float = 1.0, rescore_weight: float = 1.0, boost: float = 1.0) -> TopDocs:
        """RescoreOperation.rescore with a QueryRescore whose rescoreQuery is an exact vector query
        (S/rescore/QueryRescore.java:40-57)."""
        return self._rescore("nrtgpu_rescore_vectors", hits, field, self.SIMILARITY[similarity],
                             np.ascontiguousarray(query, dtype=np.float32), window, query_weight, rescore_weight, boost)

    def rescore_byte_vectors(self, hits: TopDocs, field: int, similarity: str, query: np.ndarray, window: int,
                             query_weight: float = 1.0, rescore_weight: float = 1.0, boost: float = 1.0) -> TopDocs:
        """The same over a byte vector field (the rescoreQuery is an ExactByteVectorQuery); query: int8."""
        sim = self._byte_similarity(similarity)
        query = _int8_rows(query, "query")
        if query.shape[0] != 1:
            raise ValueError("one query vector")
        return self._rescore("nrtgpu_rescore_byte_vectors", hits, field, sim, query[0], window, query_weight, rescore_weight, boost)

    def _rescore(self, entry: str, hits: TopDocs, field: int, sim: int, query: np.ndarray, window: int, query_weight: float,
                 rescore_weight: float, boost: float) -> TopDocs:
        d = np.ascontiguousarray(hits.docs, dtype=np.int32)
        s = np.ascontiguousarray(hits.scores, dtype=np.float32)
        h = _outputs(1, max(int(window), 1), int(window))
        _lib.check(getattr(_lib.load(), entry)(self.ctx._h, self._segs, self._bases, len(self.leaves), int(field), sim,
                                               query.ctypes.data, len(query), C.c_float(boost), d.ctypes.data, s.ctypes.data, len(d),
                                               float(query_weight), float(rescore_weight), int(window), h.outs))
        got = h.topdocs(0)
        return TopDocs(got.docs, got.scores, hits.total_hits, hits.relation_gte)

    def search_hybrid_batch(self, queries: Sequence[Query], managers: Sequence[TopScoreDocCollectorManager], field: int,
                            similarity: str, query_vectors: np.ndarray, window: int, query_weight: float = 1.0,
                            rescore_weight: float = 1.0, boost: float = 1.0) -> List[TopDocs]:
        """search() followed by the vector rescorer for every query, fused on the device (config C5)."""
        return self._hybrid("nrtgpu_search_hybrid_batch", queries, managers, field, self.SIMILARITY[similarity],
                            np.ascontiguousarray(np.atleast_2d(query_vectors), dtype=np.float32), window, query_weight, rescore_weight, boost)

    def search_hybrid_bytes_batch(self, queries: Sequence[Query], managers: Sequence[TopScoreDocCollectorManager], field: int,
                                  similarity: str, query_vectors: np.ndarray, window: int, query_weight: float = 1.0,
                                  rescore_weight: float = 1.0, boost: float = 1.0) -> List[TopDocs]:
        """The same with a byte vector field as the rescorer (search() + rescore_byte_vectors per query); query_vectors: int8."""
        return self._hybrid("nrtgpu_search_hybrid_bytes_batch", queries, managers, field, self._byte_similarity(similarity),
                            _int8_rows(query_vectors, "query vectors"), window, query_weight, rescore_weight, boost)

    def _hybrid(self, entry: str, queries: Sequence[Query], managers: Sequence[TopScoreDocCollectorManager], field: int, sim: int,
                qv: np.ndarray, window: int, query_weight: float, rescore_weight: float, boost: float, dist_mode: Optional[int] = None) -> list:
        """dist_mode: the entry is the one over docid-range shards, which takes the exchange mode after the window and delivers only
        this rank's slice of the batch (None for the others)."""
        n = len(queries)
        if qv.shape[0] != n:
            raise ValueError("one query vector per query")
        m = self._marshal(queries, managers)
        h = _outputs(n, max(int(window), 1), int(window))
        _lib.check(getattr(_lib.load(), entry)(
            self.ctx._h, self._segs, self._bases, len(self.leaves), m.queries, n, int(field), sim, qv.ctypes.data, qv.shape[1],
            C.c_float(boost), float(query_weight), float(rescore_weight), int(window), *(() if dist_mode is None else (int(dist_mode),)), h.outs))
        return h.lists(none_if_negative=dist_mode is not None)

    def dist_search_hybrid_batch(self, queries: Sequence[Query], managers: Sequence[TopScoreDocCollectorManager], field: int,
                                 similarity: str, query_vectors: np.ndarray, window: int, query_weight: float = 1.0,
                                 rescore_weight: float = 1.0, boost: float = 1.0, mode: int = EXCHANGE_ALLGATHER) -> List[Optional[TopDocs]]:
        """The hybrid over docid-range shards (nrtgpu_dist_search_hybrid_batch): this rank's leaves; every rank passes the same
        queries and query vectors."""
        return self._hybrid("nrtgpu_dist_search_hybrid_batch", queries, managers, field, self.SIMILARITY[similarity],
                            np.ascontiguousarray(np.atleast_2d(query_vectors), dtype=np.float32), window, query_weight, rescore_weight, boost, mode)


# ---- pre-marshalled batches (bench / serving loop: no Python work inside the timed region) --------
class PreparedBatch:
    """A batch of queries marshalled once; `run()` is a single C-ABI call."""

    def __init__(self, searcher: GpuIndexSearcher, queries: Sequence[Query],
                 managers: Sequence[TopScoreDocCollectorManager]):
        self.searcher = searcher
        self.n = len(queries)
        self._m = searcher._marshal(queries, managers)
        self.k = max(int(m.num_hits) for m in managers)
        self._holder = _Outputs(self.n, self.k).begin(self.k)   # this batch's own: it lives across calls
        self._outs, self.docs, self.scores = self._holder.outs, self._holder.docs, self._holder.scores

    def run(self) -> None:
        s = self.searcher
        _lib.check(_lib.load().nrtgpu_search_bm25_batch(s.ctx._h, s._segs, s._bases, len(s.leaves),
                                                        self._m.queries, self.n, self._outs))

    def run_device(self, k_stride: int, d_keys: int, d_counts: int, d_hits: int, epoch: int = -1) -> None:
        """Results stay in HBM (device pointers as ints) for the RCCL all-gather.  epoch >= 0: take part in
        the context's cross-GPU bound exchange (GpuContext.exchange_open) as that batch number."""
        s = self.searcher
        _lib.check(_lib.load().nrtgpu_search_bm25_batch_device_epoch(
            s.ctx._h, s._segs, s._bases, len(s.leaves), self._m.queries, self.n, int(k_stride),
            C.c_void_p(d_keys), C.c_void_p(d_counts), C.c_void_p(d_hits), int(epoch)))

    def begin_device(self, k_stride: int, d_keys: int, d_counts: int, d_hits: int, epoch: int = -1) -> int:
        """run_device in two halves (nrtgpu_search_bm25_batch_device_begin): plans and enqueues, returns a pending handle at
        once; wait_device(handle) blocks until the results are complete in HBM."""
        s = self.searcher
        h = C.c_void_p()
        _lib.check(_lib.load().nrtgpu_search_bm25_batch_device_begin(
            s.ctx._h, s._segs, s._bases, len(s.leaves), self._m.queries, self.n, int(k_stride),
            C.c_void_p(d_keys), C.c_void_p(d_counts), C.c_void_p(d_hits), int(epoch), C.byref(h)))
        return h.value

    def begin_shard_device(self, k_stride: int, d_keys: int, d_counts: int, d_hits: int, spec_world: int, d_guess: int) -> int:
        """begin_device for ONE SHARD of a search that `spec_world` GPUs share (nrtgpu_search_bm25_shard_device_begin): the
        speculative thresholds are guesses at the whole search's k-th score, the largest per query is left in d_guess (n x u64 in
        HBM) for the check against the merged list (PreparedMerge.run_dist_checked).  spec_world 0: no speculation."""
        s = self.searcher
        h = C.c_void_p()
        _lib.check(_lib.load().nrtgpu_search_bm25_shard_device_begin(
            s.ctx._h, s._segs, s._bases, len(s.leaves), self._m.queries, self.n, int(k_stride),
            C.c_void_p(d_keys), C.c_void_p(d_counts), C.c_void_p(d_hits), int(spec_world), C.c_void_p(d_guess or None), C.byref(h)))
        return h.value

    def note_shard_speculation(self, n_queries: int, n_failed: int) -> None:
        s = self.searcher
        _lib.check(_lib.load().nrtgpu_note_shard_speculation(s.ctx._h, s._segs, len(s.leaves), int(n_queries), int(n_failed)))

    @staticmethod
    def wait_device(handle: int) -> None:
        _lib.check(_lib.load().nrtgpu_pending_wait(C.c_void_p(handle)))

    def topdocs(self, qi: int) -> TopDocs:
        return self._holder.topdocs(qi)


class PreparedMerge:
    """TopDocs.merge of all-gathered per-GPU results, output arrays marshalled once; `run()` is a
    single C-ABI call (nrtgpu_merge_topk_device).  List l of query q is row l * n_queries + q of the
    gathered arrays (all_gather_into_tensor concatenation order)."""

    def __init__(self, ctx: GpuContext, n_lists: int, n_queries: int, k_stride: int, ks: Sequence[int],
                 thresholds: Sequence[int]):
        self.ctx, self.n_lists, self.n, self.k_stride = ctx, int(n_lists), int(n_queries), int(k_stride)
        self._ks = np.ascontiguousarray(ks, dtype=np.int32)
        self._thr = np.ascontiguousarray(thresholds, dtype=np.int32)
        kmax = int(self._ks.max())
        self._holder = _Outputs(self.n, kmax).begin(kmax)   # this merge's own: it lives across calls
        self._outs, self.docs, self.scores = self._holder.outs, self._holder.docs, self._holder.scores

    def run(self, d_keys: int, d_counts: int, d_hits: int) -> None:
        _lib.check(_lib.load().nrtgpu_merge_topk_device(
            self.ctx._h, self.n_lists, self.n, self.k_stride, C.c_void_p(d_keys), C.c_void_p(d_counts),
            C.c_void_p(d_hits), self._ks.ctypes.data, self._thr.ctypes.data, self._outs))

    def run_dist(self, d_keys: int, d_counts: int, d_hits: int, mode: int = EXCHANGE_ALLGATHER) -> None:
        """This rank's device-resident shard results -> RCCL exchange inside the library -> merge
        (nrtgpu_dist_exchange_merge; GpuContext.dist_init first; n_lists must equal the world size).  EXCHANGE_ALLTOALL:
        only this rank's slice of the batch is merged and delivered (owned(qi))."""
        _lib.check(_lib.load().nrtgpu_dist_exchange_merge(
            self.ctx._h, self.n, self.k_stride, C.c_void_p(d_keys), C.c_void_p(d_counts), C.c_void_p(d_hits),
            self._ks.ctypes.data, self._thr.ctypes.data, int(mode), self._outs))

    def run_dist_checked(self, d_keys: int, d_counts: int, d_hits: int, d_guess: int, mode: int = EXCHANGE_ALLGATHER) -> np.ndarray:
        """run_dist with the shards' speculative thresholds (PreparedBatch.begin_shard_device's d_guess) checked against the
        merged lists (nrtgpu_dist_exchange_merge_checked) -> the indices of the queries EVERY rank has to run again without
        speculation (the same on every rank)."""
        failed = np.zeros(self.n, dtype=np.uint8)
        n_failed = C.c_int32(0)
        _lib.check(_lib.load().nrtgpu_dist_exchange_merge_checked(
            self.ctx._h, self.n, self.k_stride, C.c_void_p(d_keys), C.c_void_p(d_counts), C.c_void_p(d_hits), C.c_void_p(d_guess),
            self._ks.ctypes.data, self._thr.ctypes.data, int(mode), self._outs, failed.ctypes.data, C.byref(n_failed)))
        return np.flatnonzero(failed) if n_failed.value else np.zeros(0, dtype=np.int64)

    def kth_keys(self) -> np.ndarray:
        """Per query the key -- (score bits << 32) | (0xFFFFFFFF - docid), as the device packs it (csrc/plan.h: pack_key) -- of
        rank k of the merged list, 0 where the list is shorter: what a shard's guess is checked against (bench.py's emulated
        exchange does the check itself; the library's is nrtgpu_dist_exchange_merge_checked)."""
        n_hits = np.frombuffer(self._outs, dtype=np.int32).reshape(self.n, C.sizeof(_lib.TopDocs) // 4)[:, 0]
        rows = np.arange(self.n)
        col = self._ks.astype(np.int64) - 1
        keys = (self.scores.view(np.uint32)[rows, col].astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - self.docs[rows, col].astype(np.uint64))
        return np.where(n_hits >= self._ks, keys, np.uint64(0))

    def owned(self, qi: int) -> bool:
        return self._outs[qi].total_hits >= 0

    def topdocs(self, qi: int) -> TopDocs:
        return self._holder.topdocs(qi)


def merge_topk_device(ctx: GpuContext, n_lists: int, n_queries: int, k_stride: int, d_keys: int, d_counts: int,
                      d_hits: int, ks: Sequence[int], thresholds: Sequence[int]) -> List[TopDocs]:
    """TopDocs.merge of all-gathered per-GPU results (device pointers as ints)."""
    pm = PreparedMerge(ctx, n_lists, n_queries, k_stride, ks, thresholds)
    pm.run(d_keys, d_counts, d_hits)
    return [pm.topdocs(qi) for qi in range(n_queries)]


def slices(max_docs: Sequence[int], num_docs: Optional[Sequence[int]] = None, virtual_shards: int = 1,
           slice_max_docs: int = 250_000, slice_max_segments: int = 5):
    """MyIndexSearcher.slices / slicesForShards (S/search/MyIndexSearcher.java:79-208).
    -> (slices as lists of leaf indices in the reference's slice order, shard_of_leaf)."""
    n = len(max_docs)
    md = np.ascontiguousarray(max_docs, dtype=np.int32)
    nd = np.ascontiguousarray(num_docs if num_docs is not None else max_docs, dtype=np.int32)
    sl = np.full(max(n, 1), -1, dtype=np.int32)
    sh = np.full(max(n, 1), -1, dtype=np.int32)
    ns = _lib.load().nrtgpu_slices(n, md.ctypes.data, nd.ctypes.data, None, int(virtual_shards), int(slice_max_docs),
                                   int(slice_max_segments), sl.ctypes.data, sh.ctypes.data)
    if ns < 0:
        _lib.check(ns)
    out: List[List[int]] = [[] for _ in range(ns)]
    for i in range(n):
        out[sl[i]].append(i)
    return out, sh[:n].tolist()


def _marshal_counted(searcher: "GpuIndexSearcher", queries: Sequence[Query], managers: Sequence[TopScoreDocCollectorManager]) -> _Marshalled:
    """The queries of a route that counts matching clauses itself (sorted searches, terms and range counts): a BooleanQuery of MUST
    clauses only goes down as MUST clauses, not as the disjunction with minimumNumberShouldMatch = n the scoring routes take."""
    m = searcher._marshal(queries, managers)
    for qi, query in enumerate(queries):
        if isinstance(query, BooleanQuery) and query.must and not query.should and not isinstance(query.must[0], DisjunctionMaxQuery):
            q = m.queries[qi]
            for ti in range(q.n_terms):
                q.terms[ti].occur = 1
            q.min_should_match = 0
    return m


def _marshal_sorted(searcher: "GpuIndexSearcher", queries: Sequence[Query], managers: Sequence[TopScoreDocCollectorManager],
                    sorts: Sequence[SortField], afters: Optional[Sequence[Optional[FieldDoc]]]):
    """The queries and nrtgpu_field_sort per query of a sorted search.  A BooleanQuery of MUST clauses only goes down as MUST
    clauses (the route counts them itself), not as the disjunction with minimumNumberShouldMatch = n the scoring routes take."""
    if len(sorts) != len(queries) or (afters is not None and len(afters) != len(queries)):
        raise ValueError(f"{len(sorts)} sorts / {None if afters is None else len(afters)} afters for {len(queries)} queries")
    m = _marshal_counted(searcher, queries, managers)
    fs = (_lib.FieldSort * len(queries))()
    for qi, sort in enumerate(sorts):
        if sort.kind not in DOC_VALUE_KINDS:
            raise UnsupportedQuery(f"a sort of kind {sort.kind!r}")
        after = afters[qi] if afters is not None else None
        fs[qi] = _lib.FieldSort(int(sort.field), int(bool(sort.reverse)), _value_bits(sort.kind, sort.missing), int(after is not None),
                                int(after.doc) if after is not None else 0, _value_bits(sort.kind, after.value) if after is not None else 0)
    m.keep.append(fs)
    return m, fs


def search_sorted_batch(searcher: "GpuIndexSearcher", queries: Sequence[Query], managers: Sequence[TopScoreDocCollectorManager],
                        sorts: Sequence[SortField], afters: Optional[Sequence[Optional[FieldDoc]]] = None) -> List[TopFieldDocs]:
    """Sorted searches (nrtgpu_search_sorted_batch): the hits of queries[i] ordered by sorts[i] (value in the sort's direction,
    ties by docid ascending), the page behind afters[i] when that is given (managers[i].after stays None: the cursor of a sorted
    search is a FieldDoc).  total_hits is exact; scores are not computed."""
    m, fs = _marshal_sorted(searcher, queries, managers, sorts, afters)
    n = len(m.queries)
    h = _text_outputs(n, managers)
    _lib.check(_lib.load().nrtgpu_search_sorted_batch(searcher.ctx._h, searcher._segs, searcher._bases, len(searcher.leaves), m.queries, fs, n,
                                                      C.cast(h.outs, C.POINTER(_lib.FieldDocs))))
    return [TopFieldDocs(t.docs, t.scores.view(DOC_VALUE_KINDS[sort.kind][1]), t.total_hits, t.relation_gte) for t, sort in zip(h.lists(), sorts)]


def sorted_supported(searcher: "GpuIndexSearcher", query: Query, manager: TopScoreDocCollectorManager, sort: SortField,
                     after: Optional[FieldDoc] = None) -> bool:
    """The eligibility predicate alone (nrtgpu_sorted_supported)."""
    m, fs = _marshal_sorted(searcher, [query], [manager], [sort], [after])
    return _supported(_lib.load().nrtgpu_sorted_supported(searcher.ctx._h, searcher._segs, len(searcher.leaves), m.queries, fs))


def sort_value_code(kind: str, reverse: bool, value_bits: int) -> int:
    """The high word of the key a value sorts under (nrtgpu_sort_value_code: the function the kernel compiles).  No device."""
    out = C.c_uint32(0)
    _lib.check(_lib.load().nrtgpu_sort_value_code(DOC_VALUE_KINDS[kind][0], int(bool(reverse)), C.c_uint32(int(value_bits)), C.byref(out)))
    return int(out.value)


@dataclasses.dataclass(frozen=True)
class TermsCollector:
    """A TermsCollector over an int or float field (source FIELD, order COUNT, no nested collectors): `field` names the doc value
    column of kind `kind` -- single-valued (GpuSegment.add_doc_values) or multi-valued (add_doc_values_multi: every value instance
    of a hit counts, as for a SORTED_SET facet uploaded as its global ordinals); `size` and `order_desc` are what the caller's reduce() applies
    to the returned map (fill_bucket_result), the device does not read them.  kind "long" / "double": a collector over a single-valued
    64-bit column (add_doc_values64), for count_terms64_batch / count_docset_terms64_batch."""

    field: int
    size: int
    order_desc: bool = True
    kind: str = "int"


@dataclasses.dataclass
class TermCounts:
    """The count map of one query (nrtgpu_term_counts): the distinct values of its hits, ascending in the kind's order, and the
    hits per value.  overflowed: the hits hold more than max_buckets distinct values -- no buckets, hits_with_value -1, total_hits
    still exact; the request goes to the CPU path."""

    values: np.ndarray          # int32 / float32 (a NaN bucket reads 0x7FC00000)
    counts: np.ndarray          # int32
    total_hits: int
    hits_with_value: int
    overflowed: bool

    @property
    def value_bits(self) -> np.ndarray:
        return self.values.view(np.uint32)


@dataclasses.dataclass
class BucketResult:
    buckets: List[Tuple[Union[int, float], int]]   # (key, count), best first
    total_buckets: int
    total_other_counts: int


def fill_bucket_result(values, counts, size: int, order_desc: bool = True) -> BucketResult:
    """TermsCollectorManager.fillBucketResultByCount over a returned count map: the `size` buckets with the largest (order_desc)
    or smallest counts, best first; total_buckets = len(map); total_other_counts = the sum of the counts left out.  An empty map
    or size <= 0 gives the empty result, as in the reference.  Ties are broken by value ascending (the map's order).  The
    reference's ties follow its hash map's iteration order, so ANY order among equal counts at the cut is a valid answer; away
    from ties the results are the reference's."""
    keys = np.asarray(values).tolist()
    cnts = np.asarray(counts).tolist()
    if not keys or size <= 0:
        return BucketResult([], 0, 0)
    order = sorted(range(len(keys)), key=lambda i: (-cnts[i] if order_desc else cnts[i], i))
    kept = order[:size]
    return BucketResult([(keys[i], int(cnts[i])) for i in kept], len(keys), int(sum(cnts[i] for i in order[size:])))


def _marshal_terms(searcher: "GpuIndexSearcher", queries: Sequence[Query], collectors: Sequence[TermsCollector], max_buckets,
                   managers: Optional[Sequence[TopScoreDocCollectorManager]]):
    """The queries and nrtgpu_terms_count per query of a terms aggregation (MUST-only queries as in _marshal_sorted)."""
    n = len(queries)
    if len(collectors) != n:
        raise ValueError(f"{len(collectors)} collectors for {n} queries")
    bounds = [int(max_buckets)] * n if np.isscalar(max_buckets) else [int(b) for b in max_buckets]
    if len(bounds) != n:
        raise ValueError(f"{len(bounds)} max_buckets for {n} queries")
    for c in collectors:
        if c.kind not in DOC_VALUE_KINDS:
            raise UnsupportedQuery(f"a terms collector of kind {c.kind!r}")
    mgrs = list(managers) if managers is not None else [TopScoreDocCollectorManager(1)] * n
    m, _ = _marshal_sorted(searcher, queries, mgrs, [SortField(c.field, c.kind) for c in collectors], None)
    tc = (_lib.TermsCount * n)()
    for qi, (c, b) in enumerate(zip(collectors, bounds)):
        tc[qi] = _lib.TermsCount(int(c.field), b)
    m.keep.append(tc)
    return m, tc, bounds


def count_terms_batch(searcher: "GpuIndexSearcher", queries: Sequence[Query], collectors: Sequence[TermsCollector], max_buckets=4096,
                      managers: Optional[Sequence[TopScoreDocCollectorManager]] = None) -> List[TermCounts]:
    """Terms aggregations (nrtgpu_count_terms_batch): per query the whole map value -> hits of collectors[i].field over the hits
    of queries[i]; max_buckets: one bound for all, or one per query.  No hits are returned: the request's top-k comes from a
    search entry.  Apply size and order with fill_bucket_result."""
    m, tc, bounds = _marshal_terms(searcher, queries, collectors, max_buckets, managers)
    n = len(queries)
    width = max([max(b, 1) for b in bounds], default=1)
    bits = np.zeros((n, width), dtype=np.uint32)
    counts = np.zeros((n, width), dtype=np.int32)
    outs = (_lib.TermCounts * n)()
    for qi in range(n):
        outs[qi].capacity = max(bounds[qi], 0)
        outs[qi].value_bits = C.cast(bits.ctypes.data + qi * width * 4, C.POINTER(C.c_uint32))
        outs[qi].counts = C.cast(counts.ctypes.data + qi * width * 4, C.POINTER(C.c_int32))
    _lib.check(_lib.load().nrtgpu_count_terms_batch(searcher.ctx._h, searcher._segs, searcher._bases, len(searcher.leaves), m.queries, tc, n, outs))
    return [TermCounts(bits[qi, : o.n_buckets].view(DOC_VALUE_KINDS[c.kind][1]).copy(), counts[qi, : o.n_buckets].copy(), int(o.total_hits),
                       int(o.hits_with_value), bool(o.overflowed)) for qi, (o, c) in enumerate(zip(outs, collectors))]


def count_terms_supported(searcher: "GpuIndexSearcher", query: Query, collector: TermsCollector, max_buckets: int = 4096,
                          manager: Optional[TopScoreDocCollectorManager] = None) -> bool:
    """The eligibility predicate alone (nrtgpu_count_terms_supported)."""
    m, tc, _ = _marshal_terms(searcher, [query], [collector], max_buckets, None if manager is None else [manager])
    return _supported(_lib.load().nrtgpu_count_terms_supported(searcher.ctx._h, searcher._segs, len(searcher.leaves), m.queries, tc))


@dataclasses.dataclass(frozen=True)
class RangeClause:
    """IntFieldDef / FloatFieldDef.getRangeQuery over a field with doc values (a multi-valued column: SOME value of the doc): lower <= value <= upper, both bounds
    INCLUSIVE, in the order of the column's kind (floats: -0.0 < +0.0, NaN above +inf).  An exclusive bound is the caller's to map
    (lower + 1 / np.nextafter).  A doc without a value fails the clause; lower > upper matches nothing."""

    field: int
    kind: str
    lower: Union[int, float]
    upper: Union[int, float]


@dataclasses.dataclass(frozen=True)
class DocSetQuery:
    """A query without a text clause: MatchAllDocsQuery (all three empty), or a BooleanQuery of FILTER / MUST_NOT clauses only --
    resident masks and numeric ranges.  Its hits are the live docs inside every filter and every range and outside every must_not."""

    filter: Tuple[MaskFilter, ...] = ()
    must_not: Tuple[MaskFilter, ...] = ()
    ranges: Tuple[RangeClause, ...] = ()


@dataclasses.dataclass(frozen=True)
class ValueClause:
    """One clause of a mask built on the device from a doc value column (GpuSegment.set_mask_from_values; nrtgpu_value_clause):
    range_ (RangeClause's rule: lower <= value <= upper, inclusive, in the kind's order), exists (FieldExistsQuery: the doc has a
    value; a NaN is one) or in_set (TermInSetQuery / IntPoint.newSetQuery: a value equal to a listed one; floats compare as
    encoded points: -0.0 and +0.0 are different members, any NaN matches every NaN).  Over a multi-valued column SOME value of
    the doc passes; a doc without a value fails every clause.  `kind` says how lower / upper / values become bits -- the column's
    own kind is the resident column's.  Use the constructors."""

    clause: str                          # "range" | "exists" | "in_set"
    field: int
    kind: str = "int"
    lower_bits: int = 0
    upper_bits: int = 0
    value_bits: bytes = b""             # in_set: the values' bits, uint32 after uint32 in native order (np.frombuffer(.., np.uint32))

    @classmethod
    def range_(cls, field: int, kind: str, lower, upper) -> "ValueClause":
        if kind not in DOC_VALUE_KINDS:
            raise UnsupportedQuery(f"a range clause of kind {kind!r}")
        return cls("range", int(field), kind, _value_bits(kind, lower), _value_bits(kind, upper))

    @classmethod
    def exists(cls, field: int) -> "ValueClause":
        return cls("exists", int(field))

    @classmethod
    def in_set(cls, field: int, kind: str, values) -> "ValueClause":
        """values: any order, duplicates allowed; an array of the kind's dtype, or uint32 for the kind's raw bits (a NaN with a
        payload), or a sequence of Python numbers.  No silent cast of an array of another dtype."""
        if kind not in DOC_VALUE_KINDS:
            raise UnsupportedQuery(f"an in-set clause of kind {kind!r}")
        if isinstance(values, np.ndarray):
            if values.dtype not in (DOC_VALUE_KINDS[kind][1], np.dtype(np.uint32)):
                raise TypeError(f"values of kind {kind!r} must be {DOC_VALUE_KINDS[kind][1]} (or uint32 bits), got {values.dtype}")
            bits = np.ascontiguousarray(values).reshape(-1).view(np.uint32)
        else:
            bits = np.array(list(values), dtype=DOC_VALUE_KINDS[kind][1]).reshape(-1).view(np.uint32)
        if not 1 <= len(bits) <= _lib.NRTGPU_MAX_SET_VALUES:
            raise ValueError(f"{len(bits)} values in a set: 1..{_lib.NRTGPU_MAX_SET_VALUES}")
        return cls("in_set", int(field), kind, 0, 0, bits.tobytes())


_VALUE_CLAUSE_KINDS = {"range": _lib.NRTGPU_CLAUSE_RANGE, "exists": _lib.NRTGPU_CLAUSE_EXISTS, "in_set": _lib.NRTGPU_CLAUSE_IN_SET}


def _marshal_value_clauses(clauses: Sequence[ValueClause]):
    """nrtgpu_value_clause per clause (and what keeps the sets' arrays alive)."""
    n = len(clauses)
    if not 1 <= n <= _lib.NRTGPU_MAX_RANGES:
        raise ValueError(f"{n} clauses: 1..{_lib.NRTGPU_MAX_RANGES}")
    vc = (_lib.ValueClause * n)()
    keep: list = [vc]
    for i, c in enumerate(clauses):
        if c.clause not in _VALUE_CLAUSE_KINDS:
            raise UnsupportedQuery(f"a value clause {c.clause!r}")
        r = vc[i]
        r.kind, r.field_id = _VALUE_CLAUSE_KINDS[c.clause], int(c.field)
        if c.clause == "range":
            r.lower_bits, r.upper_bits = int(c.lower_bits), int(c.upper_bits)
        elif c.clause == "in_set":
            n_values = len(c.value_bits) // 4
            if len(c.value_bits) % 4 or not 1 <= n_values <= _lib.NRTGPU_MAX_SET_VALUES:
                raise ValueError(f"{len(c.value_bits)} bytes of values in a set: 1..{_lib.NRTGPU_MAX_SET_VALUES} values of 4 bytes")
            arr = (C.c_uint32 * n_values).from_buffer_copy(c.value_bits)
            keep.append(arr)
            r.n_values, r.value_bits = n_values, arr
    return vc, keep


def _marshal_docsets(docsets: Sequence[DocSetQuery], managers: Sequence[TopScoreDocCollectorManager]):
    """nrtgpu_docset_query per query (and what keeps its arrays alive)."""
    n = len(docsets)
    if len(managers) != n:
        raise ValueError(f"{len(managers)} managers for {n} doc-set queries")
    ds = (_lib.DocsetQuery * n)()
    keep: list = [ds]
    for qi, (d, mgr) in enumerate(zip(docsets, managers)):
        if mgr.after is not None or mgr.min_competitive_score != 0.0:
            raise UnsupportedQuery("a doc-set query has no score cursor and no min_competitive_score")
        q = ds[qi]
        filters, must_nots = [int(f.mask_id) for f in d.filter], [int(f.mask_id) for f in d.must_not]
        q.filter_mask = filters[0] if filters else 0
        q.must_not_mask = must_nots[0] if must_nots else 0
        for ids, n_name, p_name in ((filters[1:], "n_more_filters", "more_filters"), (must_nots[1:], "n_more_must_not", "more_must_not")):
            if ids:
                arr = (C.c_int32 * len(ids))(*ids)
                keep.append(arr)
                setattr(q, n_name, len(ids))
                setattr(q, p_name, arr)
        if d.ranges:
            for r in d.ranges:
                if r.kind not in DOC_VALUE_KINDS:
                    raise UnsupportedQuery(f"a range clause of kind {r.kind!r}")
            rc = (_lib.RangeClause * len(d.ranges))(*[_lib.RangeClause(int(r.field), _value_bits(r.kind, r.lower), _value_bits(r.kind, r.upper), 0)
                                                      for r in d.ranges])
            keep.append(rc)
            q.ranges = rc
        q.n_ranges = len(d.ranges)
        q.k = int(mgr.num_hits)
        q.total_hits_threshold = int(mgr.total_hits_threshold)
    return ds, keep


def _docset_sorts(sorts: Sequence[SortField], afters, n: int):
    if len(sorts) != n or (afters is not None and len(afters) != n):
        raise ValueError(f"{len(sorts)} sorts / {None if afters is None else len(afters)} afters for {n} queries")
    fs = (_lib.FieldSort * n)()
    for qi, sort in enumerate(sorts):
        if sort.kind not in DOC_VALUE_KINDS:
            raise UnsupportedQuery(f"a sort of kind {sort.kind!r}")
        after = afters[qi] if afters is not None else None
        fs[qi] = _lib.FieldSort(int(sort.field), int(bool(sort.reverse)), _value_bits(sort.kind, sort.missing), int(after is not None),
                                int(after.doc) if after is not None else 0, _value_bits(sort.kind, after.value) if after is not None else 0)
    return fs


def search_docset_sorted_batch(searcher: "GpuIndexSearcher", docsets: Sequence[DocSetQuery], managers: Sequence[TopScoreDocCollectorManager],
                               sorts: Sequence[SortField], afters: Optional[Sequence[Optional[FieldDoc]]] = None) -> List[TopFieldDocs]:
    """Sorted doc-set searches (nrtgpu_search_docset_sorted_batch): the hits of docsets[i] ordered by sorts[i], the page behind
    afters[i] when that is given -- search_sorted_batch's results over a hit set without a text clause."""
    ds, keep = _marshal_docsets(docsets, managers)
    n = len(docsets)
    fs = _docset_sorts(sorts, afters, n)
    h = _text_outputs(n, managers)
    _lib.check(_lib.load().nrtgpu_search_docset_sorted_batch(searcher.ctx._h, searcher._segs, searcher._bases, len(searcher.leaves), ds, fs, n,
                                                             C.cast(h.outs, C.POINTER(_lib.FieldDocs))))
    del keep
    return [TopFieldDocs(t.docs, t.scores.view(DOC_VALUE_KINDS[sort.kind][1]), t.total_hits, t.relation_gte) for t, sort in zip(h.lists(), sorts)]


def docset_sorted_supported(searcher: "GpuIndexSearcher", docset: DocSetQuery, manager: TopScoreDocCollectorManager, sort: SortField,
                            after: Optional[FieldDoc] = None) -> bool:
    """The eligibility predicate alone (nrtgpu_docset_sorted_supported)."""
    ds, keep = _marshal_docsets([docset], [manager])
    fs = _docset_sorts([sort], [after], 1)
    rc = _lib.load().nrtgpu_docset_sorted_supported(searcher.ctx._h, searcher._segs, len(searcher.leaves), ds, fs)
    del keep
    return _supported(rc)


def _docset_terms(docsets, collectors: Sequence[TermsCollector], max_buckets, managers):
    n = len(docsets)
    if len(collectors) != n:
        raise ValueError(f"{len(collectors)} collectors for {n} queries")
    bounds = [int(max_buckets)] * n if np.isscalar(max_buckets) else [int(b) for b in max_buckets]
    if len(bounds) != n:
        raise ValueError(f"{len(bounds)} max_buckets for {n} queries")
    for c in collectors:
        if c.kind not in DOC_VALUE_KINDS:
            raise UnsupportedQuery(f"a terms collector of kind {c.kind!r}")
    mgrs = list(managers) if managers is not None else [TopScoreDocCollectorManager(1)] * n
    ds, keep = _marshal_docsets(docsets, mgrs)
    tc = (_lib.TermsCount * n)(*[_lib.TermsCount(int(c.field), b) for c, b in zip(collectors, bounds)])
    return ds, keep, tc, bounds


def count_docset_terms_batch(searcher: "GpuIndexSearcher", docsets: Sequence[DocSetQuery], collectors: Sequence[TermsCollector], max_buckets=4096,
                             managers: Optional[Sequence[TopScoreDocCollectorManager]] = None) -> List[TermCounts]:
    """Terms aggregations over doc sets (nrtgpu_count_docset_terms_batch): count_terms_batch's results over a hit set without a
    text clause."""
    ds, keep, tc, bounds = _docset_terms(docsets, collectors, max_buckets, managers)
    n = len(docsets)
    width = max([max(b, 1) for b in bounds], default=1)
    bits = np.zeros((n, width), dtype=np.uint32)
    counts = np.zeros((n, width), dtype=np.int32)
    outs = (_lib.TermCounts * n)()
    for qi in range(n):
        outs[qi].capacity = max(bounds[qi], 0)
        outs[qi].value_bits = C.cast(bits.ctypes.data + qi * width * 4, C.POINTER(C.c_uint32))
        outs[qi].counts = C.cast(counts.ctypes.data + qi * width * 4, C.POINTER(C.c_int32))
    _lib.check(_lib.load().nrtgpu_count_docset_terms_batch(searcher.ctx._h, searcher._segs, searcher._bases, len(searcher.leaves), ds, tc, n, outs))
    del keep
    return [TermCounts(bits[qi, : o.n_buckets].view(DOC_VALUE_KINDS[c.kind][1]).copy(), counts[qi, : o.n_buckets].copy(), int(o.total_hits),
                       int(o.hits_with_value), bool(o.overflowed)) for qi, (o, c) in enumerate(zip(outs, collectors))]


def count_docset_terms_supported(searcher: "GpuIndexSearcher", docset: DocSetQuery, collector: TermsCollector, max_buckets: int = 4096,
                                 manager: Optional[TopScoreDocCollectorManager] = None) -> bool:
    """The eligibility predicate alone (nrtgpu_count_docset_terms_supported)."""
    ds, keep, tc, _ = _docset_terms([docset], [collector], max_buckets, None if manager is None else [manager])
    rc = _lib.load().nrtgpu_count_docset_terms_supported(searcher.ctx._h, searcher._segs, len(searcher.leaves), ds, tc)
    del keep
    return _supported(rc)


def range_accepts(kind: str, lower_bits: int, upper_bits: int, value_bits: int) -> bool:
    """Whether a range clause keeps a value (nrtgpu_range_accepts: the function the kernels compile).  No device."""
    out = C.c_int32(0)
    _lib.check(_lib.load().nrtgpu_range_accepts(DOC_VALUE_KINDS[kind][0], C.c_uint32(int(lower_bits)), C.c_uint32(int(upper_bits)),
                                                C.c_uint32(int(value_bits)), C.byref(out)))
    return bool(out.value)


# ---- 64-bit columns: sort by a LONG / DATE_TIME / DOUBLE field, masks from such columns ----------------------------------------
@dataclasses.dataclass(frozen=True)
class SortField64:
    """SortField(field, Type.LONG / Type.DOUBLE, reverse) over a 64-bit doc value column (GpuSegment.add_doc_values64); `missing`
    as in SortField (the reference passes Long.MIN_VALUE / MAX_VALUE or -+inf)."""

    field: int
    kind: str = "long"
    reverse: bool = False
    missing: Union[int, float] = 0


@dataclasses.dataclass
class TopFieldDocs64:
    docs: np.ndarray            # int32 global docids, in the sort's order
    values: np.ndarray          # int64 / float64: the value each hit sorted as (the missing value for a doc without one)
    total_hits: int
    relation_gte: bool

    @property
    def value_bits(self) -> np.ndarray:
        return self.values.view(np.uint64)


@dataclasses.dataclass(frozen=True)
class ValueClause64:
    """One clause of a mask built from a 64-bit column (GpuSegment.set_mask_from_values64; nrtgpu_value_clause64): range_ (lower
    <= value <= upper, inclusive, Long.compare / the order of doubleToSortableLong) or exists.  Use the constructors."""

    clause: str                          # "range" | "exists"
    field: int
    kind: str = "long"
    lower_bits: int = 0
    upper_bits: int = 0

    @classmethod
    def range_(cls, field: int, kind: str, lower, upper) -> "ValueClause64":
        if kind not in DOC_VALUE_KINDS64:
            raise UnsupportedQuery(f"a 64-bit range clause of kind {kind!r}")
        return cls("range", int(field), kind, _value_bits64(kind, lower), _value_bits64(kind, upper))

    @classmethod
    def exists(cls, field: int) -> "ValueClause64":
        return cls("exists", int(field))


def _field_sorts64(sorts: Sequence[SortField64], afters, n: int):
    if len(sorts) != n or (afters is not None and len(afters) != n):
        raise ValueError(f"{len(sorts)} sorts / {None if afters is None else len(afters)} afters for {n} queries")
    fs = (_lib.FieldSort64 * n)()
    for qi, sort in enumerate(sorts):
        if sort.kind not in DOC_VALUE_KINDS64:
            raise UnsupportedQuery(f"a 64-bit sort of kind {sort.kind!r}")
        after = afters[qi] if afters is not None else None
        fs[qi] = _lib.FieldSort64(int(sort.field), int(bool(sort.reverse)), _value_bits64(sort.kind, sort.missing), int(after is not None),
                                  int(after.doc) if after is not None else 0, _value_bits64(sort.kind, after.value) if after is not None else 0)
    return fs


class _Outputs64:
    """The nrtgpu_fielddocs64 of a call: rows of an int32 and a uint64 array."""

    def __init__(self, managers):
        caps = [max(int(mgr.num_hits), 1) for mgr in managers]
        n, width = len(caps), max(caps, default=1)
        self.outs = (_lib.FieldDocs64 * n)()
        self.docs = np.zeros((n, width), dtype=np.int32)
        self.bits = np.zeros((n, width), dtype=np.uint64)
        for qi in range(n):
            self.outs[qi].capacity = caps[qi]
            self.outs[qi].docs = C.cast(self.docs.ctypes.data + qi * width * 4, C.POINTER(C.c_int32))
            self.outs[qi].value_bits = C.cast(self.bits.ctypes.data + qi * width * 8, C.POINTER(C.c_uint64))

    def lists(self, sorts) -> List[TopFieldDocs64]:
        return [TopFieldDocs64(self.docs[qi, : o.n_hits].copy(), self.bits[qi, : o.n_hits].copy().view(DOC_VALUE_KINDS64[sort.kind][1]), int(o.total_hits),
                               bool(o.total_hits_is_lower_bound)) for qi, (o, sort) in enumerate(zip(self.outs, sorts))]


def _marshal_sorted64(searcher: "GpuIndexSearcher", queries: Sequence[Query], managers: Sequence[TopScoreDocCollectorManager],
                      sorts: Sequence[SortField64], afters):
    """_marshal_sorted's queries (a BooleanQuery of MUST clauses only goes down as MUST clauses) beside nrtgpu_field_sort64 records."""
    fs = _field_sorts64(sorts, afters, len(queries))
    m, _ = _marshal_sorted(searcher, queries, managers, [SortField(int(s.field)) for s in sorts], None)
    m.keep.append(fs)
    return m, fs


def search_sorted64_batch(searcher: "GpuIndexSearcher", queries: Sequence[Query], managers: Sequence[TopScoreDocCollectorManager],
                          sorts: Sequence[SortField64], afters: Optional[Sequence[Optional[FieldDoc]]] = None) -> List[TopFieldDocs64]:
    """Sorted searches over 64-bit columns (nrtgpu_search_sorted64_batch): search_sorted_batch's results with int64 / float64
    values ("newest first" over epoch millis)."""
    m, fs = _marshal_sorted64(searcher, queries, managers, sorts, afters)
    n = len(m.queries)
    h = _Outputs64(managers)
    _lib.check(_lib.load().nrtgpu_search_sorted64_batch(searcher.ctx._h, searcher._segs, searcher._bases, len(searcher.leaves), m.queries, fs, n, h.outs))
    return h.lists(sorts)


def sorted64_supported(searcher: "GpuIndexSearcher", query: Query, manager: TopScoreDocCollectorManager, sort: SortField64,
                       after: Optional[FieldDoc] = None) -> bool:
    """The eligibility predicate alone (nrtgpu_sorted64_supported)."""
    m, fs = _marshal_sorted64(searcher, [query], [manager], [sort], [after])
    return _supported(_lib.load().nrtgpu_sorted64_supported(searcher.ctx._h, searcher._segs, len(searcher.leaves), m.queries, fs))


def search_docset_sorted64_batch(searcher: "GpuIndexSearcher", docsets: Sequence[DocSetQuery], managers: Sequence[TopScoreDocCollectorManager],
                                 sorts: Sequence[SortField64], afters: Optional[Sequence[Optional[FieldDoc]]] = None) -> List[TopFieldDocs64]:
    """Sorted doc-set searches over 64-bit columns (nrtgpu_search_docset_sorted64_batch)."""
    ds, keep = _marshal_docsets(docsets, managers)
    n = len(docsets)
    fs = _field_sorts64(sorts, afters, n)
    h = _Outputs64(managers)
    _lib.check(_lib.load().nrtgpu_search_docset_sorted64_batch(searcher.ctx._h, searcher._segs, searcher._bases, len(searcher.leaves), ds, fs, n, h.outs))
    del keep
    return h.lists(sorts)


def docset_sorted64_supported(searcher: "GpuIndexSearcher", docset: DocSetQuery, manager: TopScoreDocCollectorManager, sort: SortField64,
                              after: Optional[FieldDoc] = None) -> bool:
    """The eligibility predicate alone (nrtgpu_docset_sorted64_supported)."""
    ds, keep = _marshal_docsets([docset], [manager])
    fs = _field_sorts64([sort], [after], 1)
    rc = _lib.load().nrtgpu_docset_sorted64_supported(searcher.ctx._h, searcher._segs, len(searcher.leaves), ds, fs)
    del keep
    return _supported(rc)


def sort_key64(kind: str, reverse: bool, lo_bits: int, hi_bits: int, missing_bits: int, doc_bits: int, has_value: bool, value_bits: int,
               global_doc: int) -> int:
    """The packed key of one doc (nrtgpu_sort_key64: the function the kernels compile).  No device.  NrtGpuError with code
    NRTGPU_ERR_UNSUPPORTED when the window does not fit beside doc_bits docid bits."""
    out = C.c_uint64(0)
    _lib.check(_lib.load().nrtgpu_sort_key64(DOC_VALUE_KINDS64[kind][0], int(bool(reverse)), C.c_uint64(int(lo_bits)), C.c_uint64(int(hi_bits)),
                                             C.c_uint64(int(missing_bits)), int(doc_bits), int(bool(has_value)), C.c_uint64(int(value_bits)),
                                             int(global_doc), C.byref(out)))
    return int(out.value)


def range_accepts64(kind: str, lower_bits: int, upper_bits: int, value_bits: int) -> bool:
    """Whether a 64-bit range clause keeps a value (nrtgpu_range_accepts64: the function the kernel compiles).  No device."""
    out = C.c_int32(0)
    _lib.check(_lib.load().nrtgpu_range_accepts64(DOC_VALUE_KINDS64[kind][0], C.c_uint64(int(lower_bits)), C.c_uint64(int(upper_bits)),
                                                  C.c_uint64(int(value_bits)), C.byref(out)))
    return bool(out.value)


# ---- terms aggregation over 64-bit columns: TermsCollector(kind="long" / "double") ---------------------------------------------
@dataclasses.dataclass
class TermCounts64:
    """TermCounts over a LONG / DATE_TIME / DOUBLE column (nrtgpu_term_counts64): the distinct values of the hits, ascending in
    the kind's order (Long.compare / Double.compare), and the hits per value; overflowed as there."""

    values: np.ndarray          # int64 / float64 (a NaN bucket reads 0x7FF8000000000000)
    counts: np.ndarray          # int32
    total_hits: int
    hits_with_value: int
    overflowed: bool

    @property
    def value_bits(self) -> np.ndarray:
        return self.values.view(np.uint64)


class _TermOutputs64:
    """The nrtgpu_term_counts64 of a call: rows of a uint64 and an int32 array."""

    def __init__(self, bounds):
        n, width = len(bounds), max([max(b, 1) for b in bounds], default=1)
        self.outs = (_lib.TermCounts64 * n)()
        self.bits = np.zeros((n, width), dtype=np.uint64)
        self.counts = np.zeros((n, width), dtype=np.int32)
        for qi in range(n):
            self.outs[qi].capacity = max(bounds[qi], 0)
            self.outs[qi].value_bits = C.cast(self.bits.ctypes.data + qi * width * 8, C.POINTER(C.c_uint64))
            self.outs[qi].counts = C.cast(self.counts.ctypes.data + qi * width * 4, C.POINTER(C.c_int32))

    def lists(self, collectors) -> List[TermCounts64]:
        return [TermCounts64(self.bits[qi, : o.n_buckets].copy().view(DOC_VALUE_KINDS64[c.kind][1]), self.counts[qi, : o.n_buckets].copy(),
                             int(o.total_hits), int(o.hits_with_value), bool(o.overflowed)) for qi, (o, c) in enumerate(zip(self.outs, collectors))]


def _terms64(collectors: Sequence[TermsCollector], max_buckets, n: int):
    """The nrtgpu_terms_count per query of a count over 64-bit columns, and the bounds."""
    if len(collectors) != n:
        raise ValueError(f"{len(collectors)} collectors for {n} queries")
    bounds = [int(max_buckets)] * n if np.isscalar(max_buckets) else [int(b) for b in max_buckets]
    if len(bounds) != n:
        raise ValueError(f"{len(bounds)} max_buckets for {n} queries")
    for c in collectors:
        if c.kind not in DOC_VALUE_KINDS64:
            raise UnsupportedQuery(f"a 64-bit terms collector of kind {c.kind!r}")
    tc = (_lib.TermsCount * n)(*[_lib.TermsCount(int(c.field), b) for c, b in zip(collectors, bounds)])
    return tc, bounds


def _marshal_terms64(searcher: "GpuIndexSearcher", queries: Sequence[Query], collectors: Sequence[TermsCollector], max_buckets, managers):
    n = len(queries)
    tc, bounds = _terms64(collectors, max_buckets, n)
    mgrs = list(managers) if managers is not None else [TopScoreDocCollectorManager(1)] * n
    m = _marshal_counted(searcher, queries, mgrs)
    m.keep.append(tc)
    return m, tc, bounds


def count_terms64_batch(searcher: "GpuIndexSearcher", queries: Sequence[Query], collectors: Sequence[TermsCollector], max_buckets=4096,
                        managers: Optional[Sequence[TopScoreDocCollectorManager]] = None) -> List[TermCounts64]:
    """Terms aggregations over 64-bit columns (nrtgpu_count_terms64_batch): count_terms_batch's results with int64 / float64
    values; collectors[i].kind is "long" (LONG, DATE_TIME as epoch millis) or "double".  A batch may mix the two."""
    m, tc, bounds = _marshal_terms64(searcher, queries, collectors, max_buckets, managers)
    h = _TermOutputs64(bounds)
    _lib.check(_lib.load().nrtgpu_count_terms64_batch(searcher.ctx._h, searcher._segs, searcher._bases, len(searcher.leaves), m.queries, tc, len(queries), h.outs))
    return h.lists(collectors)


def count_terms64_supported(searcher: "GpuIndexSearcher", query: Query, collector: TermsCollector, max_buckets: int = 4096,
                            manager: Optional[TopScoreDocCollectorManager] = None) -> bool:
    """The eligibility predicate alone (nrtgpu_count_terms64_supported)."""
    m, tc, _ = _marshal_terms64(searcher, [query], [collector], max_buckets, None if manager is None else [manager])
    return _supported(_lib.load().nrtgpu_count_terms64_supported(searcher.ctx._h, searcher._segs, len(searcher.leaves), m.queries, tc))


def count_docset_terms64_batch(searcher: "GpuIndexSearcher", docsets: Sequence[DocSetQuery], collectors: Sequence[TermsCollector], max_buckets=4096,
                               managers: Optional[Sequence[TopScoreDocCollectorManager]] = None) -> List[TermCounts64]:
    """Terms aggregations over 64-bit columns and doc sets (nrtgpu_count_docset_terms64_batch)."""
    n = len(docsets)
    tc, bounds = _terms64(collectors, max_buckets, n)
    ds, keep = _marshal_docsets(docsets, list(managers) if managers is not None else [TopScoreDocCollectorManager(1)] * n)
    h = _TermOutputs64(bounds)
    _lib.check(_lib.load().nrtgpu_count_docset_terms64_batch(searcher.ctx._h, searcher._segs, searcher._bases, len(searcher.leaves), ds, tc, n, h.outs))
    del keep
    return h.lists(collectors)


def count_docset_terms64_supported(searcher: "GpuIndexSearcher", docset: DocSetQuery, collector: TermsCollector, max_buckets: int = 4096,
                                   manager: Optional[TopScoreDocCollectorManager] = None) -> bool:
    """The eligibility predicate alone (nrtgpu_count_docset_terms64_supported)."""
    tc, _ = _terms64([collector], max_buckets, 1)
    ds, keep = _marshal_docsets([docset], [manager if manager is not None else TopScoreDocCollectorManager(1)])
    rc = _lib.load().nrtgpu_count_docset_terms64_supported(searcher.ctx._h, searcher._segs, len(searcher.leaves), ds, tc)
    del keep
    return _supported(rc)


def terms_home_slots64(kind: str, value_bits: int, max_buckets: int) -> Tuple[int, int]:
    """The home slots of a value in a workgroup's count table and in a query's table of max_buckets (nrtgpu_terms_home_slots64:
    the function the kernels compile).  No device."""
    lds, table = C.c_uint32(0), C.c_uint32(0)
    _lib.check(_lib.load().nrtgpu_terms_home_slots64(DOC_VALUE_KINDS64[kind][0], C.c_uint64(int(value_bits)), int(max_buckets), C.byref(lds), C.byref(table)))
    return int(lds.value), int(table.value)


# ---- numeric range facets: a query's hits counted per requested value range (all four single-valued kinds) -----------------------
ALL_DOC_VALUE_KINDS = {**DOC_VALUE_KINDS, **DOC_VALUE_KINDS64}
_INT_LIMITS = {"int": (-2**31, 2**31 - 1), "long": (-2**63, 2**63 - 1)}


def _any_value_bits(kind: str, value) -> int:
    return _value_bits64(kind, value) if kind in DOC_VALUE_KINDS64 else _value_bits(kind, value)


@dataclasses.dataclass(frozen=True)
class NumericRange:
    """One NumericRangeType of a Facet.numericRange request (search.proto:1285-1327): label, min, minInclusive, max, maxInclusive;
    min and max are the proto's int64.  bounds(kind) restates the constructors of LongRange (INT / LONG fields) and DoubleRange
    (DOUBLE fields) [Lucene-recall: read from memory of Lucene 10, never from a run]: it yields the INCLUSIVE bounds the device call
    takes."""

    label: str
    min: Union[int, float]
    min_inclusive: bool
    max: Union[int, float]
    max_inclusive: bool

    def bounds(self, kind: str) -> Tuple[Union[int, float], Union[int, float]]:
        """-> (lower, upper), both inclusive, values of the kind.  ValueError where the reference's constructor throws: an exclusive
        bound at the type's extreme (LongRange), a NaN bound (DoubleRange), min > max after the adjustment.  An INT field's bounds
        are longs in the reference; what lies outside int32 is cut to it here (a range no int lies in comes back as the empty (1, 0)).
        "float" has no counterpart in the reference (it refuses FLOAT fields): DoubleRange's rule in float32 steps."""
        if kind not in ALL_DOC_VALUE_KINDS:
            raise UnsupportedQuery(f"a numeric range over a column of kind {kind!r}")
        if kind in _INT_LIMITS:
            lo, hi = int(self.min), int(self.max)
            if not self.min_inclusive:
                if lo == 2**63 - 1:
                    raise ValueError(f"range {self.label!r}: an exclusive min at Long.MAX_VALUE matches nothing")
                lo += 1
            if not self.max_inclusive:
                if hi == -2**63:
                    raise ValueError(f"range {self.label!r}: an exclusive max at Long.MIN_VALUE matches nothing")
                hi -= 1
            if lo > hi:
                raise ValueError(f"range {self.label!r}: min {lo} > max {hi}")
            least, greatest = _INT_LIMITS[kind]
            lo, hi = max(lo, least), min(hi, greatest)
            return (lo, hi) if lo <= hi else (1, 0)
        dt = np.float64 if kind == "double" else np.float32
        lo, hi = dt(self.min), dt(self.max)   # (the proto's int64 widened, as Java's implicit conversion does)
        if np.isnan(lo) or np.isnan(hi):
            raise ValueError(f"range {self.label!r}: a NaN bound")
        if not self.min_inclusive:
            lo = np.nextafter(lo, dt(np.inf))      # Math.nextUp
        if not self.max_inclusive:
            hi = np.nextafter(hi, dt(-np.inf))     # Math.nextDown
        if lo > hi:
            raise ValueError(f"range {self.label!r}: min {lo} > max {hi}")
        return float(lo), float(hi)


@dataclasses.dataclass(frozen=True)
class RangeCounter:
    """A numeric range facet over the single-valued doc value column `field` of kind `kind` ("int", "float", "long", "double").
    ranges: NumericRange records, or (lower_bits, upper_bits) pairs -- the inclusive bounds as bits of the kind, what the C call
    takes (lower above upper in the kind's order: an empty range, counted as 0).  topN, labels and the order of the result stay
    with the caller."""

    field: int
    kind: str
    ranges: Tuple[Union[NumericRange, Tuple[int, int]], ...]


@dataclasses.dataclass
class RangeCounts:
    """The facet of one query (nrtgpu_range_counts): hits per range in request order; hits_with_value is the reference's totCount
    behind FacetResult.value."""

    counts: np.ndarray          # int64
    total_hits: int
    hits_with_value: int


def _marshal_range_counters(counters: Sequence[RangeCounter]):
    """nrtgpu_range_count per query, the outputs, and what keeps the arrays alive."""
    n = len(counters)
    rc = (_lib.RangeCount * n)()
    outs = (_lib.RangeCounts * n)()
    width = max([max(len(c.ranges), 1) for c in counters], default=1)
    counts = np.zeros((n, width), dtype=np.int64)
    keep: list = [rc, outs, counts]
    for qi, c in enumerate(counters):
        if c.kind not in ALL_DOC_VALUE_KINDS:
            raise UnsupportedQuery(f"a range counter of kind {c.kind!r}")
        vr = (_lib.ValueRange * max(len(c.ranges), 1))()
        for i, r in enumerate(c.ranges):
            if isinstance(r, NumericRange):
                lo, hi = r.bounds(c.kind)
                vr[i] = _lib.ValueRange(_any_value_bits(c.kind, lo), _any_value_bits(c.kind, hi))
            else:
                vr[i] = _lib.ValueRange(int(r[0]), int(r[1]))
        keep.append(vr)
        rc[qi] = _lib.RangeCount(int(c.field), len(c.ranges), vr)
        outs[qi].counts = C.cast(counts.ctypes.data + qi * width * 8, C.POINTER(C.c_int64))
        outs[qi].capacity = width
    return rc, outs, counts, keep


def _range_counts(counters, outs, counts) -> List[RangeCounts]:
    return [RangeCounts(counts[qi, : len(c.ranges)].copy(), int(o.total_hits), int(o.hits_with_value)) for qi, (c, o) in enumerate(zip(counters, outs))]


def _marshal_range_queries(searcher: "GpuIndexSearcher", queries: Sequence[Query], counters: Sequence[RangeCounter], managers):
    if len(counters) != len(queries):
        raise ValueError(f"{len(counters)} range counters for {len(queries)} queries")
    mgrs = list(managers) if managers is not None else [TopScoreDocCollectorManager(1)] * len(queries)
    return _marshal_counted(searcher, queries, mgrs)


def count_ranges_batch(searcher: "GpuIndexSearcher", queries: Sequence[Query], counters: Sequence[RangeCounter],
                       managers: Optional[Sequence[TopScoreDocCollectorManager]] = None) -> List[RangeCounts]:
    """Numeric range facets (nrtgpu_count_ranges_batch): per query the hits of queries[i] counted per range of counters[i].  The
    columns of one call must be of one width ("int" / "float", or "long" / "double").  No hits are returned."""
    m = _marshal_range_queries(searcher, queries, counters, managers)
    rc, outs, counts, keep = _marshal_range_counters(counters)
    _lib.check(_lib.load().nrtgpu_count_ranges_batch(searcher.ctx._h, searcher._segs, searcher._bases, len(searcher.leaves), m.queries, rc, len(queries), outs))
    del keep
    return _range_counts(counters, outs, counts)


def count_ranges_supported(searcher: "GpuIndexSearcher", query: Query, counter: RangeCounter, manager: Optional[TopScoreDocCollectorManager] = None) -> bool:
    """The eligibility predicate alone (nrtgpu_count_ranges_supported)."""
    m = _marshal_range_queries(searcher, [query], [counter], None if manager is None else [manager])
    rc, _, _, keep = _marshal_range_counters([counter])
    r = _lib.load().nrtgpu_count_ranges_supported(searcher.ctx._h, searcher._segs, len(searcher.leaves), m.queries, rc)
    del keep
    return _supported(r)


def count_docset_ranges_batch(searcher: "GpuIndexSearcher", docsets: Sequence[DocSetQuery], counters: Sequence[RangeCounter],
                              managers: Optional[Sequence[TopScoreDocCollectorManager]] = None) -> List[RangeCounts]:
    """Numeric range facets over doc sets (nrtgpu_count_docset_ranges_batch): count_ranges_batch's results over a hit set without
    a text clause."""
    if len(counters) != len(docsets):
        raise ValueError(f"{len(counters)} range counters for {len(docsets)} queries")
    ds, dkeep = _marshal_docsets(docsets, list(managers) if managers is not None else [TopScoreDocCollectorManager(1)] * len(docsets))
    rc, outs, counts, keep = _marshal_range_counters(counters)
    _lib.check(_lib.load().nrtgpu_count_docset_ranges_batch(searcher.ctx._h, searcher._segs, searcher._bases, len(searcher.leaves), ds, rc, len(docsets), outs))
    del keep, dkeep
    return _range_counts(counters, outs, counts)


def count_docset_ranges_supported(searcher: "GpuIndexSearcher", docset: DocSetQuery, counter: RangeCounter,
                                  manager: Optional[TopScoreDocCollectorManager] = None) -> bool:
    """The eligibility predicate alone (nrtgpu_count_docset_ranges_supported)."""
    ds, dkeep = _marshal_docsets([docset], [manager if manager is not None else TopScoreDocCollectorManager(1)])
    rc, _, _, keep = _marshal_range_counters([counter])
    r = _lib.load().nrtgpu_count_docset_ranges_supported(searcher.ctx._h, searcher._segs, len(searcher.leaves), ds, rc)
    del keep, dkeep
    return _supported(r)


def range_cuts(kind: str, ranges: Sequence[Tuple[int, int]]) -> List[int]:
    """The cut points, as codes of the kind, of a list of (lower_bits, upper_bits) ranges (nrtgpu_range_cuts: the function the host
    plans with).  No device."""
    n = len(ranges)
    vr = (_lib.ValueRange * max(n, 1))(*[_lib.ValueRange(int(lo), int(hi)) for lo, hi in ranges])
    out = (C.c_uint64 * (2 * _lib.NRTGPU_MAX_COUNT_RANGES))()
    n_cuts = C.c_int32(0)
    _lib.check(_lib.load().nrtgpu_range_cuts(ALL_DOC_VALUE_KINDS[kind][0], vr, n, out, C.byref(n_cuts)))
    return [int(out[i]) for i in range(n_cuts.value)]


def range_interval(kind: str, cuts: Sequence[int], value_bits: int) -> int:
    """The elementary interval of a value among cut points: the number of cuts <= its code (nrtgpu_range_interval: the search the
    kernels compile).  No device."""
    arr = (C.c_uint64 * max(len(cuts), 1))(*[int(c) for c in cuts])
    out = C.c_int32(0)
    _lib.check(_lib.load().nrtgpu_range_interval(ALL_DOC_VALUE_KINDS[kind][0], arr, len(cuts), C.c_uint64(int(value_bits)), C.byref(out)))
    return int(out.value)


def debug_knn_bounds(sim: int, dim: int, q_norm2: float, q_l1: float, q_absmax: float, nv_max: float, nv_min: float,
                     rows_absmax: float, score_boost: float = 1.0, m: float = 0.0, s: float = 0.0) -> dict:
    """Test hook of the development library (nrtgpu_debug_knn_bounds): the rounding bounds the exact float vector search certifies
    its answers with, from the library's own code; `dim` is the resident dimension (a multiple of 16).  No context, no device."""
    out = np.zeros(10, dtype=np.float64)
    _lib.check(_lib.load().nrtgpu_debug_knn_bounds(int(sim), int(dim), float(q_norm2), float(q_l1), C.c_float(q_absmax), float(nv_max),
                                                   float(nv_min), C.c_float(rows_absmax), C.c_float(score_boost), float(m), float(s),
                                                   out.ctypes.data))
    names = ("e32", "e16", "result_upper32", "result_upper16", "estimate_lower32", "estimate_lower16", "q_scale", "rows_scale")
    d = {n: float(out[i]) for i, n in enumerate(names)}
    d["q_scale_usable"], d["rows_scale_usable"] = bool(out[8]), bool(out[9])
    return d


def debug_wave_kth(keys: np.ndarray, r: int) -> int:
    """Test hook of the development library (nrtgpu_debug_wave_kth): the r-th largest (1-based) of the packed 64-bit keys as ONE
    wave selects it (topk.hiph: topk_kth_wave -- the MaxScore walk's estimator); a zero key is an unwritten slot."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    out = np.zeros(1, dtype=np.uint64)
    _lib.check(_lib.load().nrtgpu_debug_wave_kth(keys.ctypes.data, len(keys), int(r), out.ctypes.data))
    return int(out[0])


# one walk row (csrc/plan.h: DWalkRow), as nrtgpu_debug_walk_rows returns it
WALK_ROW_DTYPE = np.dtype([("docids", "<u8"), ("fnorm", "<u8"), ("suffix", "<u8"), ("ub", "<u8"), ("weight", "<f4"), ("fx_scale", "<i4"),
                           ("flags", "<u4"), ("pad", "<u4"), ("u_after", "<u8"), ("look", "<u8"), ("cells", "<u8"), ("start", "<u8")])
assert WALK_ROW_DTYPE.itemsize == 80


def debug_walk_value(weight: float, freqs, norm_bytes, table256: np.ndarray, fx_scale: int, fx_shift: int) -> np.ndarray:
    """Test hook of the development library (nrtgpu_debug_walk_value): what a posting of (freq, norm byte) adds to a doc's
    fixed-point sum, computed on the device by the statement the scorers use -- one uint64 per (freq, norm byte) pair."""
    f = np.ascontiguousarray(freqs, dtype=np.uint32)
    nb = np.ascontiguousarray(norm_bytes, dtype=np.uint32)
    tab = np.ascontiguousarray(table256, dtype=np.float32)
    assert f.shape == nb.shape and f.ndim == 1 and tab.shape == (256,)
    out = np.zeros(len(f), dtype=np.uint64)
    _lib.check(_lib.load().nrtgpu_debug_walk_value(C.c_float(float(weight)), f.ctypes.data, nb.ctypes.data, len(f), tab.ctypes.data, int(fx_scale),
                                                  int(fx_shift), out.ctypes.data))
    return out


def blend(retriever_docs: Sequence[np.ndarray], retriever_scores: Optional[Sequence[np.ndarray]] = None,
          boosts: Optional[Sequence[float]] = None, mode: str = "rrf", k: int = 60, start_hit: int = 0, top_hits: int = 10) -> TopDocs:
    """BlenderOperation.blend through the library (nrtgpu_blend): weighted RRF or score order, ties in the reference's order."""
    n = len(retriever_docs)
    docs = [np.ascontiguousarray(d, dtype=np.int32) for d in retriever_docs]
    scs = [np.ascontiguousarray(s_, dtype=np.float32) for s_ in retriever_scores] if retriever_scores is not None else None
    dp = (C.c_void_p * max(n, 1))(*[d.ctypes.data for d in docs])
    sp = (C.c_void_p * max(n, 1))(*[s_.ctypes.data for s_ in scs]) if scs is not None else None
    counts = np.asarray([len(d) for d in docs], dtype=np.int32)
    b = np.ascontiguousarray(boosts, dtype=np.float32) if boosts is not None else None
    h = _outputs(1, max(int(top_hits), 1))
    _lib.check(_lib.load().nrtgpu_blend(n, dp, sp, counts.ctypes.data, b.ctypes.data if b is not None else None,
                                        0 if mode == "rrf" else 1, int(k), int(start_hit), int(top_hits), h.outs))
    return h.topdocs(0)


# ---- blenders (multi-retriever; O(k) host work that stays in Java in the reference) ----------------
def weighted_rrf_blend(retriever_hits: Sequence[np.ndarray], boosts: Optional[Sequence[float]] = None, k: int = 60,
                       start_hit: int = 0, top_hits: int = 10) -> TopDocs:
    """WeightedRrfBlenderOperation.mergeHits + BlenderOperation.sortAndPaginate
    (S/search/multiretriever/blender/operation/WeightedRrfBlenderOperation.java:53-78,
    .../score/WeightedRRFScoreDoc.java:62,75): score(doc) = sum over retrievers of boost / (k + rank),
    rank 1-based, accumulated in fp32 in retriever declaration order.  Equal scores are returned in
    docid order here (the reference leaves ties to its heap's order)."""
    if k < 1:
        raise ValueError(f"k must be >= 1, got: {k}")
    if top_hits == 0 or start_hit > top_hits:
        return TopDocs(np.zeros(0, np.int32), np.zeros(0, np.float32), 0, True)
    merged: Dict[int, np.float32] = {}
    for ri, docs in enumerate(retriever_hits):
        w = np.float32(1.0 if boosts is None else boosts[ri])
        for i, doc in enumerate(np.asarray(docs).tolist()):
            contrib = np.float32(w / np.float32(k + i + 1))
            merged[doc] = np.float32(merged[doc] + contrib) if doc in merged else contrib
    order = sorted(merged.items(), key=lambda kv: (-float(kv[1]), kv[0]))[: min(top_hits, len(merged))]
    page = order[min(start_hit, len(order)):]
    return TopDocs(np.asarray([d for d, _ in page], np.int32), np.asarray([s for _, s in page], np.float32),
                   len(merged), True)
