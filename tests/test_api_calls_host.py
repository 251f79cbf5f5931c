"""What nrtsearch_amd/api.py hands the library and what it gives back to its caller, recorded.

A pure-Python recorder stands in for libnrtgpu.so (no built library, no GPU): every public method of GpuIndexSearcher, PreparedBatch
and PreparedMerge that ends in a library call is driven with the smallest inputs that tell the cases apart, and the recorded calls --
entry, scalars, which pointers are NULL, the pointees, every output element's capacity -- and the returned TopDocs are compared with
tests/golden/api_calls.json, which the same recorder wrote from the api.py BEFORE the binding got one output holder and one call path
per entry kind (tests/golden/README.md).  After every case the call is made again with other answers: what the first call returned
must not change, i.e. nothing handed to a caller aliases an output array the binding keeps.

    python tests/test_api_calls_host.py OUT.json     writes the record of the nrtsearch_amd package on sys.path
"""
import ctypes as C
import hashlib
import inspect
import json
import os
import re
import sys
import types

import numpy as np
import pytest

from nrtsearch_amd import _lib, api

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "api_calls.json")

# ---- the C ABI as the recorder reads it: name:kind per argument ---------------------------------------------------------------------
# h handle, S segment handles, B doc bases, i / f scalars, d device address, p pointer (NULL or not), H handle out, N int out,
# Q / F / G / K arrays of nrtgpu_bm25_query / _function_score / _clause_groups / _knn_clauses (n elements, 1 without an n),
# O nrtgpu_topdocs (n or nq elements; O1: one, by reference or as an array of one), <dtype>[<count>] host array whose size follows from the call's scalars
HEAD = "ctx:h segs:S bases:B n_segs:i "
KNN = HEAD + "field:i sim:i "
DEVICE = HEAD + "queries:Q n:i k_stride:i d_keys:d d_counts:d d_hits:d "
SIGNATURES = {
    "nrtgpu_search_bm25_batch": HEAD + "queries:Q n:i outs:O",
    "nrtgpu_search_function_score_batch": HEAD + "queries:Q fs:F n:i outs:O",
    "nrtgpu_search_multi_match_batch": HEAD + "queries:Q gs:G n:i outs:O",
    "nrtgpu_search_function_score_multi_match_batch": HEAD + "queries:Q gs:G fs:F n:i outs:O",
    "nrtgpu_search_text_knn_batch": HEAD + "queries:Q kc:K n:i outs:O",
    "nrtgpu_dist_search_bm25_batch_mode": HEAD + "queries:Q n:i mode:i outs:O",
    "nrtgpu_search_bm25_coalesced": HEAD + "queries:Q outs:O1",
    "nrtgpu_query_supported": "ctx:h segs:S n_segs:i queries:Q",
    "nrtgpu_function_score_supported": "ctx:h segs:S n_segs:i queries:Q fs:F",
    "nrtgpu_multi_match_supported": "ctx:h segs:S n_segs:i queries:Q gs:G",
    "nrtgpu_function_score_multi_match_supported": "ctx:h segs:S n_segs:i queries:Q gs:G fs:F",
    "nrtgpu_text_knn_supported": "ctx:h segs:S n_segs:i queries:Q kc:K",
    "nrtgpu_debug_walk_rows": HEAD + "queries:Q n:i begin:p count:p rows:p total:i",
    "nrtgpu_knn_exact": KNN + "qv:f4[nq*dim] nq:i dim:i k:i boost:f outs:O",
    "nrtgpu_knn_exact_bytes": KNN + "qv:i1[nq*dim] nq:i dim:i k:i boost:f outs:O",
    "nrtgpu_dist_knn_exact": KNN + "qv:f4[nq*dim] nq:i dim:i k:i boost:f mode:i outs:O",
    "nrtgpu_knn_search": KNN + "qv:f4[nq*dim] nq:i dim:i k:i boost:f mask:i min_score:f outs:O",
    "nrtgpu_knn_search_bytes": KNN + "qv:i1[nq*dim] nq:i dim:i k:i boost:f mask:i min_score:f outs:O",
    "nrtgpu_knn_search_requests": KNN + "qv:f4[nq*dim] nq:i dim:i ks:i4[nq] boosts:f4[nq] masks:i4[nq] min_scores:f4[nq] outs:O",
    "nrtgpu_knn_search_bytes_requests": KNN + "qv:i1[nq*dim] nq:i dim:i ks:i4[nq] boosts:f4[nq] masks:i4[nq] min_scores:f4[nq] outs:O",
    "nrtgpu_knn_exact_coalesced": KNN + "qv:f4[dim] dim:i k:i boost:f outs:O1",
    "nrtgpu_knn_exact_bytes_coalesced": KNN + "qv:i1[dim] dim:i k:i boost:f outs:O1",
    "nrtgpu_knn_search_coalesced": KNN + "qv:f4[dim] dim:i k:i boost:f mask:i min_score:f outs:O1",
    "nrtgpu_knn_search_bytes_coalesced": KNN + "qv:i1[dim] dim:i k:i boost:f mask:i min_score:f outs:O1",
    "nrtgpu_knn_exact_relation": HEAD + "field:i k:i threshold:i",
    "nrtgpu_rescore_vectors": KNN + "qv:f4[dim] dim:i boost:f docs:i4[n_hits] scores:f4[n_hits] n_hits:i query_weight:f rescore_weight:f window:i outs:O1",
    "nrtgpu_rescore_byte_vectors": KNN + "qv:i1[dim] dim:i boost:f docs:i4[n_hits] scores:f4[n_hits] n_hits:i query_weight:f rescore_weight:f window:i outs:O1",
    "nrtgpu_search_hybrid_batch": HEAD + "queries:Q n:i field:i sim:i qv:f4[n*dim] dim:i boost:f query_weight:f rescore_weight:f window:i outs:O",
    "nrtgpu_search_hybrid_bytes_batch": HEAD + "queries:Q n:i field:i sim:i qv:i1[n*dim] dim:i boost:f query_weight:f rescore_weight:f window:i outs:O",
    "nrtgpu_dist_search_hybrid_batch": HEAD + "queries:Q n:i field:i sim:i qv:f4[n*dim] dim:i boost:f query_weight:f rescore_weight:f window:i mode:i outs:O",
    "nrtgpu_search_bm25_batch_device_epoch": DEVICE + "epoch:i",
    "nrtgpu_search_bm25_batch_device_begin": DEVICE + "epoch:i pending:H",
    "nrtgpu_search_bm25_shard_device_begin": DEVICE + "spec_world:i d_guess:d pending:H",
    "nrtgpu_note_shard_speculation": "ctx:h segs:S n_segs:i n_queries:i n_failed:i",
    "nrtgpu_pending_wait": "pending:d",
    "nrtgpu_merge_topk_device": "ctx:h n_lists:i n:i k_stride:i d_keys:d d_counts:d d_hits:d ks:i4[n] thresholds:i4[n] outs:O",
    "nrtgpu_dist_exchange_merge": "ctx:h n:i k_stride:i d_keys:d d_counts:d d_hits:d ks:i4[n] thresholds:i4[n] mode:i outs:O",
    "nrtgpu_dist_exchange_merge_checked": "ctx:h n:i k_stride:i d_keys:d d_counts:d d_hits:d d_guess:d ks:i4[n] thresholds:i4[n] mode:i outs:O failed:u1[n] n_failed:N",
    "nrtgpu_blend": "n:i docs:p scores:p counts:i4[n] boosts:f4[n] mode:i k:i start_hit:i top_hits:i outs:O1",
}
# how many elements a pointer field of a record addresses (the record, the nrtgpu_bm25_query beside it)
FIELD_COUNTS = {
    ("Bm25Query", "terms"): lambda r, q: r.n_terms, ("Bm25Query", "norm_cache"): lambda r, q: 256 * r.n_caches,
    ("Bm25Query", "more_filters"): lambda r, q: r.n_more_filters, ("Bm25Query", "more_must_not"): lambda r, q: r.n_more_must_not,
    ("FunctionScore", "functions"): lambda r, q: r.n_functions,
    ("ClauseGroups", "group_of_term"): lambda r, q: q.n_terms, ("ClauseGroups", "group_min_should_match"): lambda r, q: r.n_groups,
    ("KnnClauses", "lists"): lambda r, q: r.n_lists, ("DocScores", "docs"): lambda r, q: r.n, ("DocScores", "scores"): lambda r, q: r.n,
}
DTYPES = {"f4": np.float32, "i4": np.int32, "i1": np.int8, "u1": np.uint8}


def digest(raw: bytes) -> str:
    return hashlib.sha256(raw).hexdigest()[:16]


def record_of(r, query=None):
    """A ctypes record with what its pointers address: short arrays as lists, long ones as a hash of their bytes."""
    out = {}
    for name, _ in r._fields_:
        v = getattr(r, name)
        if isinstance(v, (int, float)):
            out[name] = v
        elif not v:
            out[name] = None
        else:
            n = FIELD_COUNTS[type(r).__name__, name](r, query)
            if hasattr(v._type_, "_fields_"):
                out[name] = [record_of(e) for e in v[:n]]
            else:
                out[name] = v[:n] if n <= 16 else digest(C.string_at(v, n * C.sizeof(v._type_)))
    return out


class Recorder:
    """Stands in for the loaded library: every entry of SIGNATURES is a callable that records its call and fills its outputs."""

    def __init__(self):
        self.calls, self.rc, self.salt, self.recording = [], {}, 0, True

    # what the marshalling reads from the library on its way: not recorded
    @staticmethod
    def nrtgpu_last_error():
        return b"the recorder's error"

    @staticmethod
    def nrtgpu_bm25_idf(doc_count, doc_freq):
        return float(np.float32(1.0 + doc_freq / (doc_count + 1.0)))

    @staticmethod
    def nrtgpu_bm25_avgdl(sum_total_term_freq, doc_count):
        return float(np.float32(sum_total_term_freq / doc_count))

    @staticmethod
    def nrtgpu_bm25_norm_cache(avgdl, k1, b, out):
        np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_float)), (256,))[:] = np.arange(256, dtype=np.float32) * np.float32(avgdl.value)

    def __getattr__(self, entry):
        if entry not in SIGNATURES:
            raise AttributeError(entry)
        return lambda *args: self._call(entry, args)

    def _call(self, entry, args):
        spec = [a.split(":") for a in SIGNATURES[entry].split()]
        assert len(args) == len(spec), (entry, len(args), len(spec))
        scalars = {}
        for (name, kind), a in zip(spec, args):
            if kind == "i":
                assert isinstance(a, int), (entry, name, a)
                scalars[name] = a
            elif kind == "f":
                scalars[name] = a.value if isinstance(a, (C.c_float, C.c_double)) else float(a)
        n = scalars.get("n", scalars.get("nq", 1))
        queries = next((a for (_, kind), a in zip(spec, args) if kind == "Q"), None)
        rec, outs = {"entry": entry}, []
        for (name, kind), a in zip(spec, args):
            if kind in "if":
                rec[name] = scalars[name]
            elif kind in "hd":
                rec[name] = a.value
            elif kind in "SB":
                rec[name] = list(a)
            elif kind == "p":
                rec[name] = "NULL" if a is None else "set"
            elif kind in "HN":
                a._obj.value = 0x7000 + len(self.calls) if kind == "H" else 1
            elif kind in "QFGK":
                assert len(a) >= n, (entry, name)
                rec[name] = [record_of(a[i], queries[i]) for i in range(n)]
            elif kind in ("O", "O1"):
                count = n if kind == "O" else 1
                assert hasattr(a, "_obj") or len(a) >= count, (entry, name)
                outs = [a._obj] if hasattr(a, "_obj") else [a[i] for i in range(count)]
                rec[name] = [[o.capacity, bool(o.docs), bool(o.scores)] for o in outs]
            else:
                dtype, count = re.fullmatch(r"(\w\d)\[(.+)\]", kind).groups()
                if a is None:
                    rec[name] = None
                else:
                    count = eval(count, {}, scalars)
                    rec[name] = digest(C.string_at(a, count * np.dtype(DTYPES[dtype]).itemsize))
                    if name == "failed":
                        C.memset(a + count - 1, 1, 1)
        if self.recording:
            self.calls.append(rec)
        rc = self.rc.get(entry, 0)
        if rc == 0:
            for qi, o in enumerate(outs):
                o.n_hits = max(min(o.capacity, 3), 0)
                for j in range(o.n_hits):
                    o.docs[j] = 100 * qi + j + self.salt
                    o.scores[j] = qi + 0.5 - 0.125 * j + self.salt
                o.total_hits = -1 if (entry.startswith("nrtgpu_dist_") and qi & 1) else 10 + qi + self.salt
                o.total_hits_is_lower_bound = qi & 1
        return rc


def plain(v):
    """What a method returned, as JSON holds it."""
    if isinstance(v, api.TopDocs):
        assert v.docs.dtype == np.int32 and v.scores.dtype == np.float32
        return {"docs": v.docs.tolist(), "scores": v.scores.tolist(), "total_hits": v.total_hits, "relation_gte": v.relation_gte}
    if isinstance(v, (list, tuple)):
        return [plain(x) for x in v]
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, np.generic):
        return v.item()
    return v


def drive(rec):
    """Every case -- {"case", "calls", "result" or "raises"} -- in order; rec is what _lib.load() returns meanwhile."""
    def case(name, fn, again=True):
        rec.calls = []
        try:
            got = fn()
        except Exception as e:   # the type and the text are part of the record
            return {"case": name, "calls": rec.calls, "raises": [type(e).__name__, str(e)]}
        out = {"case": name, "calls": rec.calls, "result": plain(got)}
        if again:   # the same call with other answers: what the first one returned stays as it was
            rec.salt, rec.recording = 1000, False
            try:
                fn()
            finally:
                rec.salt, rec.recording = 0, True
            assert plain(got) == out["result"], f"{name}: the result changed with the next call of the same shape"
        return out

    T, B, MF, M = api.TermQuery, api.BoostQuery, api.MaskFilter, api.TopScoreDocCollectorManager
    stats = api.IndexStatistics()
    stats.fields[0], stats.fields[1] = api.CollectionStatistics(1000, 50000), api.CollectionStatistics(900, 18000)
    stats.doc_freq.update({(0, 1): 10, (0, 2): 20, (0, 3): 5, (1, 1): 7, (1, 2): 9})
    ctx = types.SimpleNamespace(_h=C.c_void_p(0x1000))
    leaves = [types.SimpleNamespace(_h=C.c_void_p(0x2000 + 16 * i), doc_base=500 * i) for i in range(2)]
    sr1, sr = api.GpuIndexSearcher(ctx, leaves[:1], stats), api.GpuIndexSearcher(ctx, leaves, stats)

    queries = [api.BooleanQuery((T(0, 1), B(T(1, 2), 2.0))), T(0, 3),
               api.BooleanQuery((T(0, 1), T(0, 2)), 1, (MF(3), MF(4)), (MF(5),))]
    managers = [M(5), M(1, after=api.ScoreDoc(7, 1.5), total_hits_threshold=10), M(0, min_competitive_score=0.25)]
    dismax = api.DisjunctionMaxQuery((T(0, 1), T(1, 1)), 0.3)
    fsq = [api.FunctionScoreQuery(queries[0], (api.WeightFunction(2.0, 3), api.WeightFunction(0.5)), "sum", "replace", 0.5, True),
           api.FunctionScoreQuery(queries[1])]
    mmq = [api.MultiMatchQuery("cross_fields", ((T(0, 1), T(1, 1)), (T(0, 2),)), "should", 1, 0.2, (MF(3),)),
           api.MultiMatchQuery("best_fields", ((T(0, 1), T(0, 2)), (T(1, 1),)), "should", (1, 0), 0.1)]
    fsmm = [api.FunctionScoreQuery(mmq[0], (api.WeightFunction(3.0, 4),)), api.FunctionScoreQuery(mmq[1], (), "multiply", "sum")]
    clauses = [[api.KnnClause(np.array([3, 9]), np.array([0.5, 0.25]), 2.0)], [], [api.KnnClause(np.zeros(0), np.zeros(0))]]

    yield case("search_batch", lambda: sr.search_batch(queries, managers))
    yield case("search_batch/one leaf", lambda: sr1.search_batch(queries[:2], managers[:2]))
    yield case("search_batch/dismax", lambda: sr.search_batch([dismax, api.BooleanQuery((T(0, 2),), must=(T(0, 1),))], managers[:2]))
    yield case("search_batch/unsupported", lambda: sr.search_batch([api.BooleanQuery()], managers[:1]))
    yield case("search", lambda: sr.search(queries[0], managers[0]))
    yield case("search_function_score_batch", lambda: sr.search_function_score_batch(fsq, managers[:2]))
    yield case("search_text_knn_batch", lambda: sr.search_text_knn_batch(queries, clauses, managers))
    yield case("search_text_knn_batch/count", lambda: sr.search_text_knn_batch(queries, clauses[:2], managers))
    yield case("search_with_knn", lambda: sr.search_with_knn(queries[0], managers[0], [(5, "cosine", [1.0, 2.0, 2.0, 4.0], 2, 1.5, MF(3)),
                                                                                    (5, "cosine", [0.0, 1.0, 0.0, 0.0], 1, 1.0, None),
                                                                                    (6, "normalized_cosine", [3.0, 6.0, 6.0, 12.0], 3, 2.0, None)]))
    yield case("search_multi_match_batch", lambda: sr.search_multi_match_batch(mmq, managers[:2]))
    yield case("search_function_score_multi_match_batch", lambda: sr.search_function_score_multi_match_batch(fsmm, managers[1:]))
    yield case("debug_walk_rows", lambda: (rec.rc.update(nrtgpu_debug_walk_rows=2), sr.debug_walk_rows(queries[:2], managers[:2]))[1][:2], again=False)
    rec.rc.clear()
    yield case("dist_search_batch", lambda: sr.dist_search_batch(queries, managers, api.EXCHANGE_ALLTOALL | api.EXCHANGE_NO_SPECULATION))
    yield case("search_coalesced", lambda: sr.search_coalesced(queries[2], managers[0]))
    yield case("search_coalesced/num_hits 0", lambda: sr1.search_coalesced(queries[1], managers[2]))
    predicates = [("supported", "nrtgpu_query_supported", lambda: sr.supported(queries[2], managers[0])),
                  ("function_score_supported", "nrtgpu_function_score_supported", lambda: sr.function_score_supported(fsq[0], managers[0])),
                  ("text_knn_supported", "nrtgpu_text_knn_supported", lambda: sr.text_knn_supported(queries[2], clauses[0], managers[0])),
                  ("multi_match_supported", "nrtgpu_multi_match_supported", lambda: sr.multi_match_supported(mmq[1], managers[0])),
                  ("function_score_multi_match_supported", "nrtgpu_function_score_multi_match_supported",
                   lambda: sr.function_score_multi_match_supported(fsmm[0], managers[0]))]
    for name, entry, fn in predicates:
        for rc in (_lib.NRTGPU_OK, _lib.NRTGPU_ERR_UNSUPPORTED, _lib.NRTGPU_ERR_INVALID_ARG):
            rec.rc[entry] = rc
            yield case(f"{name}/rc {rc}", fn, again=False)
    for rc in (0, 1, _lib.NRTGPU_ERR_INVALID_ARG):
        rec.rc["nrtgpu_knn_exact_relation"] = rc
        yield case(f"knn_exact_relation/rc {rc}", lambda: sr.knn_exact_relation(5, 10), again=False)
    rec.rc.clear()

    # query vectors whose norms are exact in float32 whatever the order of the sum: the bytes sent do not depend on the BLAS at hand
    qf = np.array([[1.0, 2.0, 2.0, 4.0], [2.0, 4.0, 4.0, 8.0], [0.0, 3.0, 0.0, 4.0]], dtype=np.float32)
    qb = np.array([[1, -2, 3, -4], [127, -128, 0, 5], [9, 9, 9, 9]], dtype=np.int8)
    masks = [MF(3), None, MF(4)]
    for sim in ("cosine", "normalized_cosine"):
        yield case(f"knn_exact/{sim}", lambda: sr.knn_exact(5, sim, qf, 2, 1.5))
        yield case(f"knn_exact_coalesced/{sim}", lambda: sr.knn_exact_coalesced(5, sim, qf[1], 2, 0.5))
        yield case(f"knn_search/{sim}", lambda: sr.knn_search(5, sim, qf, 4, 2.0, MF(3), 0.25))
        yield case(f"knn_search_requests/{sim}", lambda: sr.knn_search_requests(5, sim, qf, [1, 5, 2], [1.0, 2.0, 0.5], masks, [0.0, 0.5, 0.25]))
        yield case(f"knn_search_coalesced/{sim}", lambda: sr.knn_search_coalesced(5, sim, qf[2], 3, 1.0, MF(4), 0.125))
        yield case(f"dist_knn_exact/{sim}", lambda: sr.dist_knn_exact(5, sim, qf, 2, 1.5, api.EXCHANGE_ALLTOALL))
    yield case("knn_exact/k 1, one query, one leaf", lambda: sr1.knn_exact(5, "l2_norm", qf[0], 1))
    yield case("knn_exact/k 0", lambda: sr.knn_exact(5, "dot_product", qf[:2], 0))
    yield case("knn_exact_coalesced/k 0", lambda: sr.knn_exact_coalesced(5, "max_inner_product", qf[0], 0))
    yield case("knn_search/defaults", lambda: sr.knn_search(5, "cosine", qf, 1))
    yield case("knn_search_requests/ks alone", lambda: sr.knn_search_requests(5, "cosine", qf, [2, 1, 3]))
    yield case("knn_search_requests/ks 0", lambda: sr.knn_search_requests(5, "cosine", qf[:2], [0, 0]))
    yield case("knn_search_requests/count", lambda: sr.knn_search_requests(5, "cosine", qf, [2, 1, 3], filters=masks[:2]))
    yield case("knn_search_coalesced/k 0", lambda: sr.knn_search_coalesced(5, "cosine", qf[0], 0))
    yield case("knn_exact_bytes", lambda: sr.knn_exact_bytes(6, "cosine", qb, 2, 1.5))
    yield case("knn_exact_bytes/normalized_cosine", lambda: sr.knn_exact_bytes(6, "normalized_cosine", qb, 2))
    yield case("knn_exact_bytes/float queries", lambda: sr.knn_exact_bytes(6, "cosine", qf, 2))
    yield case("knn_search_bytes", lambda: sr.knn_search_bytes(6, "l2_norm", qb, 4, 2.0, MF(3), 0.25))
    yield case("knn_search_bytes_requests", lambda: sr.knn_search_bytes_requests(6, "dot_product", qb, [1, 5, 2], [1.0, 2.0, 0.5], masks, [0.0, 0.5, 0.25]))
    yield case("knn_search_bytes_requests/ks alone", lambda: sr1.knn_search_bytes_requests(6, "dot_product", qb, [2, 1, 3]))
    yield case("knn_search_bytes_requests/count", lambda: sr.knn_search_bytes_requests(6, "dot_product", qb, [2, 1]))
    yield case("knn_search_bytes_coalesced", lambda: sr.knn_search_bytes_coalesced(6, "cosine", qb[1], 2, 1.5, MF(3), 0.5))
    yield case("knn_search_bytes_coalesced/k 0", lambda: sr.knn_search_bytes_coalesced(6, "cosine", qb[1], 0))
    yield case("knn_exact_bytes_coalesced", lambda: sr.knn_exact_bytes_coalesced(6, "max_inner_product", qb[2], 1, 2.0))
    yield case("knn_exact_bytes_coalesced/k 0", lambda: sr.knn_exact_bytes_coalesced(6, "cosine", qb[2], 0))

    hits = api.TopDocs(np.array([4, 8, 15], np.int32), np.array([3.0, 2.0, 1.0], np.float32), 42, True)
    for window in (0, 2):
        yield case(f"rescore_vectors/window {window}", lambda: sr.rescore_vectors(hits, 5, "cosine", qf[0], window, 0.5, 2.0, 1.5))
        yield case(f"rescore_byte_vectors/window {window}", lambda: sr.rescore_byte_vectors(hits, 6, "cosine", qb[0], window, 0.5, 2.0, 1.5))
        yield case(f"search_hybrid_batch/window {window}", lambda: sr.search_hybrid_batch(queries, managers, 5, "l2_norm", qf, window, 0.5, 2.0, 1.5))
        yield case(f"search_hybrid_bytes_batch/window {window}",
                   lambda: sr.search_hybrid_bytes_batch(queries, managers, 6, "l2_norm", qb, window, 0.5, 2.0, 1.5))
        yield case(f"dist_search_hybrid_batch/window {window}",
                   lambda: sr.dist_search_hybrid_batch(queries, managers, 5, "cosine", qf, window, 0.5, 2.0, 1.5, api.EXCHANGE_ALLTOALL))
    yield case("rescore_byte_vectors/two queries", lambda: sr.rescore_byte_vectors(hits, 6, "cosine", qb[:2], 2))
    yield case("search_hybrid_batch/count", lambda: sr.search_hybrid_batch(queries, managers, 5, "cosine", qf[:2], 2))
    yield case("dist_search_hybrid_batch/count", lambda: sr.dist_search_hybrid_batch(queries, managers, 5, "cosine", qf[:2], 2))

    pb = api.PreparedBatch(sr, queries, managers)
    assert (pb.n, pb.k, len(pb._outs), pb.docs.shape, pb.scores.shape, len(pb._m.queries)) == (3, 5, 3, (3, 5), (3, 5), 3)
    yield case("PreparedBatch.run", lambda: (pb.run(), [pb.topdocs(qi) for qi in range(pb.n)])[1])
    yield case("PreparedBatch.topdocs", lambda: (pb.run(), pb.topdocs(2))[1])
    yield case("PreparedBatch.run_device", lambda: pb.run_device(8, 0x100, 0x200, 0x300, 4), again=False)
    yield case("PreparedBatch.begin_device", lambda: pb.begin_device(8, 0x100, 0x200, 0x300), again=False)
    yield case("PreparedBatch.begin_shard_device", lambda: pb.begin_shard_device(8, 0x100, 0x200, 0x300, 2, 0x400), again=False)
    yield case("PreparedBatch.begin_shard_device/no guess", lambda: pb.begin_shard_device(8, 0x100, 0x200, 0x300, 0, 0), again=False)
    yield case("PreparedBatch.note_shard_speculation", lambda: pb.note_shard_speculation(3, 1), again=False)
    yield case("PreparedBatch.wait_device", lambda: api.PreparedBatch.wait_device(0x7001), again=False)
    pm = api.PreparedMerge(ctx, 2, 3, 8, [2, 5, 1], [1000, 10, 1000])
    assert (len(pm._outs), pm.docs.shape, pm.scores.shape) == (3, (3, 5), (3, 5))
    yield case("PreparedMerge.run", lambda: (pm.run(0x100, 0x200, 0x300), [pm.topdocs(qi) for qi in range(3)])[1])
    yield case("PreparedMerge.kth_keys", lambda: (pm.run(0x100, 0x200, 0x300), pm.kth_keys())[1])
    yield case("PreparedMerge.run_dist", lambda: (pm.run_dist(0x100, 0x200, 0x300, api.EXCHANGE_ALLTOALL), pm.topdocs(0))[1])
    yield case("PreparedMerge.owned", lambda: [pm.owned(qi) for qi in range(3)], again=False)
    yield case("PreparedMerge.run_dist_checked", lambda: (pm.run_dist_checked(0x100, 0x200, 0x300, 0x400), pm.topdocs(2)))
    yield case("PreparedMerge.topdocs", lambda: (pm.run(0x100, 0x200, 0x300), pm.topdocs(1))[1])
    yield case("merge_topk_device", lambda: api.merge_topk_device(ctx, 2, 2, 8, 0x100, 0x200, 0x300, [3, 1], [1000, 1000]))
    yield case("blend", lambda: api.blend([np.array([1, 2, 3]), np.array([3, 4])], [np.array([3.0, 2.0, 1.0]), np.array([5.0, 4.0])], [1.0, 2.0],
                                         "score", 60, 0, 2))
    yield case("blend/rrf, top_hits 0", lambda: api.blend([np.array([1, 2, 3])], top_hits=0))


@pytest.fixture(scope="module")
def driven():
    rec = Recorder()
    with pytest.MonkeyPatch.context() as monkeypatch:
        monkeypatch.setattr(_lib, "load", lambda: rec)
        return {c["case"]: c for c in drive(rec)}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return {c["case"]: c for c in json.load(f)["cases"]}


def test_the_calls_and_results_are_the_recorded_ones(driven, golden):
    assert list(driven) == list(golden)
    for name, want in golden.items():
        got = json.loads(json.dumps(driven[name]))
        for key in ("raises", "result", "calls"):
            assert got.get(key) == want.get(key), f"{name}: {key} differs from tests/golden/api_calls.json"


def test_every_public_method_is_driven(driven):
    names = {c.split("/")[0] for c in driven}
    for cls, prefix in ((api.GpuIndexSearcher, ""), (api.PreparedBatch, "PreparedBatch."), (api.PreparedMerge, "PreparedMerge.")):
        for method, _ in inspect.getmembers(cls, inspect.isfunction):
            assert method.startswith("_") or prefix + method in names, f"{cls.__name__}.{method} is not driven"


def test_the_refusals_keep_their_type_and_text(driven):
    assert driven["search_batch/unsupported"]["raises"] == ["UnsupportedQuery", "empty BooleanQuery"]
    assert driven["knn_search_requests/count"]["raises"] == ["ValueError", "filters: 2 values for 3 queries"]
    assert driven["knn_search_bytes_requests/count"]["raises"] == ["ValueError", "ks: 2 values for 3 queries"]
    assert driven["supported/rc -1"]["raises"] == ["NrtGpuError", "nrtgpu error -1: the recorder's error"]
    assert driven["supported/rc 0"]["result"] is True and driven["supported/rc -4"]["result"] is False
    assert driven["dist_search_batch"]["result"][1] is None and driven["dist_search_batch"]["result"][0] is not None


if __name__ == "__main__":
    recorder = Recorder()
    _lib.load = lambda: recorder
    with open(sys.argv[1], "w") as f:
        json.dump({"cases": list(drive(recorder))}, f, indent=0)
        f.write("\n")
