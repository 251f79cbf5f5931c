/*
 * nrtgpu_dev.h -- test hooks and measurement helpers of the development build (-DNRTGPU_DEV, libnrtgpu_dev.so).  NOT part
 * of the drop-in boundary (include/nrtgpu.h -- the header the Java binding mirrors): the product library exports none of
 * this, compiles no instrumented kernel, reads no experiment knob from the environment (runtime_internal.h: dev_env_*), and
 * rejects every non-zero value of nrtgpu_config.flags bits 8-11 (7 = instrumented kernels, same results; kernels.hip:
 * variants 1-4 and 6 drop work to time the rest and return wrong results).  The GPU tests that need a hook run against the
 * development library (tests/conftest.py: dev_lib) -- the same sources with these few functions added.
 */
#ifndef NRTGPU_DEV_H
#define NRTGPU_DEV_H
#include "nrtgpu.h"
#ifdef __cplusplus
extern "C" {
#endif
/* Closed-loop load generator (C concurrent clients): `clients` native threads each issue one query at a
 * time through nrtgpu_search_bm25_coalesced for duration_ms, cycling through `queries`.
 * out4 = {completed queries, elapsed seconds, p50 latency ms, p99 latency ms}. */
int  nrtgpu_bench_closed_loop(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                              const nrtgpu_bm25_query* queries, int32_t n_queries, int32_t clients, int32_t duration_ms,
                              double* out4);
/* TEST HOOKS for the coalescers (this one, nrtgpu_knn_exact_coalesced, nrtgpu_knn_search_coalesced and their byte twins).  hold != 0: no leader leaves with less than a
 * full batch (max_batch queries) / panel (64 queries) until the hold is released -- a test queues a known set of callers behind
 * it, waits until nrtgpu_debug_coalescer_pending (which: 0 = BM25, 1 = exact vector search, 2 = knn requests, 3 = knn requests over byte
 * fields, 4 = exact search over byte fields) reports all of them, releases,
 * and may then assert the batches formed BY CONSTRUCTION (what a batch is must not depend on the host's speed).  Not for
 * production callers: a held coalescer parks every request. */
int  nrtgpu_debug_hold_coalescers(nrtgpu_ctx* ctx, int32_t hold);
int  nrtgpu_debug_coalescer_pending(nrtgpu_ctx* ctx, int32_t which);
/* TEST HOOK for the one-call multi-GPU searches (nrtgpu_dist_search_bm25_batch[_mode], nrtgpu_dist_knn_exact,
 * nrtgpu_dist_search_hybrid_batch): the NEXT such call on this context (nrtgpu_dist_init first) fails `step` (>= 0) with
 * NRTGPU_ERR_STATE ("injected"), as a host-side error before anything of that step is enqueued: 0 the shard search (BM25, kNN,
 * the hybrid's first pass), 1 the merge after an exchange (BM25: the first one, with the verdicts), 2 the BM25 re-run, 3 the
 * hybrid's merge of the first pass, 4 the hybrid tail, 5 the merge after the BM25 re-run's exchange.  failed_query (>= 0): that
 * query's speculative guess counts as failed in this rank's verdicts (BM25 with speculation), so that the call runs it again --
 * a test plants the same query on every rank.  -1: none. */
int  nrtgpu_debug_dist_inject(nrtgpu_ctx* ctx, int32_t step, int32_t failed_query);
/* TEST HOOK: segment handles of the context (uploads and forks) that have not been freed yet.  nrtgpu_segment_release under
 * running searches defers the free to the last of them: this count is how a test observes that it happened. */
int64_t nrtgpu_debug_live_segments(nrtgpu_ctx* ctx);
/* Speculative thresholds (nrtgpu_set_speculation): out3 = {queries run under speculation, queries whose guess failed the
 * merge's check and were run again, 1 once the library has switched speculation off for this context} -- the three
 * nrtgpu_stats.spec_* values on their own. */
int  nrtgpu_debug_spec_counters(nrtgpu_ctx* ctx, int64_t* out3);
/* TEST HOOK: which doc -> posting lookup structure the seal gave a term of a sealed segment (the MaxScore walk's later clauses;
 * the policy and the budget nrtgpu_config.lookup_budget_pct: segment.cpp, build_term_aux).  *kind: 0 none (the term is searched
 * in its cell of the tile-granular table), 1 records per 32 docs, 2 lookup cells; *shift: log2 of the docs per lookup cell
 * (kind 2, else 0); *bytes: the structure's size.  Answers from the host's copy of the decision: no device work.
 * NRTGPU_ERR_INVALID_ARG when the segment holds no such term. */
int  nrtgpu_debug_term_lookup(const nrtgpu_seg* seg, int32_t field_id, int64_t term_hash, int32_t* kind, int32_t* shift, int64_t* bytes);
/* TEST HOOK: the rounding bounds the exact float vector search certifies its answers with, from the library's own code
 * (host_math.h: knn_bound32 / knn_bound16 / knn_sketch_scale; plan.h: knn_result_upper / knn_estimate_lower) -- no context, no
 * device work.  sim 0-3 as in nrtgpu_knn_exact; dim: the RESIDENT dimension (the field's, rounded up to 16); q_norm2, q_l1,
 * q_absmax: the query's |q|^2, 1-norm and largest |element|; nv_max / nv_min: the largest / smallest non-zero |v|^2 of the rows
 * (+inf: none); rows_absmax: the rows' largest |element| (the leaf with the smallest one when there are several); score_boost:
 * the boost inside the score (1 on the knn request path).  out10 = {E of an fp32 estimate, E of the fp16 sketch's estimate,
 * knn_result_upper(m) under each of the two, knn_estimate_lower(s) under each of the two, the query's sketch scale, the rows',
 * 1 when the query's scale is usable (else the panel nominates from the fp32 rows), 1 when the rows' is (else no sketch is
 * built)}. */
int  nrtgpu_debug_knn_bounds(int32_t sim, int32_t dim, double q_norm2, double q_l1, float q_absmax, double nv_max, double nv_min,
                             float rows_absmax, float score_boost, double m, double s, double* out10);
/* TEST HOOK for the unpacking of a knn request panel (nrtgpu_knn_search_requests: a pass is searched with the largest k of its
 * members, k_pass) -- no context, no device work.  scores / docs: n_queries lists of k_stride (>= k_pass) entries sorted by (score
 * desc, doc asc), counts[q] of them valid (<= k_stride).  Member q gets the first min(counts[q], ks[q], out[q].capacity) hits, its
 * scores multiplied by boosts[q] (equal products re-ordered by docid), total_hits = the hits returned.  NULL ks / boosts: k_pass / 1
 * for all. */
int  nrtgpu_debug_knn_unpack(const float* scores, const int32_t* docs, const uint32_t* counts, int32_t k_stride, int32_t n_queries,
                             int32_t k_pass, const int32_t* ks, const float* boosts, nrtgpu_topdocs* out);

#define NRTGPU_FLAG_PROFILE (7 << 8)  /* instrumented kernels (same results): per-item phase cycle and event counters
                                       * (nrtgpu_get_scan_profile, nrtgpu_get_maxscore_profile).  Bits 8-11 hold no other
                                       * value in the product library: nrtgpu_create rejects them */
/* sums over all items since the last reset, instrumented kernel only (wave 0 of each workgroup;
 * cycles = shader clock): [0] prologue cycles, [1] cycles waiting at the rendezvous barrier,
 * [2] rendezvous cycles incl. that wait, [3] walk cycles, [4] epilogue cycles, [5] rendezvous,
 * [6] compactions, [7] sub-tiles, [8] rendezvous: selection cycles, [9] sparse sub-tiles (collected
 * through the postings), [10] rendezvous: keep cycles, [11] rendezvous: publish + append cycles, [12] sub-tiles with candidates,
 * [13] sub-tiles with a possibly competitive doc, [14] last wave's finish cycle, [15] first wave's */
int  nrtgpu_get_scan_profile(nrtgpu_ctx* ctx, double* out16);
/* the same flag, items of the MaxScore route; sums over items since the last reset: [0] doc windows walked, [1] top-k
 * compactions, [2] posting chunks (512 postings), [3] postings streamed, [4] postings whose bound reached theta,
 * [5] docs evaluated, [6] lookups in later clauses, [7] candidates collected; shader-clock cycles: [8] item prologue,
 * [9] whole item, [10] waves in meetings (waiting + compaction), [11] waves out of windows waiting for the item's end,
 * [12] waves in part prologues, [13] waves walking windows, [14] the item's last wave running out of windows, [15] item
 * epilogue ([10]-[13]: summed over the item's 12 waves) */
int  nrtgpu_get_maxscore_profile(nrtgpu_ctx* ctx, double* out16);
/* the same flag, the MaxScore route's MEETINGS (all twelve waves of a workgroup stop: maxscore.hip, ms_compact); sums over items
 * since the last reset: out4 = {meetings, meetings called because the candidate buffer overflowed, meetings that compacted the
 * buffer (= nrtgpu_get_maxscore_profile [1]), speculative estimates made by ONE wave while the others walked on (ms_estimate)}.
 * A meeting that is no overflow meeting was called for a speculative estimate alone: none in the product's walk, where the
 * estimate has left the meeting; NRTGPU_MS_SPEC_MEET=1 (environment, this library only, read per call) brings them back for an
 * A/B in one process. */
int  nrtgpu_debug_maxscore_meetings(nrtgpu_ctx* ctx, int64_t* out4);
/* ... and, over the same items, the speculative guesses that raised a workgroup's theta IN a meeting (the histogram's bucket edge
 * of an overflow compaction, or the estimate of a meeting called for one): what decides how many of an overflow compaction's k best
 * keys are still live.  NRTGPU_MS_KEEP_LIVE=0 (environment, this library only, read per call) makes a compaction keep the k best,
 * dead keys included, as it used to -- for an A/B in one process. */
int  nrtgpu_debug_maxscore_meeting_guesses(nrtgpu_ctx* ctx, int64_t* out1);
/* TEST HOOK: the one-wave selection the estimator uses (topk.hiph: topk_kth_wave), run by a one-wave kernel over keys[0..n)
 * held in LDS as the walk holds them: *out = the r-th largest (1-based) of the keys, a zero key being an unwritten slot (it ranks
 * below every key).  1 <= r <= n <= the walk's candidate buffer (2304 slots). */
int  nrtgpu_debug_wave_kth(const uint64_t* keys, int32_t n, int32_t r, uint64_t* out);
/* TEST HOOK: the MaxScore route's WALK ROWS (plan.h: DWalkRow) of a batch, as the plan expansion writes them on the device: the
 * batch is planned as a search would plan it and expanded; nothing is searched.  out_begin[q * n_segs + leaf]: the first row of
 * (query, leaf), -1 when the leaf holds none of the query's terms (or lacks a MUST term) or the query is not on the MaxScore route;
 * out_n[q * n_segs + leaf]: how many (the clauses the leaf holds, heaviest first).  Row r is ten 64-bit words at out_rows[10 r]:
 * {docid column, score-code column, S_c, ub_c, weight bits | fx_scale << 32, flags, u_after_c, lookup structure, cell table, first
 * posting} -- ub_c the clause's exact maximum score in the leaf, u_after_c what the later clauses add at most, S_c the two
 * combined, all in the query's common fixed-point scale.  Returns the number of rows (<= cap_rows are written), < 0: -error. */
int64_t nrtgpu_debug_walk_rows(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                               const nrtgpu_bm25_query* queries, int32_t n_queries, int32_t* out_begin, int32_t* out_n,
                               uint64_t* out_rows, int64_t cap_rows);
/* TEST HOOK: what ONE posting adds to a doc's fixed-point sum, computed on the device by the statement the scorers and the walk
 * rows use: out[i] = (integer BM25 score of (weight, freq[i], table256[norm[i]]) at scale 2^fx_scale) << fx_shift. */
int  nrtgpu_debug_walk_value(float weight, const uint32_t* freq, const uint32_t* norm, int32_t n, const float* table256, int32_t fx_scale,
                             uint32_t fx_shift, uint64_t* out);
/* the same flag: WHEN the pieces of the last MaxScore launch ran.  Per output slot eight words -- {start, end} on the device's
 * 100 MHz wall clock, the item worked on, the doc windows walked, when the workgroup's round began (persistent workgroups choose
 * work round after round), the CU (XCC << 8 | SE, SH, CU), the round, the workgroup; a slot nobody used is all zeros.  The first
 * *n_items slots are the items' owners; slots beyond the call's items (MaxScore + scan) are HELPERS: workgroups that shared the
 * windows of an item someone else owns.  Returns the number of slots (<= cap_slots are written); the makespan of the
 * launch against its balanced load is max(end) - min(start) vs sum(end - start) / CUs. */
int64_t nrtgpu_get_maxscore_item_walls(nrtgpu_ctx* ctx, uint64_t* out, int64_t cap_slots, int64_t* n_items);

#ifdef __cplusplus
}
#endif
#endif /* NRTGPU_DEV_H */
