// finalscore.cpp -- the host path the final-score routes share (funcscore.cpp: function-score queries, multimatch.cpp:
// multi-match queries, funcscore_multimatch.cpp: the one around the other): their entry checks and refusals, the exhaustive plan, and everything from "the plan and the route's
// records exist" to "out[], the diagnostics and the statistics are filled".  On the device: the existing plan expansion, then the
// route's scorer (finalscore.hiph) over all items, then the existing merge and per-slice relation.  A route whose answer is not
// a list of hits (termscount.cpp) asks for workspace bytes of its own, zeroed with the per-slice sums, and collects them itself
// behind the wait (FinalScoreOwn); the routes that ask for none enqueue and copy what they always did.
#include "runtime_internal.h"

namespace nrtgpu {
namespace rt {

int final_score_enter(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs, bool null_argument, const int32_t* n_queries) {
  if (!ctx || null_argument || (n_segs > 0 && !segs)) return fail(NRTGPU_ERR_INVALID_ARG, "NULL argument");
  if (n_queries) {
    if (int rc = check_batch_size(ctx, *n_queries, n_segs)) return rc;
  } else if (n_segs < 0) {
    return fail(NRTGPU_ERR_INVALID_ARG, "n_segs must be >= 0");
  }
  for (int si = 0; si < n_segs; ++si)
    if (!segs[si]) return fail(NRTGPU_ERR_INVALID_ARG, "segment %d is NULL", si);
  if (n_queries) NRT_CHECK_DEADLINE("before the search was planned");
  HIP_TRY(hipSetDevice(ctx->device));
  return NRTGPU_OK;
}

int final_score_check_flags(const nrtgpu_ctx* ctx, const char* route) {
  if (ctx->cfg.flags & NRTGPU_FLAG_PACKED_POSTINGS)
    return fail(NRTGPU_ERR_UNSUPPORTED, "%s queries do not run over packed postings (NRTGPU_FLAG_PACKED_POSTINGS)", route);
  if (ctx->cfg.flags & NRTGPU_FLAG_NO_FIXED_POINT)
    return fail(NRTGPU_ERR_UNSUPPORTED, "%s queries need the fixed-point accumulators (NRTGPU_FLAG_NO_FIXED_POINT is set)", route);
  return NRTGPU_OK;
}

int final_score_plan(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs, const nrtgpu_bm25_query* queries,
                     int32_t n_queries, const char* route, HostPlan& hp) {
  if (int rc = build_plan(ctx, segs, doc_bases, n_segs, queries, n_queries, hp, 0)) return rc;
  if (!hp.fixed_point)
    return fail(NRTGPU_ERR_UNSUPPORTED, "%s queries need the fixed-point accumulators (the weights of a query in this batch span too many binades)", route);
  return NRTGPU_OK;
}

// Plan upload, expansion, the route's scorer over all items, merge, per-slice relation: enqueued at once on the slot's stream.
// The scorer wants the whole GPU like the two scorers of search.cpp and takes its turn among them on the device.
static int enqueue_final_score(nrtgpu_ctx* ctx, Slot* slot, const HostPlan& hp, int32_t n_queries, const PlanBytes* extras, int n_extras,
                               FinalScoreLaunch launch, const FinalScoreOwn* own, bool counts_past, uint64_t** out_keys, uint32_t** out_counts,
                               uint64_t** out_hits, const char** d_own) {
  forget_foreign_hip_error();
  const size_t n_items = hp.items.size();
  PlanLayout L(hp, n_items, (size_t)n_queries, hp.k_stride);   // theta: zeros (no min_competitive_score on these routes), then the kernel's
  size_t o_extra[kFinalScoreExtras] = {};                      // the route's own arrays, in its order
  if (n_extras < 0 || n_extras > kFinalScoreExtras) return fail(NRTGPU_ERR_STATE, "final score: %d extra plan arrays", n_extras);
  for (int i = 0; i < n_extras; ++i) o_extra[i] = L.plan.take(extras[i].bytes);
  const size_t plan_bytes = L.plan.off;
  if (int rc = slot->h_plan.reserve(plan_bytes)) return rc;
  if (int rc = slot->d_plan.reserve(plan_bytes)) return rc;
  const size_t o_ssum = L.work.take((size_t)n_queries * hp.n_slices * 4);    // hits per (query, searcher slice): zeroed per call
  const size_t o_past = counts_past ? L.work.take((size_t)n_queries * hp.n_slices * 4) : 0;   // ... those behind the query's cursor: zeroed with them
  const size_t o_own = own ? L.work.take(own->work_bytes) : 0;                // the route's own output: zeroed with the sums
  if (int rc = slot->d_work.reserve(L.work.off)) return rc;
  char* hb = (char*)slot->h_plan.p;
  char* db = (char*)slot->d_plan.p;
  char* wb = (char*)slot->d_work.p;
  L.fill(hb, hp);
  const void* d_extra[kFinalScoreExtras] = {};
  for (int i = 0; i < n_extras; ++i) {
    PlanLayout::put(hb, o_extra[i], extras[i].p, extras[i].bytes);
    d_extra[i] = db + o_extra[i];
  }
  L.put_expand_head(hb, db, nullptr);   // (no walk rows on these routes)
  hipStream_t st = slot->stream;
  HIP_TRY(hipMemcpyAsync(db, hb, plan_bytes, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(wb + o_ssum, 0, L.work.off - o_ssum, st));
  const bool timing = ctx->cfg.collect_timing != 0;
  launch_expand_terms(st, (const DQExpand*)(db + L.qexpand), (const DQTerm*)(db + L.qterms), (const uint32_t*)(db + L.qs_begin), (uint32_t)n_queries,
                      hp.n_leaves, (DTerm*)(wb + L.terms));
  FinalScoreArgs a{};
  a.n_items = (uint32_t)n_items;
  a.items = (const DItem*)(db + L.items);
  a.parts = (const DPart*)(db + L.parts);
  a.terms = (const DTerm*)(wb + L.terms);
  a.queries = (const DQuery*)(db + L.queries);
  a.caches = (const float*)(db + L.caches);
  a.theta_g = (unsigned long long*)(db + L.theta);
  a.slice_sum = (uint32_t*)(wb + o_ssum);
  a.slice_past = counts_past ? (uint32_t*)(wb + o_past) : nullptr;
  a.item_keys = (uint64_t*)(wb + L.item_keys);
  a.item_counts = (uint32_t*)(wb + L.item_counts);
  a.item_hits = (uint64_t*)(wb + L.item_hits);
  a.k_stride = hp.k_stride;
  a.own = own ? wb + o_own : nullptr;
  a.own_user = own ? own->user : nullptr;
  {
    std::unique_lock<std::mutex> gpu(ctx->gpu_mu);
    if (ctx->last_turn) HIP_TRY(hipStreamWaitEvent(st, ctx->last_turn, 0));
    if (ctx->last_knn_turn) HIP_TRY(hipStreamWaitEvent(st, ctx->last_knn_turn, 0));
    if (timing) HIP_TRY(hipEventRecord(slot->ev0, st));
    launch(st, a, d_extra);
    if (timing) HIP_TRY(hipEventRecord(slot->ev1, st));
    HIP_TRY(hipEventRecord(slot->ev_turn, st));   // the turn ends behind the scorer, as in enqueue_search
    ctx->last_turn = slot->ev_turn;
    launch_merge_topk(st, (uint32_t)n_queries, a.item_keys, a.item_counts, a.item_hits, (const uint32_t*)(db + L.list_idx),
                      (const uint32_t*)(db + L.q_base), (const uint32_t*)(db + L.q_nlists), hp.k_stride, (const uint32_t*)(db + L.q_k),
                      (uint64_t*)(wb + L.out_keys), (uint32_t*)(wb + L.out_counts), (uint64_t*)(wb + L.out_hits), hp.k_stride);
    if (counts_past) launch_slice_relation_past(st, a.slice_sum, a.slice_past, a.queries, hp.n_slices, (uint64_t*)(wb + L.out_hits), (uint32_t)n_queries);
    else launch_slice_relation(st, a.slice_sum, a.queries, hp.n_slices, (uint64_t*)(wb + L.out_hits), (uint32_t)n_queries);
    if (timing) HIP_TRY(hipEventRecord(slot->ev2, st));
  }
  HIP_TRY(hipGetLastError());
  *out_keys = (uint64_t*)(wb + L.out_keys);
  *out_counts = (uint32_t*)(wb + L.out_counts);
  *out_hits = (uint64_t*)(wb + L.out_hits);
  *d_own = own ? wb + o_own : nullptr;
  return NRTGPU_OK;
}

int final_score_run(nrtgpu_ctx* ctx, const HostPlan& hp, const nrtgpu_bm25_query* queries, int32_t n_queries, nrtgpu_topdocs* out, double t0,
                    const PlanBytes* extras, int n_extras, FinalScoreLaunch launch, const FinalScoreOwn* own, bool counts_past) {
  const double plan_ms = now_ms() - t0;

  Slot* slot = nullptr;
  acquire_slot(ctx, &slot);
  SlotGuard guard{ctx, slot};
  const double queue_ms = now_ms() - t0 - plan_ms;
  NRT_CHECK_DEADLINE("while the search waited for a workspace");   // (nothing has been launched)
  const size_t kb = (size_t)n_queries * hp.k_stride * 8, cb = (size_t)n_queries * 4, hb = (size_t)n_queries * 8;
  Carver oc;
  const size_t o_k = oc.take(kb), o_c = oc.take(cb), o_h = oc.take(hb);
  if (int rc = slot->h_out.reserve(oc.off)) return rc;
  char* ho = (char*)slot->h_out.p;
  uint64_t* d_keys = nullptr;
  uint32_t* d_counts = nullptr;
  uint64_t* d_hits = nullptr;
  const char* d_own = nullptr;
  if (int rc = enqueue_final_score(ctx, slot, hp, n_queries, extras, n_extras, launch, own, counts_past, &d_keys, &d_counts, &d_hits, &d_own)) return rc;
  HIP_TRY(hipMemcpyAsync(ho + o_k, d_keys, kb, hipMemcpyDeviceToHost, slot->stream));
  HIP_TRY(hipMemcpyAsync(ho + o_c, d_counts, cb, hipMemcpyDeviceToHost, slot->stream));
  HIP_TRY(hipMemcpyAsync(ho + o_h, d_hits, hb, hipMemcpyDeviceToHost, slot->stream));
  HIP_TRY(wait_for_stream((ctx->cfg.flags & NRTGPU_FLAG_BLOCKING_WAIT) != 0, slot->stream, slot->ev_wait));
  const uint64_t* keys = (const uint64_t*)(ho + o_k);
  const uint32_t* cnts = (const uint32_t*)(ho + o_c);
  const uint64_t* hits = (const uint64_t*)(ho + o_h);
  // (without the MaxScore route's lower bounds: the count is exact; the high bits of `hits` carry slice_relation_kernel's tag, and a
  // page shorter than numHits is EQUAL_TO)
  for (int qi = 0; qi < n_queries; ++qi) unpack_topdocs(keys + (size_t)qi * hp.k_stride, cnts[qi], hits[qi], queries[qi].k, 0, cnts[qi], &out[qi]);
  if (own && own->collect)
    if (int rc = own->collect(ctx, slot, d_own, own->user)) return rc;
  account(ctx, slot, hp, n_queries, plan_ms, t0, queue_ms);
  return NRTGPU_OK;
}

}  // namespace rt
}  // namespace nrtgpu
