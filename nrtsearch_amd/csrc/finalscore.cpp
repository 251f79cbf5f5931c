// finalscore.cpp -- the host path the two final-score routes share (funcscore.cpp: function-score queries, multimatch.cpp:
// multi-match queries): their entry checks and refusals, the exhaustive plan, and everything from "the plan and the route's
// records exist" to "out[], the diagnostics and the statistics are filled".  On the device: the existing plan expansion, then the
// route's scorer (finalscore.hiph) over all items, then the existing merge and per-slice relation.
#include "runtime_internal.h"

namespace nrtgpu {
namespace rt {

int final_score_enter(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs, bool null_argument, const int32_t* n_queries) {
  if (!ctx || null_argument || (n_segs > 0 && !segs)) return fail(NRTGPU_ERR_INVALID_ARG, "NULL argument");
  if (n_queries) {
    if (*n_queries <= 0 || n_segs < 0) return fail(NRTGPU_ERR_INVALID_ARG, "n_queries must be > 0");
    if (*n_queries > ctx->cfg.max_batch) return fail(NRTGPU_ERR_INVALID_ARG, "batch of %d exceeds max_batch %d", *n_queries, ctx->cfg.max_batch);
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
                               FinalScoreLaunch launch, uint64_t** out_keys, uint32_t** out_counts, uint64_t** out_hits) {
  forget_foreign_hip_error();
  const size_t n_items = hp.items.size();
  Carver pc;
  const size_t o_queries = pc.take(hp.queries.size() * sizeof(DQuery));
  const size_t o_items = pc.take(n_items * sizeof(DItem));
  const size_t o_parts = pc.take(hp.parts.size() * sizeof(DPart));
  const size_t o_qterms = pc.take(hp.qterms.size() * sizeof(DQTerm));
  const size_t o_qexp = pc.take(sizeof(DExpandHead) + hp.qexpand.size() * sizeof(DQExpand)) + sizeof(DExpandHead);
  const size_t o_qsb = pc.take(hp.qs_begin.size() * 4);
  const size_t o_caches = pc.take(hp.caches.size() * sizeof(float));
  const size_t o_lidx = pc.take(hp.list_idx.size() * 4);
  const size_t o_qbase = pc.take(hp.q_base.size() * 4);
  const size_t o_qnl = pc.take(hp.q_nlists.size() * 4);
  const size_t o_qk = pc.take(hp.q_k.size() * 4);
  const size_t o_theta = pc.take(hp.theta_init.size() * 8);   // zeros (no min_competitive_score on these routes), then the kernel's
  size_t o_extra[kFinalScoreExtras] = {};                      // the route's own arrays, in its order
  if (n_extras < 0 || n_extras > kFinalScoreExtras) return fail(NRTGPU_ERR_STATE, "final score: %d extra plan arrays", n_extras);
  for (int i = 0; i < n_extras; ++i) o_extra[i] = pc.take(extras[i].bytes);
  const size_t plan_bytes = pc.off;
  if (int rc = slot->h_plan.reserve(plan_bytes)) return rc;
  if (int rc = slot->d_plan.reserve(plan_bytes)) return rc;
  Carver wc;
  const size_t o_ikeys = wc.take(n_items * (size_t)hp.k_stride * 8);
  const size_t o_icnt = wc.take(n_items * 4);
  const size_t o_ihits = wc.take(n_items * 8);
  const size_t o_okeys = wc.take((size_t)n_queries * hp.k_stride * 8);
  const size_t o_ocnt = wc.take((size_t)n_queries * 4);
  const size_t o_ohits = wc.take((size_t)n_queries * 8);
  const size_t o_terms = wc.take((size_t)hp.n_dterms * sizeof(DTerm));   // written by expand_terms_kernel
  const size_t o_ssum = wc.take((size_t)n_queries * hp.n_slices * 4);    // hits per (query, searcher slice): zeroed per call
  if (int rc = slot->d_work.reserve(wc.off)) return rc;
  char* hb = (char*)slot->h_plan.p;
  char* db = (char*)slot->d_plan.p;
  char* wb = (char*)slot->d_work.p;
  auto put = [&](size_t off, const void* src, size_t bytes) {
    if (bytes) memcpy(hb + off, src, bytes);
  };
  put(o_queries, hp.queries.data(), hp.queries.size() * sizeof(DQuery));
  put(o_items, hp.items.data(), n_items * sizeof(DItem));
  put(o_parts, hp.parts.data(), hp.parts.size() * sizeof(DPart));
  put(o_qterms, hp.qterms.data(), hp.qterms.size() * sizeof(DQTerm));
  put(o_qexp, hp.qexpand.data(), hp.qexpand.size() * sizeof(DQExpand));
  put(o_qsb, hp.qs_begin.data(), hp.qs_begin.size() * 4);
  put(o_caches, hp.caches.data(), hp.caches.size() * sizeof(float));
  put(o_lidx, hp.list_idx.data(), hp.list_idx.size() * 4);
  put(o_qbase, hp.q_base.data(), hp.q_base.size() * 4);
  put(o_qnl, hp.q_nlists.data(), hp.q_nlists.size() * 4);
  put(o_qk, hp.q_k.data(), hp.q_k.size() * 4);
  put(o_theta, hp.theta_init.data(), hp.theta_init.size() * 8);
  const void* d_extra[kFinalScoreExtras] = {};
  for (int i = 0; i < n_extras; ++i) {
    put(o_extra[i], extras[i].p, extras[i].bytes);
    d_extra[i] = db + o_extra[i];
  }
  {   // what the plan expansion reads in front of the DQExpand array (plan.h: DExpandHead); no walk rows on these routes
    DExpandHead xh{};
    xh.caches = (const float*)(db + o_caches);
    xh.queries = (const DQuery*)(db + o_queries);
    xh.rows = nullptr;
    memcpy(hb + o_qexp - sizeof(DExpandHead), &xh, sizeof(xh));
  }
  hipStream_t st = slot->stream;
  HIP_TRY(hipMemcpyAsync(db, hb, plan_bytes, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(wb + o_ssum, 0, wc.off - o_ssum, st));
  const bool timing = ctx->cfg.collect_timing != 0;
  launch_expand_terms(st, (const DQExpand*)(db + o_qexp), (const DQTerm*)(db + o_qterms), (const uint32_t*)(db + o_qsb), (uint32_t)n_queries,
                      hp.n_leaves, (DTerm*)(wb + o_terms));
  FinalScoreArgs a{};
  a.n_items = (uint32_t)n_items;
  a.items = (const DItem*)(db + o_items);
  a.parts = (const DPart*)(db + o_parts);
  a.terms = (const DTerm*)(wb + o_terms);
  a.queries = (const DQuery*)(db + o_queries);
  a.caches = (const float*)(db + o_caches);
  a.theta_g = (unsigned long long*)(db + o_theta);
  a.slice_sum = (uint32_t*)(wb + o_ssum);
  a.item_keys = (uint64_t*)(wb + o_ikeys);
  a.item_counts = (uint32_t*)(wb + o_icnt);
  a.item_hits = (uint64_t*)(wb + o_ihits);
  a.k_stride = hp.k_stride;
  {
    std::unique_lock<std::mutex> gpu(ctx->gpu_mu);
    if (ctx->last_turn) HIP_TRY(hipStreamWaitEvent(st, ctx->last_turn, 0));
    if (ctx->last_knn_turn) HIP_TRY(hipStreamWaitEvent(st, ctx->last_knn_turn, 0));
    if (timing) HIP_TRY(hipEventRecord(slot->ev0, st));
    launch(st, a, d_extra);
    if (timing) HIP_TRY(hipEventRecord(slot->ev1, st));
    HIP_TRY(hipEventRecord(slot->ev_turn, st));   // the turn ends behind the scorer, as in enqueue_search
    ctx->last_turn = slot->ev_turn;
    launch_merge_topk(st, (uint32_t)n_queries, a.item_keys, a.item_counts, a.item_hits, (const uint32_t*)(db + o_lidx),
                      (const uint32_t*)(db + o_qbase), (const uint32_t*)(db + o_qnl), hp.k_stride, (const uint32_t*)(db + o_qk),
                      (uint64_t*)(wb + o_okeys), (uint32_t*)(wb + o_ocnt), (uint64_t*)(wb + o_ohits), hp.k_stride);
    launch_slice_relation(st, a.slice_sum, a.queries, hp.n_slices, (uint64_t*)(wb + o_ohits), (uint32_t)n_queries);
    if (timing) HIP_TRY(hipEventRecord(slot->ev2, st));
  }
  HIP_TRY(hipGetLastError());
  *out_keys = (uint64_t*)(wb + o_okeys);
  *out_counts = (uint32_t*)(wb + o_ocnt);
  *out_hits = (uint64_t*)(wb + o_ohits);
  return NRTGPU_OK;
}

int final_score_run(nrtgpu_ctx* ctx, const HostPlan& hp, const nrtgpu_bm25_query* queries, int32_t n_queries, nrtgpu_topdocs* out, double t0,
                    const PlanBytes* extras, int n_extras, FinalScoreLaunch launch) {
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
  if (int rc = enqueue_final_score(ctx, slot, hp, n_queries, extras, n_extras, launch, &d_keys, &d_counts, &d_hits)) return rc;
  HIP_TRY(hipMemcpyAsync(ho + o_k, d_keys, kb, hipMemcpyDeviceToHost, slot->stream));
  HIP_TRY(hipMemcpyAsync(ho + o_c, d_counts, cb, hipMemcpyDeviceToHost, slot->stream));
  HIP_TRY(hipMemcpyAsync(ho + o_h, d_hits, hb, hipMemcpyDeviceToHost, slot->stream));
  HIP_TRY(wait_for_stream((ctx->cfg.flags & NRTGPU_FLAG_BLOCKING_WAIT) != 0, slot->stream, slot->ev_wait));
  const uint64_t* keys = (const uint64_t*)(ho + o_k);
  const uint32_t* cnts = (const uint32_t*)(ho + o_c);
  const uint64_t* hits = (const uint64_t*)(ho + o_h);
  for (int qi = 0; qi < n_queries; ++qi) {
    // (search.cpp: unpack_topdocs, without the MaxScore route's lower bounds: the count is exact; the high bits of `hits` carry
    // slice_relation_kernel's tag, and a page shorter than numHits is EQUAL_TO)
    nrtgpu_topdocs& o = out[qi];
    const uint64_t* kq = keys + (size_t)qi * hp.k_stride;
    const int32_t cap = o.capacity > 0 ? o.capacity : queries[qi].k;
    const int32_t m = std::min<int32_t>((int32_t)cnts[qi], cap);
    if (o.docs)
      for (int32_t i = 0; i < m; ++i) o.docs[i] = (int32_t)key_doc(kq[i]);
    if (o.scores)
      for (int32_t i = 0; i < m; ++i) o.scores[i] = key_score(kq[i]);
    o.n_hits = m;
    o.total_hits = (int64_t)(hits[qi] & (kHitsPrunedUnit - 1));
    o.total_hits_is_lower_bound = ((hits[qi] >> 48) != 0 && cnts[qi] == (uint32_t)queries[qi].k) ? 1 : 0;
  }
  float kernel_ms = 0.f, merge_ms = 0.f;
  if (ctx->cfg.collect_timing) {
    (void)hipEventElapsedTime(&kernel_ms, slot->ev0, slot->ev1);
    (void)hipEventElapsedTime(&merge_ms, slot->ev1, slot->ev2);
  }
  {
    nrtgpu_diagnostics d{};
    d.total_ms = now_ms() - t0;
    d.plan_ms = plan_ms;
    d.queue_ms = queue_ms;
    d.device_ms = (double)kernel_ms + (double)merge_ms;
    d.postings = hp.postings;
    d.queries = n_queries;
    d.items_maxscore = 0;
    d.items_scan = (int32_t)hp.items.size();
    g_diag = d;
  }
  std::lock_guard<std::mutex> lk(ctx->stats_mu);
  ctx->stats.batches += 1;
  ctx->stats.queries += n_queries;
  ctx->stats.scan_launches += hp.items.empty() ? 0 : 1;
  ctx->stats.fixed_point_launches += hp.items.empty() ? 0 : 1;
  ctx->stats.scan_ms += hp.items.empty() ? 0.f : kernel_ms;
  ctx->stats.merge_ms += merge_ms;
  ctx->stats.scan_postings += hp.postings;
  ctx->stats.scan_items += (int64_t)hp.items.size();
  ctx->stats.host_plan_ms += plan_ms;
  return NRTGPU_OK;
}

}  // namespace rt
}  // namespace nrtgpu
