// funcscore.cpp -- function-score queries (include/nrtgpu.h: nrtgpu_search_function_score_batch): MultiFunctionScoreQuery with
// weight functions over a BM25 disjunction.  The inner queries are planned as the exhaustive route plans them (build_plan,
// prune = 0: the reference scores the wrapper under ScoreMode.COMPLETE, nothing may be skipped); beside the plan go one
// DFuncQuery per query and one DFuncMasks per part (plan.h).  On the device: the existing plan expansion, then
// bm25_function_score_kernel (funcscore.hip) over all items, then the existing merge and per-slice relation.
#include "runtime_internal.h"

// the record the kernel and nrtgpu_function_score_value read, from the caller's struct; refusals by the header's table
static int function_record(const nrtgpu_function_score& fs, int qi, DFuncQuery* out) {
  if (fs.n_functions < 0 || fs.n_functions > NRTGPU_MAX_FUNCTIONS)
    return fail(NRTGPU_ERR_INVALID_ARG, "query %d: n_functions %d outside 0..%d", qi, fs.n_functions, NRTGPU_MAX_FUNCTIONS);
  if (fs.n_functions > 0 && !fs.functions) return fail(NRTGPU_ERR_INVALID_ARG, "query %d: functions is NULL", qi);
  if (fs.score_mode < 0 || fs.score_mode > 1) return fail(NRTGPU_ERR_INVALID_ARG, "query %d: score_mode %d outside 0..1", qi, fs.score_mode);
  if (fs.boost_mode < 0 || fs.boost_mode > 2) return fail(NRTGPU_ERR_INVALID_ARG, "query %d: boost_mode %d outside 0..2", qi, fs.boost_mode);
  if (!std::isfinite(fs.min_score) || fs.min_score < 0.0f) return fail(NRTGPU_ERR_INVALID_ARG, "query %d: min_score must be finite and >= 0", qi);
  if (fs.min_excluded != 0 && fs.min_excluded != 1) return fail(NRTGPU_ERR_INVALID_ARG, "query %d: min_excluded must be 0 or 1", qi);
  DFuncQuery r{};
  r.n_functions = fs.n_functions;
  r.score_mode = fs.score_mode;
  r.boost_mode = fs.boost_mode;
  r.min_excluded = fs.min_excluded;
  r.min_score = fs.min_score;
  for (int i = 0; i < fs.n_functions; ++i) {
    const float w = fs.functions[i].weight;
    if (!std::isfinite(w) || w == 0.0f)
      return fail(NRTGPU_ERR_INVALID_ARG, "query %d function %d: the weight must be finite and not 0 (a request's 0 means 1: the caller maps it)", qi, i);
    if (fs.functions[i].filter_mask < 0) return fail(NRTGPU_ERR_INVALID_ARG, "query %d function %d: mask ids must be >= 0", qi, i);
    r.weight[i] = w;
  }
  for (int i = 0; i < fs.n_functions; ++i)   // (MultiFunctionScoreQuery.java:454-460 may or may not throw on the negative score: the caller keeps Lucene)
    if (fs.functions[i].weight < 0.0f) return fail(NRTGPU_ERR_UNSUPPORTED, "query %d function %d: a negative weight", qi, i);
  if (out) *out = r;
  return NRTGPU_OK;
}

extern "C" int nrtgpu_function_score_value(const nrtgpu_function_score* fs, uint32_t matched, float inner, float* out_score, int32_t* out_is_hit) {
  if (!fs || !out_score || !out_is_hit) return fail(NRTGPU_ERR_INVALID_ARG, "NULL argument");
  DFuncQuery r;
  if (int rc = function_record(*fs, 0, &r)) return rc;
  bool hit = false;
  *out_score = function_score_value(r, matched, inner, &hit);
  *out_is_hit = hit ? 1 : 0;
  return NRTGPU_OK;
}

// What the route refuses of a call before anything is planned (the segments' content is held).
static int check_call(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_bm25_query* queries,
                      const nrtgpu_function_score* functions, int32_t n_queries, std::vector<DFuncQuery>* records) {
  for (int qi = 0; qi < n_queries; ++qi) {
    if (int rc = validate_query(queries[qi], qi)) return rc;
    DFuncQuery r;
    if (int rc = function_record(functions[qi], qi, &r)) return rc;
    if (records) records->push_back(r);
  }
  if (ctx->cfg.flags & NRTGPU_FLAG_PACKED_POSTINGS)
    return fail(NRTGPU_ERR_UNSUPPORTED, "function-score queries do not run over packed postings (NRTGPU_FLAG_PACKED_POSTINGS)");
  if (ctx->cfg.flags & NRTGPU_FLAG_NO_FIXED_POINT)
    return fail(NRTGPU_ERR_UNSUPPORTED, "function-score queries need the fixed-point accumulators (NRTGPU_FLAG_NO_FIXED_POINT is set)");
  for (int qi = 0; qi < n_queries; ++qi) {
    const nrtgpu_bm25_query& q = queries[qi];
    if (q.disjunction_max != 0) return fail(NRTGPU_ERR_UNSUPPORTED, "query %d: a function score over a DisjunctionMaxQuery", qi);
    for (int t = 0; t < q.n_terms; ++t)
      if (q.terms[t].occur != 0) return fail(NRTGPU_ERR_UNSUPPORTED, "query %d: a function score over MUST clauses", qi);
    if (q.min_should_match > 1) return fail(NRTGPU_ERR_UNSUPPORTED, "query %d: a function score over minimumNumberShouldMatch %d", qi, q.min_should_match);
    if (q.min_competitive_score != 0.0f) return fail(NRTGPU_ERR_UNSUPPORTED, "query %d: a function score with a min_competitive_score", qi);
    for (int i = 0; i < functions[qi].n_functions; ++i) {
      const int32_t id = functions[qi].functions[i].filter_mask;
      if (id == 0) continue;
      for (int si = 0; si < n_segs; ++si)
        if (segs[si]->masks.find(id) == segs[si]->masks.end())
          return fail(NRTGPU_ERR_UNSUPPORTED, "query %d function %d: mask %d is not resident on segment %d", qi, i, id, si);
    }
  }
  return NRTGPU_OK;
}

static int plan_call(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs, const nrtgpu_bm25_query* queries,
                     int32_t n_queries, HostPlan& hp) {
  if (int rc = build_plan(ctx, segs, doc_bases, n_segs, queries, n_queries, hp, 0)) return rc;
  if (!hp.fixed_point)
    return fail(NRTGPU_ERR_UNSUPPORTED, "function-score queries need the fixed-point accumulators (the weights of a query in this batch span too many binades)");
  return NRTGPU_OK;
}

extern "C" int nrtgpu_function_score_supported(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_bm25_query* q,
                                               const nrtgpu_function_score* fs) {
  if (!ctx || !q || !fs || (n_segs > 0 && !segs)) return fail(NRTGPU_ERR_INVALID_ARG, "NULL argument");
  if (n_segs < 0) return fail(NRTGPU_ERR_INVALID_ARG, "n_segs must be >= 0");
  for (int si = 0; si < n_segs; ++si)
    if (!segs[si]) return fail(NRTGPU_ERR_INVALID_ARG, "segment %d is NULL", si);
  HIP_TRY(hipSetDevice(ctx->device));
  SegReadLocks content(segs, n_segs);
  if (int rc = check_call(ctx, segs, n_segs, q, fs, 1, nullptr)) return rc;
  HostPlan hp;   // the planner is the predicate for the inner query, as in nrtgpu_query_supported
  return plan_call(ctx, segs, nullptr, n_segs, q, 1, hp);
}

// The doc sets of every function on every part's leaf.  A part names its (query, leaf) pair by its first DTerm (HostPlan.qs_begin).
static int function_masks(const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_function_score* functions, const HostPlan& hp,
                          std::vector<DFuncMasks>* out) {
  out->assign(hp.parts.size(), DFuncMasks{});
  std::map<std::pair<int32_t, int32_t>, const uint64_t*> sets;   // (leaf, mask id) -> liveDocs & mask, resident
  for (const DItem& it : hp.items) {
    const nrtgpu_function_score& fs = functions[it.query];
    if (fs.n_functions == 0) continue;
    for (uint32_t pi = 0; pi < it.n_parts; ++pi) {
      const DPart& p = hp.parts[it.part_begin + pi];
      int32_t leaf = -1;
      for (int32_t si = 0; si < n_segs && leaf < 0; ++si)
        if (hp.qs_begin[(size_t)it.query * (size_t)n_segs + (size_t)si] == p.term_begin) leaf = si;
      if (leaf < 0 || (uint32_t)segs[leaf]->max_doc != p.max_doc) return fail(NRTGPU_ERR_STATE, "function score: a part of query %u names no leaf", it.query);
      DFuncMasks& fm = (*out)[it.part_begin + pi];
      for (int i = 0; i < fs.n_functions; ++i) {
        const int32_t id = fs.functions[i].filter_mask;
        if (id == 0) continue;   // no filter query: every doc (nullptr)
        auto found = sets.find({leaf, id});
        if (found == sets.end()) {
          // the doc is live when it is scored, so "liveDocs & mask" answers membership
          const uint64_t* bits = nullptr;
          if (int rc = accept_set_of(segs[leaf], id, 0, &bits)) return rc;
          found = sets.emplace(std::make_pair(leaf, id), bits).first;
        }
        fm.mask[i] = found->second;
      }
    }
  }
  return NRTGPU_OK;
}

// Plan upload, expansion, the function-score kernel over all items, merge, per-slice relation: enqueued at once on the slot's
// stream.  The kernel wants the whole GPU like the two scorers of search.cpp and takes its turn among them on the device.
static int enqueue_function_score(nrtgpu_ctx* ctx, Slot* slot, const HostPlan& hp, const std::vector<DFuncQuery>& records,
                                  const std::vector<DFuncMasks>& fmasks, int32_t n_queries, uint64_t** out_keys, uint32_t** out_counts,
                                  uint64_t** out_hits) {
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
  const size_t o_theta = pc.take(hp.theta_init.size() * 8);   // zeros (no min_competitive_score on this route), then the kernel's
  const size_t o_fq = pc.take(records.size() * sizeof(DFuncQuery));
  const size_t o_fm = pc.take(fmasks.size() * sizeof(DFuncMasks));
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
  put(o_fq, records.data(), records.size() * sizeof(DFuncQuery));
  put(o_fm, fmasks.data(), fmasks.size() * sizeof(DFuncMasks));
  {   // what the plan expansion reads in front of the DQExpand array (plan.h: DExpandHead); no walk rows on this route
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
  {
    std::unique_lock<std::mutex> gpu(ctx->gpu_mu);
    if (ctx->last_turn) HIP_TRY(hipStreamWaitEvent(st, ctx->last_turn, 0));
    if (ctx->last_knn_turn) HIP_TRY(hipStreamWaitEvent(st, ctx->last_knn_turn, 0));
    if (timing) HIP_TRY(hipEventRecord(slot->ev0, st));
    launch_bm25_function_score(st, (uint32_t)n_items, (const DItem*)(db + o_items), (const DPart*)(db + o_parts), (const DTerm*)(wb + o_terms),
                               (const DQuery*)(db + o_queries), (const float*)(db + o_caches), (const DFuncQuery*)(db + o_fq),
                               (const DFuncMasks*)(db + o_fm), (unsigned long long*)(db + o_theta), (uint32_t*)(wb + o_ssum),
                               (uint64_t*)(wb + o_ikeys), (uint32_t*)(wb + o_icnt), (uint64_t*)(wb + o_ihits), hp.k_stride);
    if (timing) HIP_TRY(hipEventRecord(slot->ev1, st));
    HIP_TRY(hipEventRecord(slot->ev_turn, st));   // the turn ends behind the scorer, as in enqueue_search
    ctx->last_turn = slot->ev_turn;
    launch_merge_topk(st, (uint32_t)n_queries, (const uint64_t*)(wb + o_ikeys), (const uint32_t*)(wb + o_icnt), (const uint64_t*)(wb + o_ihits),
                      (const uint32_t*)(db + o_lidx), (const uint32_t*)(db + o_qbase), (const uint32_t*)(db + o_qnl), hp.k_stride,
                      (const uint32_t*)(db + o_qk), (uint64_t*)(wb + o_okeys), (uint32_t*)(wb + o_ocnt), (uint64_t*)(wb + o_ohits), hp.k_stride);
    launch_slice_relation(st, (const uint32_t*)(wb + o_ssum), (const DQuery*)(db + o_queries), hp.n_slices, (uint64_t*)(wb + o_ohits),
                          (uint32_t)n_queries);
    if (timing) HIP_TRY(hipEventRecord(slot->ev2, st));
  }
  HIP_TRY(hipGetLastError());
  *out_keys = (uint64_t*)(wb + o_okeys);
  *out_counts = (uint32_t*)(wb + o_ocnt);
  *out_hits = (uint64_t*)(wb + o_ohits);
  return NRTGPU_OK;
}

extern "C" int nrtgpu_search_function_score_batch(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                                  const nrtgpu_bm25_query* queries, const nrtgpu_function_score* functions,
                                                  int32_t n_queries, nrtgpu_topdocs* out) {
  if (!ctx || !queries || !functions || !out || (n_segs > 0 && !segs)) return fail(NRTGPU_ERR_INVALID_ARG, "NULL argument");
  if (n_queries <= 0 || n_segs < 0) return fail(NRTGPU_ERR_INVALID_ARG, "n_queries must be > 0");
  if (n_queries > ctx->cfg.max_batch) return fail(NRTGPU_ERR_INVALID_ARG, "batch of %d exceeds max_batch %d", n_queries, ctx->cfg.max_batch);
  for (int si = 0; si < n_segs; ++si)
    if (!segs[si]) return fail(NRTGPU_ERR_INVALID_ARG, "segment %d is NULL", si);
  NRT_CHECK_DEADLINE("before the search was planned");
  HIP_TRY(hipSetDevice(ctx->device));
  const double t0 = now_ms();
  SegReadLocks content(segs, n_segs);   // until this call's kernels have finished
  std::vector<DFuncQuery> records;
  records.reserve((size_t)n_queries);
  if (int rc = check_call(ctx, segs, n_segs, queries, functions, n_queries, &records)) return rc;
  HostPlan hp;
  if (int rc = plan_call(ctx, segs, doc_bases, n_segs, queries, n_queries, hp)) return rc;
  std::vector<DFuncMasks> fmasks;
  if (int rc = function_masks(segs, n_segs, functions, hp, &fmasks)) return rc;
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
  if (int rc = enqueue_function_score(ctx, slot, hp, records, fmasks, n_queries, &d_keys, &d_counts, &d_hits)) return rc;
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
