// multimatch.cpp -- multi-match queries (include/nrtgpu.h: nrtgpu_search_multi_match_batch): the two-level shapes of the
// reference's multiMatchQuery -- a BooleanQuery over DisjunctionMaxQuery groups (cross_fields), a DisjunctionMaxQuery over
// BooleanQuery groups (best_fields).  The clauses are planned as the exhaustive route plans ONE SHOULD disjunction over all of
// them (build_plan, prune = 0, over reduced copies of the queries): the parts then cover every doc any clause matches, and the
// kernel alone decides what is a hit.  Beside the plan go one DGroupQuery per query, and every clause's group in its DQTerm
// (plan.h: kTabSlotGroupShift).  On the device: the existing plan expansion, then bm25_multi_match_kernel (multimatch.hip) over all
// items, then the existing merge and per-slice relation -- funcscore.cpp's sequence with another scorer.
#include "runtime_internal.h"

// the record the kernel and nrtgpu_multi_match_value read, from the caller's struct; refusals by the header's table.
// occur: the clauses' nrtgpu_term.occur, or nullptr = all SHOULD
static int group_record(const nrtgpu_clause_groups& g, int qi, int32_t n_terms, const int32_t* occur, int32_t min_should_match, DGroupQuery* out) {
  if (g.shape != NRTGPU_GROUPS_SUM_OF_MAX && g.shape != NRTGPU_GROUPS_MAX_OF_SUM)
    return fail(NRTGPU_ERR_INVALID_ARG, "query %d: shape %d outside 0..1", qi, g.shape);
  if (g.n_groups < 1 || g.n_groups > NRTGPU_MAX_GROUPS)
    return fail(NRTGPU_ERR_INVALID_ARG, "query %d: n_groups %d outside 1..%d", qi, g.n_groups, NRTGPU_MAX_GROUPS);
  if (!g.group_of_term) return fail(NRTGPU_ERR_INVALID_ARG, "query %d: group_of_term is NULL", qi);
  if (!std::isfinite(g.tie_breaker) || g.tie_breaker < 0.0f || g.tie_breaker > 1.0f)
    return fail(NRTGPU_ERR_INVALID_ARG, "query %d: the groups' tie_breaker must be in [0, 1]", qi);
  if (g.group_occur != 0 && g.group_occur != 1) return fail(NRTGPU_ERR_INVALID_ARG, "query %d: group_occur must be 0 or 1", qi);
  if (n_terms < 1) return fail(NRTGPU_ERR_INVALID_ARG, "query %d: no terms", qi);
  if (n_terms > NRTGPU_MAX_TERMS) return fail(NRTGPU_ERR_UNSUPPORTED, "query %d: %d clauses > %d", qi, n_terms, NRTGPU_MAX_TERMS);
  if (min_should_match < 0) return fail(NRTGPU_ERR_INVALID_ARG, "query %d: minimumNumberShouldMatch %d", qi, min_should_match);
  DGroupQuery r{};
  r.shape = (uint32_t)g.shape;
  r.n_groups = (uint32_t)g.n_groups;
  r.tie_breaker = g.tie_breaker;
  r.group_occur = (uint32_t)g.group_occur;
  r.min_should_match = (uint32_t)min_should_match;
  int n_must[NRTGPU_MAX_GROUPS] = {};
  for (int t = 0; t < n_terms; ++t) {
    const int32_t gi = g.group_of_term[t];
    if (gi < 0 || gi >= g.n_groups) return fail(NRTGPU_ERR_INVALID_ARG, "query %d term %d: group %d outside 0..%d", qi, t, gi, g.n_groups - 1);
    const int32_t oc = occur ? occur[t] : 0;
    if (oc != 0 && oc != 1) return fail(NRTGPU_ERR_INVALID_ARG, "query %d term %d: occur must be 0 (SHOULD) or 1 (MUST)", qi, t);
    r.n_clauses[gi] += 1;
    n_must[gi] += oc;
  }
  for (int gi = 0; gi < g.n_groups; ++gi)
    if (r.n_clauses[gi] == 0) return fail(NRTGPU_ERR_INVALID_ARG, "query %d: group %d is empty", qi, gi);
  if (g.shape == NRTGPU_GROUPS_SUM_OF_MAX) {
    for (int gi = 0; gi < g.n_groups; ++gi)
      if (n_must[gi] != 0) return fail(NRTGPU_ERR_INVALID_ARG, "query %d: the disjuncts of a DisjunctionMax group have no occur", qi);
  } else {
    if (g.group_occur != 0) return fail(NRTGPU_ERR_INVALID_ARG, "query %d: the disjuncts of the outer DisjunctionMaxQuery have no occur (group_occur)", qi);
    if (min_should_match != 0)
      return fail(NRTGPU_ERR_INVALID_ARG, "query %d: the outer DisjunctionMaxQuery has no minimumNumberShouldMatch (use group_min_should_match)", qi);
    for (int gi = 0; gi < g.n_groups; ++gi) {
      const int32_t m = g.group_min_should_match ? g.group_min_should_match[gi] : 0;
      if (m < 0) return fail(NRTGPU_ERR_INVALID_ARG, "query %d group %d: minimumNumberShouldMatch %d", qi, gi, m);
      r.min_match[gi] = (uint8_t)std::min<int32_t>(m, 255);
    }
    for (int gi = 0; gi < g.n_groups; ++gi) {
      if (n_must[gi] != 0 && n_must[gi] != (int)r.n_clauses[gi])
        return fail(NRTGPU_ERR_UNSUPPORTED, "query %d group %d: MUST next to SHOULD clauses inside a group", qi, gi);
      r.occur[gi] = n_must[gi] != 0 ? 1 : 0;
    }
  }
  if (out) *out = r;
  return NRTGPU_OK;
}

extern "C" int nrtgpu_multi_match_value(const nrtgpu_clause_groups* g, int32_t n_terms, const int32_t* occur, int32_t min_should_match,
                                        const float* clause_scores, uint32_t matched, float* out_score, int32_t* out_is_hit) {
  if (!g || !clause_scores || !out_score || !out_is_hit) return fail(NRTGPU_ERR_INVALID_ARG, "NULL argument");
  DGroupQuery r;
  if (int rc = group_record(*g, 0, n_terms, occur, min_should_match, &r)) return rc;
  MmOuter o{0.0, 0.0f, 0u};
  for (int gi = 0; gi < g->n_groups; ++gi) {   // groups in order, a group's clauses in clause order: the double sums' order
    double sum = 0.0;
    float best = 0.0f;
    uint32_t count = 0;
    for (int t = 0; t < n_terms; ++t) {
      if (g->group_of_term[t] != gi || ((matched >> t) & 1u) == 0u) continue;
      sum += (double)clause_scores[t];
      best = clause_scores[t] > best ? clause_scores[t] : best;
      count += 1u;
    }
    float group_score;
    if (count != 0u && multi_match_group(r, (uint32_t)gi, sum, best, count, &group_score)) multi_match_fold(o, group_score);
  }
  bool hit = false;
  *out_score = 0.0f;
  if (o.n != 0u) *out_score = multi_match_value(r, o, &hit);
  *out_is_hit = hit ? 1 : 0;
  return NRTGPU_OK;
}

// What the route refuses of a call before anything is planned; the records and the reduced copies of the queries (plain SHOULD
// disjunctions: what is planned) on the way.
static int check_call(nrtgpu_ctx* ctx, const nrtgpu_bm25_query* queries, const nrtgpu_clause_groups* groups, int32_t n_queries,
                      std::vector<DGroupQuery>* records, std::vector<nrtgpu_bm25_query>* flat, std::vector<std::vector<nrtgpu_term>>* flat_terms) {
  for (int qi = 0; qi < n_queries; ++qi) {
    const nrtgpu_bm25_query& q = queries[qi];
    if (q.disjunction_max != 0 || q.tie_breaker != 0.0f)
      return fail(NRTGPU_ERR_INVALID_ARG, "query %d: disjunction_max / tie_breaker must be 0 (the structure lives in the groups)", qi);
    nrtgpu_bm25_query f = q;
    std::vector<nrtgpu_term> ft;
    int32_t occur[NRTGPU_MAX_TERMS] = {};
    if (q.n_terms > 0 && q.n_terms <= NRTGPU_MAX_TERMS && q.terms) {
      ft.assign(q.terms, q.terms + q.n_terms);
      for (int t = 0; t < q.n_terms; ++t) {
        occur[t] = ft[(size_t)t].occur;
        ft[(size_t)t].occur = occur[t] == 1 ? 0 : occur[t];   // (anything else stays for validate_query to refuse)
      }
      f.terms = ft.data();
    }
    f.min_should_match = q.min_should_match < 0 ? q.min_should_match : 0;
    if (int rc = validate_query(f, qi)) return rc;
    DGroupQuery r;
    if (int rc = group_record(groups[qi], qi, q.n_terms, occur, q.min_should_match, &r)) return rc;
    if (q.min_competitive_score != 0.0f) return fail(NRTGPU_ERR_UNSUPPORTED, "query %d: a multi-match query with a min_competitive_score", qi);
    if (records) records->push_back(r);
    flat_terms->push_back(std::move(ft));
    flat->push_back(f);
  }
  for (int qi = 0; qi < n_queries; ++qi) (*flat)[(size_t)qi].terms = (*flat_terms)[(size_t)qi].data();   // (the vectors have settled)
  if (ctx->cfg.flags & NRTGPU_FLAG_PACKED_POSTINGS)
    return fail(NRTGPU_ERR_UNSUPPORTED, "multi-match queries do not run over packed postings (NRTGPU_FLAG_PACKED_POSTINGS)");
  if (ctx->cfg.flags & NRTGPU_FLAG_NO_FIXED_POINT)
    return fail(NRTGPU_ERR_UNSUPPORTED, "multi-match queries need the fixed-point accumulators (NRTGPU_FLAG_NO_FIXED_POINT is set)");
  return NRTGPU_OK;
}

// The plan of the reduced queries, and every clause's group into its DQTerm.  hp.qterms holds one record per clause WHOSE TERM SOME
// LEAF HOLDS, in clause order (planner.cpp: resolve_queries skips a clause of total 0): the same test on the same cache entry here.
static int plan_call(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs, const nrtgpu_bm25_query* flat,
                     const nrtgpu_clause_groups* groups, int32_t n_queries, HostPlan& hp) {
  if (int rc = build_plan(ctx, segs, doc_bases, n_segs, flat, n_queries, hp, 0)) return rc;
  if (!hp.fixed_point)
    return fail(NRTGPU_ERR_UNSUPPORTED, "multi-match queries need the fixed-point accumulators (the weights of a query in this batch span too many binades)");
  for (int qi = 0; qi < n_queries; ++qi) {
    const DQExpand& qx = hp.qexpand[(size_t)qi];
    uint32_t at = 0;
    for (int t = 0; t < flat[qi].n_terms; ++t) {
      const TermLeaves* tl = hp.lsc ? hp.lsc->get(segs, n_segs, flat[qi].terms[t].field_id, flat[qi].terms[t].term_hash) : nullptr;
      if (!tl || tl->total <= 0) continue;
      if (at >= qx.n_terms || (size_t)qx.term_begin + at >= hp.qterms.size() || hp.qterms[(size_t)qx.term_begin + at].table != tl->d_table)
        return fail(NRTGPU_ERR_STATE, "multi-match: the plan of query %d does not hold its clauses in clause order", qi);
      hp.qterms[(size_t)qx.term_begin + at].tab_slot |= ((uint32_t)groups[qi].group_of_term[t] & kTabSlotGroupMask) << kTabSlotGroupShift;
      ++at;
    }
    if (at != qx.n_terms) return fail(NRTGPU_ERR_STATE, "multi-match: the plan of query %d holds %u clauses, %u expected", qi, qx.n_terms, at);
  }
  return NRTGPU_OK;
}

extern "C" int nrtgpu_multi_match_supported(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_bm25_query* q,
                                            const nrtgpu_clause_groups* g) {
  if (!ctx || !q || !g || (n_segs > 0 && !segs)) return fail(NRTGPU_ERR_INVALID_ARG, "NULL argument");
  if (n_segs < 0) return fail(NRTGPU_ERR_INVALID_ARG, "n_segs must be >= 0");
  for (int si = 0; si < n_segs; ++si)
    if (!segs[si]) return fail(NRTGPU_ERR_INVALID_ARG, "segment %d is NULL", si);
  HIP_TRY(hipSetDevice(ctx->device));
  SegReadLocks content(segs, n_segs);
  std::vector<nrtgpu_bm25_query> flat;
  std::vector<std::vector<nrtgpu_term>> flat_terms;
  if (int rc = check_call(ctx, q, g, 1, nullptr, &flat, &flat_terms)) return rc;
  HostPlan hp;   // the planner is the predicate for the clauses, as in nrtgpu_query_supported
  return plan_call(ctx, segs, nullptr, n_segs, flat.data(), g, 1, hp);
}

// Plan upload, expansion, the multi-match kernel over all items, merge, per-slice relation: enqueued at once on the slot's stream
// (funcscore.cpp: enqueue_function_score, with the group records in place of the function records and masks).
static int enqueue_multi_match(nrtgpu_ctx* ctx, Slot* slot, const HostPlan& hp, const std::vector<DGroupQuery>& records, int32_t n_queries,
                               uint64_t** out_keys, uint32_t** out_counts, uint64_t** out_hits) {
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
  const size_t o_gq = pc.take(records.size() * sizeof(DGroupQuery));
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
  put(o_gq, records.data(), records.size() * sizeof(DGroupQuery));
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
    launch_bm25_multi_match(st, (uint32_t)n_items, (const DItem*)(db + o_items), (const DPart*)(db + o_parts), (const DTerm*)(wb + o_terms),
                            (const DQuery*)(db + o_queries), (const float*)(db + o_caches), (const DGroupQuery*)(db + o_gq),
                            (unsigned long long*)(db + o_theta), (uint32_t*)(wb + o_ssum), (uint64_t*)(wb + o_ikeys), (uint32_t*)(wb + o_icnt),
                            (uint64_t*)(wb + o_ihits), hp.k_stride);
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

extern "C" int nrtgpu_search_multi_match_batch(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                               const nrtgpu_bm25_query* queries, const nrtgpu_clause_groups* groups, int32_t n_queries,
                                               nrtgpu_topdocs* out) {
  if (!ctx || !queries || !groups || !out || (n_segs > 0 && !segs)) return fail(NRTGPU_ERR_INVALID_ARG, "NULL argument");
  if (n_queries <= 0 || n_segs < 0) return fail(NRTGPU_ERR_INVALID_ARG, "n_queries must be > 0");
  if (n_queries > ctx->cfg.max_batch) return fail(NRTGPU_ERR_INVALID_ARG, "batch of %d exceeds max_batch %d", n_queries, ctx->cfg.max_batch);
  for (int si = 0; si < n_segs; ++si)
    if (!segs[si]) return fail(NRTGPU_ERR_INVALID_ARG, "segment %d is NULL", si);
  NRT_CHECK_DEADLINE("before the search was planned");
  HIP_TRY(hipSetDevice(ctx->device));
  const double t0 = now_ms();
  SegReadLocks content(segs, n_segs);   // until this call's kernels have finished
  std::vector<DGroupQuery> records;
  std::vector<nrtgpu_bm25_query> flat;
  std::vector<std::vector<nrtgpu_term>> flat_terms;
  records.reserve((size_t)n_queries);
  flat.reserve((size_t)n_queries);
  flat_terms.reserve((size_t)n_queries);
  if (int rc = check_call(ctx, queries, groups, n_queries, &records, &flat, &flat_terms)) return rc;
  HostPlan hp;
  if (int rc = plan_call(ctx, segs, doc_bases, n_segs, flat.data(), groups, n_queries, hp)) return rc;
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
  if (int rc = enqueue_multi_match(ctx, slot, hp, records, n_queries, &d_keys, &d_counts, &d_hits)) return rc;
  HIP_TRY(hipMemcpyAsync(ho + o_k, d_keys, kb, hipMemcpyDeviceToHost, slot->stream));
  HIP_TRY(hipMemcpyAsync(ho + o_c, d_counts, cb, hipMemcpyDeviceToHost, slot->stream));
  HIP_TRY(hipMemcpyAsync(ho + o_h, d_hits, hb, hipMemcpyDeviceToHost, slot->stream));
  HIP_TRY(wait_for_stream((ctx->cfg.flags & NRTGPU_FLAG_BLOCKING_WAIT) != 0, slot->stream, slot->ev_wait));
  const uint64_t* keys = (const uint64_t*)(ho + o_k);
  const uint32_t* cnts = (const uint32_t*)(ho + o_c);
  const uint64_t* hits = (const uint64_t*)(ho + o_h);
  for (int qi = 0; qi < n_queries; ++qi) {
    // (as nrtgpu_search_function_score_batch unpacks: the count is exact; the high bits of `hits` carry slice_relation_kernel's
    // tag, and a page shorter than numHits is EQUAL_TO)
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
