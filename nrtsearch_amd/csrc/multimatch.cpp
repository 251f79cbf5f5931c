// multimatch.cpp -- multi-match queries (include/nrtgpu.h: nrtgpu_search_multi_match_batch): the two-level shapes of the
// reference's multiMatchQuery -- a BooleanQuery over DisjunctionMaxQuery groups (cross_fields), a DisjunctionMaxQuery over
// BooleanQuery groups (best_fields).  The clauses are planned as the exhaustive route plans ONE SHOULD disjunction over all of
// them (build_plan, prune = 0, over reduced copies of the queries): the parts then cover every doc any clause matches, and the
// kernel alone decides what is a hit.  Beside the plan go one DGroupQuery per query, and every clause's group in its DQTerm
// (plan.h: kTabSlotGroupShift), which bm25_multi_match_kernel (multimatch.hip) reads.  The path from the plan to the caller's
// pages is finalscore.cpp's.
#include "runtime_internal.h"

namespace nrtgpu {
namespace rt {

// the record the kernel and nrtgpu_multi_match_value read, from the caller's struct; refusals by the header's table.
// occur: the clauses' nrtgpu_term.occur, or nullptr = all SHOULD
int group_record(const nrtgpu_clause_groups& g, int qi, int32_t n_terms, const int32_t* occur, int32_t min_should_match, DGroupQuery* out) {
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

}  // namespace rt
}  // namespace nrtgpu

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

namespace nrtgpu {
namespace rt {

// What the route refuses of the queries of a call before anything is planned; the records and the reduced copies of the queries
// (plain SHOULD disjunctions: what is planned) on the way.
int multi_match_check_queries(const nrtgpu_bm25_query* queries, const nrtgpu_clause_groups* groups, int32_t n_queries, std::vector<DGroupQuery>* records,
                              std::vector<nrtgpu_bm25_query>* flat, std::vector<std::vector<nrtgpu_term>>* flat_terms) {
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
  return NRTGPU_OK;
}

// The plan of the reduced queries, and every clause's group into its DQTerm.  hp.qterms holds one record per clause WHOSE TERM SOME
// LEAF HOLDS, in clause order (planner.cpp: resolve_queries skips a clause of total 0): the same test on the same cache entry here.
int multi_match_plan(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs, const nrtgpu_bm25_query* flat,
                     const nrtgpu_clause_groups* groups, int32_t n_queries, const char* route, HostPlan& hp) {
  if (int rc = final_score_plan(ctx, segs, doc_bases, n_segs, flat, n_queries, route, hp)) return rc;
  for (int qi = 0; qi < n_queries; ++qi) {
    const DQExpand& qx = hp.qexpand[(size_t)qi];
    uint32_t at = 0;
    for (int t = 0; t < flat[qi].n_terms; ++t) {
      const TermLeaves* tl = hp.lsc ? hp.lsc->get(segs, n_segs, flat[qi].terms[t].field_id, flat[qi].terms[t].term_hash) : nullptr;
      if (!tl || tl->total <= 0) continue;
      if (at >= qx.n_terms || (size_t)qx.term_begin + at >= hp.qterms.size() || hp.qterms[(size_t)qx.term_begin + at].table != tl->d_table)
        return fail(NRTGPU_ERR_STATE, "%s: the plan of query %d does not hold its clauses in clause order", route, qi);
      hp.qterms[(size_t)qx.term_begin + at].tab_slot |= ((uint32_t)groups[qi].group_of_term[t] & kTabSlotGroupMask) << kTabSlotGroupShift;
      ++at;
    }
    if (at != qx.n_terms) return fail(NRTGPU_ERR_STATE, "%s: the plan of query %d holds %u clauses, %u expected", route, qi, qx.n_terms, at);
  }
  return NRTGPU_OK;
}

}  // namespace rt
}  // namespace nrtgpu

// the queries' refusals, then the context's flags
static int check_call(nrtgpu_ctx* ctx, const nrtgpu_bm25_query* queries, const nrtgpu_clause_groups* groups, int32_t n_queries,
                      std::vector<DGroupQuery>* records, std::vector<nrtgpu_bm25_query>* flat, std::vector<std::vector<nrtgpu_term>>* flat_terms) {
  if (int rc = multi_match_check_queries(queries, groups, n_queries, records, flat, flat_terms)) return rc;
  return final_score_check_flags(ctx, "multi-match");
}

extern "C" int nrtgpu_multi_match_supported(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_bm25_query* q,
                                            const nrtgpu_clause_groups* g) {
  if (int rc = final_score_enter(ctx, segs, n_segs, !q || !g, nullptr)) return rc;
  SegReadLocks content(segs, n_segs);
  std::vector<nrtgpu_bm25_query> flat;
  std::vector<std::vector<nrtgpu_term>> flat_terms;
  if (int rc = check_call(ctx, q, g, 1, nullptr, &flat, &flat_terms)) return rc;
  HostPlan hp;   // the planner is the predicate for the clauses, as in nrtgpu_query_supported
  return multi_match_plan(ctx, segs, nullptr, n_segs, flat.data(), g, 1, "multi-match", hp);
}

extern "C" int nrtgpu_search_multi_match_batch(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                               const nrtgpu_bm25_query* queries, const nrtgpu_clause_groups* groups, int32_t n_queries,
                                               nrtgpu_topdocs* out) {
  if (int rc = final_score_enter(ctx, segs, n_segs, !queries || !groups || !out, &n_queries)) return rc;
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
  if (int rc = multi_match_plan(ctx, segs, doc_bases, n_segs, flat.data(), groups, n_queries, "multi-match", hp)) return rc;
  const PlanBytes extras[1] = {{records.data(), records.size() * sizeof(DGroupQuery)}};
  return final_score_run(ctx, hp, queries, n_queries, out, t0, extras, 1, [](hipStream_t st, const FinalScoreArgs& a, const void* const* d_extra) {
    launch_bm25_multi_match(st, a, (const DGroupQuery*)d_extra[0]);
  }, nullptr, true);   // (counts the hits behind a cursor per slice: slice_relation_past_kernel)
}
