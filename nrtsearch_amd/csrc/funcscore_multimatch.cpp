// funcscore_multimatch.cpp -- a function score over a multi-match query (include/nrtgpu.h:
// nrtgpu_search_function_score_multi_match_batch): MultiFunctionScoreQuery with weight functions around the two-level shapes of
// multiMatchQuery.  Both halves exist: the clauses are checked, reduced and planned as multimatch.cpp does it (one DGroupQuery per
// query, a clause's group in its DQTerm), the functions are checked and their doc sets looked up as funcscore.cpp does it (one
// DFuncQuery per query, one DFuncMasks per part of the reduced queries' plan).  bm25_multi_match_function_score_kernel
// (multimatch.hip) reads all three; the path from the plan to the caller's pages is finalscore.cpp's.
#include "runtime_internal.h"

static const char* const kRoute = "function-score multi-match";

extern "C" int nrtgpu_function_score_multi_match_value(const nrtgpu_clause_groups* g, int32_t n_terms, const int32_t* occur, int32_t min_should_match,
                                                       const float* clause_scores, uint32_t matched_clauses, const nrtgpu_function_score* fs,
                                                       uint32_t matched_functions, float* out_score, int32_t* out_is_hit) {
  if (!fs || !out_score || !out_is_hit) return fail(NRTGPU_ERR_INVALID_ARG, "NULL argument");
  float inner = 0.0f;
  int32_t inner_hit = 0;   // (the groups' rule as nrtgpu_multi_match_value states it: group_record, multi_match_group / _fold / _value)
  if (int rc = nrtgpu_multi_match_value(g, n_terms, occur, min_should_match, clause_scores, matched_clauses, &inner, &inner_hit)) return rc;
  DFuncQuery r;
  if (int rc = function_record(*fs, 0, &r)) return rc;
  *out_score = inner;
  *out_is_hit = 0;
  if (inner_hit) {   // a doc the groups reject is no hit whatever the functions say
    bool hit = false;
    *out_score = function_score_value(r, matched_functions, inner, &hit);
    *out_is_hit = hit ? 1 : 0;
  }
  return NRTGPU_OK;
}

// What the route refuses of a call before anything is planned, in the header's order; the records and the reduced queries on the way.
static int check_call(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_bm25_query* queries,
                      const nrtgpu_clause_groups* groups, const nrtgpu_function_score* functions, int32_t n_queries,
                      std::vector<DGroupQuery>* grecords, std::vector<DFuncQuery>* frecords, std::vector<nrtgpu_bm25_query>* flat,
                      std::vector<std::vector<nrtgpu_term>>* flat_terms) {
  if (int rc = multi_match_check_queries(queries, groups, n_queries, grecords, flat, flat_terms)) return rc;
  for (int qi = 0; qi < n_queries; ++qi) {
    DFuncQuery r;
    if (int rc = function_record(functions[qi], qi, &r)) return rc;
    if (frecords) frecords->push_back(r);
  }
  if (int rc = final_score_check_flags(ctx, kRoute)) return rc;
  for (int qi = 0; qi < n_queries; ++qi)
    if (int rc = function_masks_resident(segs, n_segs, functions[qi], qi)) return rc;
  return NRTGPU_OK;
}

extern "C" int nrtgpu_function_score_multi_match_supported(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_bm25_query* q,
                                                           const nrtgpu_clause_groups* g, const nrtgpu_function_score* fs) {
  if (int rc = final_score_enter(ctx, segs, n_segs, !q || !g || !fs, nullptr)) return rc;
  SegReadLocks content(segs, n_segs);
  std::vector<nrtgpu_bm25_query> flat;
  std::vector<std::vector<nrtgpu_term>> flat_terms;
  if (int rc = check_call(ctx, segs, n_segs, q, g, fs, 1, nullptr, nullptr, &flat, &flat_terms)) return rc;
  HostPlan hp;   // the planner is the predicate for the clauses, as in nrtgpu_query_supported
  return multi_match_plan(ctx, segs, nullptr, n_segs, flat.data(), g, 1, kRoute, hp);
}

extern "C" int nrtgpu_search_function_score_multi_match_batch(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                                              const nrtgpu_bm25_query* queries, const nrtgpu_clause_groups* groups,
                                                              const nrtgpu_function_score* functions, int32_t n_queries, nrtgpu_topdocs* out) {
  if (int rc = final_score_enter(ctx, segs, n_segs, !queries || !groups || !functions || !out, &n_queries)) return rc;
  const double t0 = now_ms();
  SegReadLocks content(segs, n_segs);   // until this call's kernels have finished
  std::vector<DGroupQuery> grecords;
  std::vector<DFuncQuery> frecords;
  std::vector<nrtgpu_bm25_query> flat;
  std::vector<std::vector<nrtgpu_term>> flat_terms;
  grecords.reserve((size_t)n_queries);
  frecords.reserve((size_t)n_queries);
  flat.reserve((size_t)n_queries);
  flat_terms.reserve((size_t)n_queries);
  if (int rc = check_call(ctx, segs, n_segs, queries, groups, functions, n_queries, &grecords, &frecords, &flat, &flat_terms)) return rc;
  HostPlan hp;
  if (int rc = multi_match_plan(ctx, segs, doc_bases, n_segs, flat.data(), groups, n_queries, kRoute, hp)) return rc;
  std::vector<DFuncMasks> fmasks;   // per part of the reduced queries' plan
  if (int rc = function_masks(segs, n_segs, functions, hp, &fmasks)) return rc;
  const PlanBytes extras[3] = {{grecords.data(), grecords.size() * sizeof(DGroupQuery)},
                               {frecords.data(), frecords.size() * sizeof(DFuncQuery)},
                               {fmasks.data(), fmasks.size() * sizeof(DFuncMasks)}};
  return final_score_run(ctx, hp, queries, n_queries, out, t0, extras, 3, [](hipStream_t st, const FinalScoreArgs& a, const void* const* d_extra) {
    launch_bm25_multi_match_function_score(st, a, (const DGroupQuery*)d_extra[0], (const DFuncQuery*)d_extra[1], (const DFuncMasks*)d_extra[2]);
  }, nullptr, true);   // (counts the hits behind a cursor per slice: slice_relation_past_kernel)
}
