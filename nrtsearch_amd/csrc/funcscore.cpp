// funcscore.cpp -- function-score queries (include/nrtgpu.h: nrtgpu_search_function_score_batch): MultiFunctionScoreQuery with
// weight functions over a BM25 disjunction.  The inner queries are planned as the exhaustive route plans them (build_plan,
// prune = 0: the reference scores the wrapper under ScoreMode.COMPLETE, nothing may be skipped); beside the plan go one
// DFuncQuery per query and one DFuncMasks per part (plan.h), which bm25_function_score_kernel (funcscore.hip) reads.  The path
// from the plan to the caller's pages is finalscore.cpp's.
#include "runtime_internal.h"

namespace nrtgpu {
namespace rt {

// the record the kernels and nrtgpu_function_score_value read, from the caller's struct; refusals by the header's table
int function_record(const nrtgpu_function_score& fs, int qi, DFuncQuery* out) {
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

int function_masks_resident(const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_function_score& fs, int qi) {
  for (int i = 0; i < fs.n_functions; ++i) {
    const int32_t id = fs.functions[i].filter_mask;
    if (id == 0) continue;
    for (int si = 0; si < n_segs; ++si)
      if (segs[si]->masks.find(id) == segs[si]->masks.end())
        return fail(NRTGPU_ERR_UNSUPPORTED, "query %d function %d: mask %d is not resident on segment %d", qi, i, id, si);
  }
  return NRTGPU_OK;
}

}  // namespace rt
}  // namespace nrtgpu

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
  if (int rc = final_score_check_flags(ctx, "function-score")) return rc;
  for (int qi = 0; qi < n_queries; ++qi) {
    const nrtgpu_bm25_query& q = queries[qi];
    if (q.disjunction_max != 0) return fail(NRTGPU_ERR_UNSUPPORTED, "query %d: a function score over a DisjunctionMaxQuery", qi);
    for (int t = 0; t < q.n_terms; ++t)
      if (q.terms[t].occur != 0) return fail(NRTGPU_ERR_UNSUPPORTED, "query %d: a function score over MUST clauses", qi);
    if (q.min_should_match > 1) return fail(NRTGPU_ERR_UNSUPPORTED, "query %d: a function score over minimumNumberShouldMatch %d", qi, q.min_should_match);
    if (q.min_competitive_score != 0.0f) return fail(NRTGPU_ERR_UNSUPPORTED, "query %d: a function score with a min_competitive_score", qi);
    if (int rc = function_masks_resident(segs, n_segs, functions[qi], qi)) return rc;
  }
  return NRTGPU_OK;
}

extern "C" int nrtgpu_function_score_supported(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_bm25_query* q,
                                               const nrtgpu_function_score* fs) {
  if (int rc = final_score_enter(ctx, segs, n_segs, !q || !fs, nullptr)) return rc;
  SegReadLocks content(segs, n_segs);
  if (int rc = check_call(ctx, segs, n_segs, q, fs, 1, nullptr)) return rc;
  HostPlan hp;   // the planner is the predicate for the inner query, as in nrtgpu_query_supported
  return final_score_plan(ctx, segs, nullptr, n_segs, q, 1, "function-score", hp);
}

namespace nrtgpu {
namespace rt {

// The doc sets of every function on every part's leaf.  A part names its (query, leaf) pair by its first DTerm (HostPlan.qs_begin).
int function_masks(const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_function_score* functions, const HostPlan& hp,
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

}  // namespace rt
}  // namespace nrtgpu

extern "C" int nrtgpu_search_function_score_batch(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                                  const nrtgpu_bm25_query* queries, const nrtgpu_function_score* functions,
                                                  int32_t n_queries, nrtgpu_topdocs* out) {
  if (int rc = final_score_enter(ctx, segs, n_segs, !queries || !functions || !out, &n_queries)) return rc;
  const double t0 = now_ms();
  SegReadLocks content(segs, n_segs);   // until this call's kernels have finished
  std::vector<DFuncQuery> records;
  records.reserve((size_t)n_queries);
  if (int rc = check_call(ctx, segs, n_segs, queries, functions, n_queries, &records)) return rc;
  HostPlan hp;
  if (int rc = final_score_plan(ctx, segs, doc_bases, n_segs, queries, n_queries, "function-score", hp)) return rc;
  std::vector<DFuncMasks> fmasks;
  if (int rc = function_masks(segs, n_segs, functions, hp, &fmasks)) return rc;
  const PlanBytes extras[2] = {{records.data(), records.size() * sizeof(DFuncQuery)}, {fmasks.data(), fmasks.size() * sizeof(DFuncMasks)}};
  return final_score_run(ctx, hp, queries, n_queries, out, t0, extras, 2, [](hipStream_t st, const FinalScoreArgs& a, const void* const* d_extra) {
    launch_bm25_function_score(st, a, (const DFuncQuery*)d_extra[0], (const DFuncMasks*)d_extra[1]);
  }, nullptr, true);   // (counts the hits behind a cursor per slice: slice_relation_past_kernel)
}
