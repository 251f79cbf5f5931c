// fieldsort.cpp -- sort by field (include/nrtgpu.h: nrtgpu_search_sorted_batch): a text query's hits ordered by an int or float
// doc value column of the segment store (segment.cpp: nrtgpu_segment_add_doc_values) instead of by score.  The queries are
// planned as the exhaustive route plans plain SHOULD disjunctions (build_plan, prune = 0, over copies with occur and
// min_should_match cleared): the parts then cover every doc any clause matches, and bm25_field_sort_kernel (fieldsort.hip) counts
// clauses per doc and decides what is a hit from the route's own record -- the planner's MUST / minimumNumberShouldMatch special
// cases stay out of the route.  Beside the plan go one DSortQuery per query and one DSortPart per part (plan.h).  The path from
// the plan to the caller's pages is finalscore.cpp's: the keys' high words are the values' codes where the other routes have
// score bits, and unpack_topdocs is a bit copy -- the codes are turned back into value bits here.
#include <cstddef>

#include "runtime_internal.h"

static_assert(sizeof(nrtgpu_fielddocs) == sizeof(nrtgpu_topdocs) && offsetof(nrtgpu_fielddocs, docs) == offsetof(nrtgpu_topdocs, docs) &&
                  offsetof(nrtgpu_fielddocs, value_bits) == offsetof(nrtgpu_topdocs, scores) &&
                  offsetof(nrtgpu_fielddocs, total_hits) == offsetof(nrtgpu_topdocs, total_hits) &&
                  offsetof(nrtgpu_fielddocs, total_hits_is_lower_bound) == offsetof(nrtgpu_topdocs, total_hits_is_lower_bound),
              "nrtgpu_fielddocs is nrtgpu_topdocs with value bits where the scores are");
static_assert(sizeof(nrtgpu_field_sort) == 24, "nrtgpu_field_sort layout");

extern "C" int nrtgpu_sort_value_code(int32_t kind, int32_t reverse, uint32_t value_bits, uint32_t* out_key_high) {
  if (!out_key_high) return fail(NRTGPU_ERR_INVALID_ARG, "NULL argument");
  if (kind != NRTGPU_DOCVALUES_INT32 && kind != NRTGPU_DOCVALUES_FLOAT32) return fail(NRTGPU_ERR_INVALID_ARG, "doc values kind %d outside 0..1", kind);
  if (reverse != 0 && reverse != 1) return fail(NRTGPU_ERR_INVALID_ARG, "reverse %d outside 0..1", reverse);
  *out_key_high = sort_key_high((uint32_t)reverse, doc_value_code(kind, value_bits));
  return NRTGPU_OK;
}

namespace nrtgpu {
namespace rt {

// ---- what the routes over a doc value column share (this file: sorted searches; termscount.cpp: the terms aggregation) ----------
// The kind and the arity of the field's column over the leaves of the call; refusals by the header's table.
int doc_values_kind(const nrtgpu_seg* const* segs, int32_t n_segs, int32_t field_id, int qi, int* kind, bool* multi) {
  *kind = -1;
  *multi = false;
  for (int si = 0; si < n_segs; ++si) {
    const auto fit = segs[si]->fields.find(field_id);
    if (fit == segs[si]->fields.end() || fit->second.dv_kind < 0) continue;
    const bool m = fit->second.d_dv_start != nullptr;
    if (*kind >= 0 && *kind != fit->second.dv_kind)
      return fail(NRTGPU_ERR_INVALID_ARG, "query %d: the leaves of the call hold the doc values of field %d under different kinds (segment %d)", qi, field_id, si);
    if (*kind >= 0 && *multi != m)
      return fail(NRTGPU_ERR_INVALID_ARG, "query %d: the leaves of the call hold the doc values of field %d single-valued and multi-valued (segment %d)", qi, field_id, si);
    *kind = fit->second.dv_kind;
    *multi = m;
  }
  return NRTGPU_OK;
}

DSortPart doc_values_column(const nrtgpu_seg* seg, int32_t field_id) {
  const auto fit = seg->fields.find(field_id);
  if (fit == seg->fields.end() || fit->second.dv_kind < 0) return DSortPart{nullptr, nullptr};
  const FieldData& f = fit->second;
  return f.d_dv_start != nullptr ? DSortPart{f.d_dv_code, (const uint64_t*)f.d_dv_start} : DSortPart{f.d_dv_code, f.d_dv_has};
}

int doc_values_wide(int qi, int32_t field_id, const char* instead) {
  return fail(NRTGPU_ERR_UNSUPPORTED, "query %d: the doc values of field %d are a 64-bit column: %s", qi, field_id, instead);
}

// What the sorted routes refuse of a sort over a multi-valued column (beside "resident on no leaf": the column names no ONE value).
int field_sort_multi(int qi, int32_t field_id) {
  return fail(NRTGPU_ERR_UNSUPPORTED, "query %d: the doc values of field %d are multi-valued: a sort names one value per doc (upload the selector's pick, "
              "SortedNumericSelector MIN / MAX, as a single-valued column of its own)", qi, field_id);
}

int doc_values_masks_resident(const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_bm25_query& q, int qi) {
  auto resident = [&](int32_t id, const char* what) -> int {
    for (int si = 0; id != 0 && si < n_segs; ++si)
      if (segs[si]->masks.find(id) == segs[si]->masks.end())
        return fail(NRTGPU_ERR_UNSUPPORTED, "query %d: %s mask %d is not resident on segment %d", qi, what, id, si);
    return NRTGPU_OK;
  };
  if (int rc = resident(q.filter_mask, "filter")) return rc;
  if (int rc = resident(q.must_not_mask, "must_not")) return rc;
  for (int i = 0; i < q.n_more_filters; ++i)
    if (int rc = resident(q.more_filters[i], "filter")) return rc;
  for (int i = 0; i < q.n_more_must_not; ++i)
    if (int rc = resident(q.more_must_not[i], "must_not")) return rc;
  return NRTGPU_OK;
}

// What both routes refuse of one query as unsupported (kind: doc_values_kind's; under: "a sort" / "a terms count"); *need: the
// clauses a hit matches at least; the copy that is planned on the way.
int doc_values_query(const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_bm25_query& q, int qi, int kind, int32_t field_id, const char* under,
                     uint32_t* need, FlatQueries* flat) {
  if (kind < 0) return fail(NRTGPU_ERR_UNSUPPORTED, "query %d: no leaf of the call holds doc values of field %d", qi, field_id);
  if (q.disjunction_max != 0 || q.tie_breaker != 0.0f)
    return fail(NRTGPU_ERR_UNSUPPORTED, "query %d: a DisjunctionMaxQuery under %s (pass its clauses as a plain disjunction: scores are not read)", qi, under);
  int n_must = 0;
  for (int t = 0; t < q.n_terms; ++t) n_must += q.terms[t].occur;
  if (n_must != 0 && n_must != q.n_terms) return fail(NRTGPU_ERR_UNSUPPORTED, "query %d: MUST next to SHOULD clauses under %s", qi, under);
  if (q.min_competitive_score != 0.0f) return fail(NRTGPU_ERR_UNSUPPORTED, "query %d: a min_competitive_score under %s", qi, under);
  if (int rc = doc_values_masks_resident(segs, n_segs, q, qi)) return rc;
  *need = n_must != 0 ? (uint32_t)q.n_terms : (uint32_t)std::max(q.min_should_match, 1);
  nrtgpu_bm25_query f = q;
  flat->terms.emplace_back(q.terms, q.terms + q.n_terms);
  for (nrtgpu_term& t : flat->terms.back()) t.occur = 0;
  f.min_should_match = 0;
  flat->queries.push_back(f);
  return NRTGPU_OK;
}

// The sort's side of the query's record (kind: of the column over the leaves; `need` is the caller's).
void field_sort_record(const nrtgpu_field_sort& s, int kind, DSortQuery* r) {
  r->reverse = (uint32_t)s.reverse;
  r->missing_code = doc_value_code(kind, s.missing_bits);
  r->has_after = (uint32_t)s.has_after;
  r->after_key = s.has_after ? sort_key(r->reverse, doc_value_code(kind, s.after_bits), (uint32_t)s.after_doc) : ~0ull;
}

void field_sort_values(const std::vector<DSortQuery>& records, const std::vector<int>& kinds, int32_t n_queries, nrtgpu_fielddocs* out) {
  for (int qi = 0; qi < n_queries; ++qi) {
    uint32_t* v = out[qi].value_bits;
    const uint32_t reverse = records[(size_t)qi].reverse;
    for (int32_t i = 0; v && i < out[qi].n_hits; ++i) v[i] = doc_value_bits(kinds[(size_t)qi], reverse != 0u ? v[i] : ~v[i]);
  }
}

// The leaf of every part.  A part names its (query, leaf) pair by its first DTerm (HostPlan.qs_begin).
int doc_values_part_leaves(const nrtgpu_seg* const* segs, int32_t n_segs, const HostPlan& hp, const char* route, std::vector<int32_t>* out) {
  out->assign(hp.parts.size(), -1);
  for (const DItem& it : hp.items) {
    for (uint32_t pi = 0; pi < it.n_parts; ++pi) {
      const DPart& p = hp.parts[it.part_begin + pi];
      int32_t leaf = -1;
      for (int32_t si = 0; si < n_segs && leaf < 0; ++si)
        if (hp.qs_begin[(size_t)it.query * (size_t)n_segs + (size_t)si] == p.term_begin) leaf = si;
      if (leaf < 0 || (uint32_t)segs[leaf]->max_doc != p.max_doc) return fail(NRTGPU_ERR_STATE, "%s: a part of query %u names no leaf", route, it.query);
      (*out)[it.part_begin + pi] = leaf;
    }
  }
  return NRTGPU_OK;
}

// The column of every part's leaf (field_ids: per query).
int doc_values_parts(const nrtgpu_seg* const* segs, int32_t n_segs, const int32_t* field_ids, const HostPlan& hp, const char* route,
                     std::vector<DSortPart>* out) {
  std::vector<int32_t> leaves;
  if (int rc = doc_values_part_leaves(segs, n_segs, hp, route, &leaves)) return rc;
  out->assign(hp.parts.size(), DSortPart{nullptr, nullptr});
  for (const DItem& it : hp.items)
    for (uint32_t pi = 0; pi < it.n_parts; ++pi) (*out)[it.part_begin + pi] = doc_values_column(segs[leaves[it.part_begin + pi]], field_ids[it.query]);
  return NRTGPU_OK;
}

}  // namespace rt
}  // namespace nrtgpu

namespace {

// What the route refuses of a call before anything is planned (the segments' content is held); the records and the copies that
// are planned on the way.
int check_call(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_bm25_query* queries, const nrtgpu_field_sort* sorts,
               int32_t n_queries, std::vector<DSortQuery>* records, std::vector<int>* kinds, FlatQueries* flat) {
  flat->queries.reserve((size_t)n_queries);
  flat->terms.reserve((size_t)n_queries);
  std::vector<char> multi;
  for (int qi = 0; qi < n_queries; ++qi) {
    const nrtgpu_bm25_query& q = queries[qi];
    const nrtgpu_field_sort& s = sorts[qi];
    if (int rc = validate_query(q, qi)) return rc;
    if (int rc = field_sort_check(s, qi)) return rc;
    if (q.has_after != 0) return fail(NRTGPU_ERR_INVALID_ARG, "query %d: the query's has_after must be 0 (the cursor of a sorted search lives in the sort)", qi);
    int kind = -1;
    bool m = false;
    if (int rc = doc_values_kind(segs, n_segs, s.field_id, qi, &kind, &m)) return rc;
    kinds->push_back(kind);
    multi.push_back(m ? 1 : 0);
  }
  if (int rc = final_score_check_flags(ctx, "sorted")) return rc;
  for (int qi = 0; qi < n_queries; ++qi) {
    const nrtgpu_field_sort& s = sorts[qi];
    const int kind = (*kinds)[(size_t)qi];
    DSortQuery r{};
    if (kind >= kDocValuesInt64) return doc_values_wide(qi, s.field_id, "sort by it with nrtgpu_search_sorted64_batch");
    if (multi[(size_t)qi] != 0) return field_sort_multi(qi, s.field_id);
    if (int rc = doc_values_query(segs, n_segs, queries[qi], qi, kind, s.field_id, "a sort", &r.need, flat)) return rc;
    field_sort_record(s, kind, &r);
    if (records) records->push_back(r);
  }
  for (int qi = 0; qi < n_queries; ++qi) flat->queries[(size_t)qi].terms = flat->terms[(size_t)qi].data();   // (the vectors have settled)
  return NRTGPU_OK;
}

}  // namespace

extern "C" int nrtgpu_sorted_supported(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_bm25_query* q,
                                       const nrtgpu_field_sort* s) {
  if (int rc = final_score_enter(ctx, segs, n_segs, !q || !s, nullptr)) return rc;
  SegReadLocks content(segs, n_segs);
  std::vector<int> kinds;
  FlatQueries flat;
  if (int rc = check_call(ctx, segs, n_segs, q, s, 1, nullptr, &kinds, &flat)) return rc;
  HostPlan hp;   // the planner is the predicate for the clauses, as in nrtgpu_query_supported
  return final_score_plan(ctx, segs, nullptr, n_segs, flat.queries.data(), 1, "sorted", hp);
}

extern "C" int nrtgpu_search_sorted_batch(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                          const nrtgpu_bm25_query* queries, const nrtgpu_field_sort* sorts, int32_t n_queries,
                                          nrtgpu_fielddocs* out) {
  if (int rc = final_score_enter(ctx, segs, n_segs, !queries || !sorts || !out, &n_queries)) return rc;
  const double t0 = now_ms();
  SegReadLocks content(segs, n_segs);   // until this call's kernels have finished
  std::vector<DSortQuery> records;
  std::vector<int> kinds;
  FlatQueries flat;
  records.reserve((size_t)n_queries);
  if (int rc = check_call(ctx, segs, n_segs, queries, sorts, n_queries, &records, &kinds, &flat)) return rc;
  HostPlan hp;
  if (int rc = final_score_plan(ctx, segs, doc_bases, n_segs, flat.queries.data(), n_queries, "sorted", hp)) return rc;
  std::vector<DSortPart> sparts;
  std::vector<int32_t> field_ids((size_t)n_queries);
  for (int qi = 0; qi < n_queries; ++qi) field_ids[(size_t)qi] = sorts[qi].field_id;
  if (int rc = doc_values_parts(segs, n_segs, field_ids.data(), hp, "sorted", &sparts)) return rc;
  const PlanBytes extras[2] = {{records.data(), records.size() * sizeof(DSortQuery)}, {sparts.data(), sparts.size() * sizeof(DSortPart)}};
  nrtgpu_topdocs* pages = reinterpret_cast<nrtgpu_topdocs*>(out);   // (the layout is the same: the static_assert above)
  if (int rc = final_score_run(ctx, hp, queries, n_queries, pages, t0, extras, 2, [](hipStream_t st, const FinalScoreArgs& a, const void* const* d_extra) {
        launch_bm25_field_sort(st, a, (const DSortQuery*)d_extra[0], (const DSortPart*)d_extra[1]);
      }))
    return rc;
  field_sort_values(records, kinds, n_queries, out);
  return NRTGPU_OK;
}
