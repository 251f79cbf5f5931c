// docset.cpp -- doc-set requests (include/nrtgpu.h: nrtgpu_search_docset_sorted_batch, nrtgpu_count_docset_terms_batch): a sort by
// field or a terms count whose hit set is a doc set -- liveDocs, FILTER / MUST_NOT masks, numeric range clauses -- and no text
// clause.  The plan is the route's own (planner.cpp: docset_plan): parts without clauses over every tile of every leaf, the
// query's combined accept set with liveDocs in DPart.live_bits.  Beside it go the sorted / counting route's per-query record
// (fieldsort.cpp / termscount.cpp build them), one DRangeQuery per query, one DSortPart per part for the sort / count column and
// kMaxRanges per part for the range clauses' columns (plan.h).  From the plan on the path is finalscore.cpp's; the count route's
// workspace, collect() and unpacking are termscount.cpp's (over a 64-bit count column, nrtgpu_count_docset_terms64_batch:
// termscount64.cpp's).
#include <cstddef>
#include <type_traits>

#include "runtime_internal.h"

static_assert(sizeof(nrtgpu_range_clause) == 16, "nrtgpu_range_clause layout");
static_assert(sizeof(nrtgpu_docset_query) == 56 && offsetof(nrtgpu_docset_query, more_filters) == 16 && offsetof(nrtgpu_docset_query, n_ranges) == 32 &&
                  offsetof(nrtgpu_docset_query, ranges) == 40 && offsetof(nrtgpu_docset_query, total_hits_threshold) == 48,
              "nrtgpu_docset_query layout");
static_assert(NRTGPU_MAX_RANGES == kMaxRanges, "NRTGPU_MAX_RANGES");

extern "C" int nrtgpu_range_accepts(int32_t kind, uint32_t lower_bits, uint32_t upper_bits, uint32_t value_bits, int32_t* out) {
  if (!out) return fail(NRTGPU_ERR_INVALID_ARG, "NULL argument");
  if (kind != NRTGPU_DOCVALUES_INT32 && kind != NRTGPU_DOCVALUES_FLOAT32) return fail(NRTGPU_ERR_INVALID_ARG, "doc values kind %d outside 0..1", kind);
  *out = range_accepts_code(doc_value_code(kind, lower_bits), doc_value_code(kind, upper_bits), doc_value_code(kind, value_bits)) ? 1 : 0;
  return NRTGPU_OK;
}

namespace {

// What is checked and built of the doc sets of a call, whichever collector they run under.
struct DocsetCall {
  std::vector<nrtgpu_bm25_query> masks;    // per query: k, total_hits_threshold and the mask fields (what docset_plan and final_score_run read)
  std::vector<DRangeQuery> ranges;         // per query (the codes are filled once the columns' kinds are known)
  std::vector<int> range_kinds;            // per (query, clause): kMaxRanges per query
  bool any_multi = false;                  // some named column of the call (a range clause's, the 32-bit count's) is multi-valued: the launches' `multi`
};

// What the route refuses of docsets[qi] as an invalid argument, the header's table in its order.
int check_docset(const nrtgpu_docset_query& d, int qi) {
  if (d.k < 1 || d.k > NRTGPU_MAX_K) return fail(NRTGPU_ERR_INVALID_ARG, "query %d: numHits %d outside 1..%d", qi, d.k, NRTGPU_MAX_K);
  if (d.total_hits_threshold < 0) return fail(NRTGPU_ERR_INVALID_ARG, "query %d: totalHitsThreshold must be >= 0, got %d", qi, d.total_hits_threshold);
  if (d.n_ranges < 0 || d.n_ranges > NRTGPU_MAX_RANGES) return fail(NRTGPU_ERR_INVALID_ARG, "query %d: n_ranges %d outside 0..%d", qi, d.n_ranges, NRTGPU_MAX_RANGES);
  if (d.n_ranges > 0 && !d.ranges) return fail(NRTGPU_ERR_INVALID_ARG, "query %d: ranges is NULL with n_ranges %d", qi, d.n_ranges);
  for (int r = 0; r < d.n_ranges; ++r)
    if (d.ranges[r].reserved != 0) return fail(NRTGPU_ERR_INVALID_ARG, "query %d: range clause %d: reserved must be 0", qi, r);
  if (d.filter_mask < 0 || d.must_not_mask < 0) return fail(NRTGPU_ERR_INVALID_ARG, "query %d: mask ids must be >= 0", qi);
  if (d.n_more_filters < 0 || d.n_more_must_not < 0 || (d.n_more_filters > 0 && !d.more_filters) || (d.n_more_must_not > 0 && !d.more_must_not))
    return fail(NRTGPU_ERR_INVALID_ARG, "query %d: more_filters / more_must_not", qi);
  if (d.n_more_filters + (d.filter_mask != 0) > NRTGPU_MAX_MASKS || d.n_more_must_not + (d.must_not_mask != 0) > NRTGPU_MAX_MASKS)
    return fail(NRTGPU_ERR_INVALID_ARG, "query %d: more than %d FILTER or MUST_NOT clauses", qi, NRTGPU_MAX_MASKS);
  for (int i = 0; i < d.n_more_filters; ++i)
    if (d.more_filters[i] <= 0) return fail(NRTGPU_ERR_INVALID_ARG, "query %d: more_filters[%d] must be a mask id > 0", qi, i);
  for (int i = 0; i < d.n_more_must_not; ++i)
    if (d.more_must_not[i] <= 0) return fail(NRTGPU_ERR_INVALID_ARG, "query %d: more_must_not[%d] must be a mask id > 0", qi, i);
  if (d.reserved != 0) return fail(NRTGPU_ERR_INVALID_ARG, "query %d: reserved must be 0", qi);
  return NRTGPU_OK;
}

// The invalid-argument half of one doc set: check_docset, then the kinds of its range clauses' columns over the leaves (leaves
// that disagree are refused here); its records begun.
int docset_begin(const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_docset_query& d, int qi, DocsetCall* call) {
  if (int rc = check_docset(d, qi)) return rc;
  nrtgpu_bm25_query m{};
  m.k = d.k;
  m.total_hits_threshold = d.total_hits_threshold;
  m.filter_mask = d.filter_mask;
  m.must_not_mask = d.must_not_mask;
  m.n_more_filters = d.n_more_filters;
  m.more_filters = d.more_filters;
  m.n_more_must_not = d.n_more_must_not;
  m.more_must_not = d.more_must_not;
  call->masks.push_back(m);
  DRangeQuery rq{};
  rq.n_ranges = (uint32_t)d.n_ranges;
  for (int r = 0; r < kMaxRanges; ++r) {
    int kind = -1;
    bool multi = false;
    if (r < d.n_ranges)
      if (int rc = doc_values_kind(segs, n_segs, d.ranges[r].field_id, qi, &kind, &multi)) return rc;
    call->range_kinds.push_back(kind);
    if (multi) {
      rq.multi |= 1u << r;
      call->any_multi = true;
    }
  }
  call->ranges.push_back(rq);
  return NRTGPU_OK;
}

// The unsupported half, behind the collector's own column: a range clause's column on no leaf, a mask that is not resident; the
// clauses' bounds as codes.
int docset_finish(const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_docset_query& d, int qi, DocsetCall* call) {
  DRangeQuery& rq = call->ranges[(size_t)qi];
  for (int r = 0; r < d.n_ranges; ++r) {
    const int kind = call->range_kinds[(size_t)qi * (size_t)kMaxRanges + (size_t)r];
    if (kind < 0) return fail(NRTGPU_ERR_UNSUPPORTED, "query %d: no leaf of the call holds doc values of field %d (range clause %d)", qi, d.ranges[r].field_id, r);
    if (kind >= kDocValuesInt64)
      return doc_values_wide(qi, d.ranges[r].field_id, "a range over it is a mask built by nrtgpu_segment_set_mask_from_values64, named as a filter");
    rq.lo_code[r] = doc_value_code(kind, d.ranges[r].lower_bits);
    rq.hi_code[r] = doc_value_code(kind, d.ranges[r].upper_bits);
  }
  return doc_values_masks_resident(segs, n_segs, call->masks[(size_t)qi], qi);
}

int no_column(int qi, int32_t field_id) { return fail(NRTGPU_ERR_UNSUPPORTED, "query %d: no leaf of the call holds doc values of field %d", qi, field_id); }

// ---- the driver: one checking half and one running half behind every (predicate, batch entry) pair -------------------------------
// The checking half, shared by a predicate and its batch entry, in the order the header's tables promise: per query docset_begin,
// then the collector's invalid-argument step; then, per query, the collector's column refusals (on no leaf, wide / narrow,
// multi-valued), docset_finish, and the collector's record.  begin / column / record: int(int qi).
template <class Begin, class Column, class Record>
int docset_check(const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_docset_query* docsets, int32_t n_queries, DocsetCall* call, Begin begin,
                 Column column, Record record) {
  for (int qi = 0; qi < n_queries; ++qi) {
    if (int rc = docset_begin(segs, n_segs, docsets[qi], qi, call)) return rc;
    if (int rc = begin(qi)) return rc;
  }
  for (int qi = 0; qi < n_queries; ++qi) {
    if (int rc = column(qi)) return rc;
    if (int rc = docset_finish(segs, n_segs, docsets[qi], qi, call)) return rc;
    if (int rc = record(qi)) return rc;
  }
  return NRTGPU_OK;
}

// A predicate: the checking half, then the planner for the leaves (sealed, of this context) and the accept sets, with n = 1.
// check: int(DocsetCall*).
template <class Check>
int docset_supported(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs, bool null_argument, Check check) {
  if (int rc = final_score_enter(ctx, segs, n_segs, null_argument, nullptr)) return rc;
  SegReadLocks content(segs, n_segs);
  DocsetCall call;
  if (int rc = check(&call)) return rc;
  HostPlan hp;
  return docset_plan(ctx, segs, nullptr, n_segs, call.masks.data(), 1, hp);
}

// The running half of a batch entry, from the checked call to the filled pages: the plan, the columns of every part's leaf
// (HostPlan.part_leaf) -- the collector's (field_of: int32_t(uint32_t query); wide: it holds 64-bit codes) and the range
// clauses', which are 32-bit ones --, the four extras, the launch for the call's arities, final_score_run.  records: the
// collector's per-query records (extras[0]); launch[m]: its scorer, m = the call names a multi-valued column.
template <class FieldOf>
int docset_run(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs, const nrtgpu_docset_query* docsets,
               int32_t n_queries, const DocsetCall& call, double t0, PlanBytes records, FieldOf field_of, bool wide, const FinalScoreLaunch (&launch)[2],
               nrtgpu_topdocs* pages, const FinalScoreOwn* own) {
  HostPlan hp;
  if (int rc = docset_plan(ctx, segs, doc_bases, n_segs, call.masks.data(), n_queries, hp)) return rc;
  std::vector<DSortPart> sparts(hp.parts.size(), DSortPart{nullptr, nullptr}), rparts(hp.parts.size() * (size_t)kMaxRanges, DSortPart{nullptr, nullptr});
  for (const DItem& it : hp.items)
    for (uint32_t pi = 0; pi < it.n_parts; ++pi) {
      const size_t at = (size_t)it.part_begin + pi;
      const nrtgpu_seg* seg = segs[hp.part_leaf[at]];
      sparts[at] = range_count_column_of(seg, field_of(it.query), wide);   // (rangecount.cpp: despite its name the column of ANY collector at either width)
      const nrtgpu_docset_query& d = docsets[it.query];
      for (int r = 0; r < d.n_ranges; ++r) rparts[at * (size_t)kMaxRanges + (size_t)r] = doc_values_column(seg, d.ranges[r].field_id);
    }
  const PlanBytes extras[4] = {records,
                               {call.ranges.data(), call.ranges.size() * sizeof(DRangeQuery)},
                               {sparts.data(), sparts.size() * sizeof(DSortPart)},
                               {rparts.data(), rparts.size() * sizeof(DSortPart)}};
  return final_score_run(ctx, hp, call.masks.data(), n_queries, pages, t0, extras, 4, launch[call.any_multi ? 1 : 0], own);
}

// What the counting entries hand final_score_run for pages: no hits come back (the merge's lists are empty; total_hits is read from them).
std::vector<nrtgpu_topdocs> no_pages(int32_t n_queries) { return std::vector<nrtgpu_topdocs>((size_t)n_queries, nrtgpu_topdocs{}); }

// ---- the collectors: what each checks, and its scorer (d_extra: docset_run's extras) -----------------------------------------------
// A sort by a 32-bit column (fieldsort.cpp's records).
int check_sorted(const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_docset_query* docsets, const nrtgpu_field_sort* sorts, int32_t n_queries,
                 DocsetCall* call, std::vector<DSortQuery>* records, std::vector<int>* kinds) {
  std::vector<char> sort_multi;
  return docset_check(
      segs, n_segs, docsets, n_queries, call,
      [&](int qi) {
        if (int rc = field_sort_check(sorts[qi], qi)) return rc;
        int kind = -1;
        bool multi = false;
        if (int rc = doc_values_kind(segs, n_segs, sorts[qi].field_id, qi, &kind, &multi)) return rc;
        kinds->push_back(kind);
        sort_multi.push_back(multi ? 1 : 0);
        return (int)NRTGPU_OK;
      },
      [&](int qi) {
        const int kind = (*kinds)[(size_t)qi];
        if (kind < 0) return no_column(qi, sorts[qi].field_id);
        if (kind >= kDocValuesInt64) return doc_values_wide(qi, sorts[qi].field_id, "sort by it with nrtgpu_search_docset_sorted64_batch");
        if (sort_multi[(size_t)qi] != 0) return field_sort_multi(qi, sorts[qi].field_id);
        return (int)NRTGPU_OK;
      },
      [&](int qi) {
        DSortQuery r{};
        field_sort_record(sorts[qi], (*kinds)[(size_t)qi], &r);
        records->push_back(r);
        return (int)NRTGPU_OK;
      });
}
template <bool MULTI>
void launch_sorted(hipStream_t st, const FinalScoreArgs& a, const void* const* d_extra) {
  launch_docset_sort(st, MULTI, a, (const DSortQuery*)d_extra[0], (const DRangeQuery*)d_extra[1], (const DSortPart*)d_extra[2], (const DSortPart*)d_extra[3]);
}

// A sort by a 64-bit column (fieldsort64.cpp's records; in_order: the predicate's doc bases).
int check_sorted64(const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs, bool in_order, const nrtgpu_docset_query* docsets,
                   const nrtgpu_field_sort64* sorts, int32_t n_queries, DocsetCall* call, std::vector<DSort64Query>* records, std::vector<int>* kinds) {
  std::vector<char> sort_multi;
  uint32_t db = 1;
  return docset_check(
      segs, n_segs, docsets, n_queries, call,
      [&](int qi) {
        if (int rc = field_sort_check(sorts[qi], qi)) return rc;
        int kind = -1;
        bool multi = false;
        if (int rc = doc_values_kind(segs, n_segs, sorts[qi].field_id, qi, &kind, &multi)) return rc;
        kinds->push_back(kind);
        sort_multi.push_back(multi ? 1 : 0);
        return (int)NRTGPU_OK;
      },
      [&](int qi) {
        const int kind = (*kinds)[(size_t)qi];
        if (kind < 0) return no_column(qi, sorts[qi].field_id);
        if (kind < kDocValuesInt64) return field_sort64_narrow(qi, sorts[qi].field_id, sort_multi[(size_t)qi] != 0, "nrtgpu_search_docset_sorted_batch");
        return (int)NRTGPU_OK;
      },
      [&](int qi) {
        if (qi == 0)
          if (int rc = sort64_doc_bits(segs, doc_bases, n_segs, in_order, &db)) return rc;
        DSort64Query r{};
        if (int rc = field_sort64_record(segs, n_segs, sorts[qi], (*kinds)[(size_t)qi], db, qi, &r)) return rc;
        records->push_back(r);
        return (int)NRTGPU_OK;
      });
}
template <bool MULTI>
void launch_sorted64(hipStream_t st, const FinalScoreArgs& a, const void* const* d_extra) {
  launch_docset_sort64(st, MULTI, a, (const DSort64Query*)d_extra[0], (const DRangeQuery*)d_extra[1], (const DSort64Part*)d_extra[2],
                       (const DSortPart*)d_extra[3]);
}

// A terms count over a 32-bit column (termscount.cpp's records and workspace) or, WORK = TermsWork64, over a 64-bit one
// (termscount64.cpp's).  out: the batch entry's outputs (their capacities), nullptr for the predicate.
template <class WORK, class OUT>
int check_terms(const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_docset_query* docsets, const nrtgpu_terms_count* terms, const OUT* out,
                int32_t n_queries, DocsetCall* call, std::vector<DTermsQuery>* records, std::vector<int>* kinds, WORK* work) {
  constexpr bool wide = std::is_same<WORK, TermsWork64>::value;
  std::vector<char> count_multi;
  uint64_t slots = 0, cap = 0;
  if (int rc = docset_check(
          segs, n_segs, docsets, n_queries, call,
          [&](int qi) {
            int kind = -1;
            bool multi = false;
            DTermsQuery r{};
            if constexpr (wide) {
              if (int rc = terms_count64_record(segs, n_segs, terms[qi], out ? &out[qi] : nullptr, qi, &slots, &cap, &r, &kind, &multi)) return rc;
              r.need = 0u;   // (unread by the doc-set kernel; no multi-valued 64-bit column exists)
            } else {
              if (int rc = terms_count_record(segs, n_segs, terms[qi], out ? &out[qi] : nullptr, qi, &slots, &cap, &r, &kind, &multi)) return rc;
              call->any_multi = call->any_multi || multi;
            }
            kinds->push_back(kind);
            count_multi.push_back(multi ? 1 : 0);
            records->push_back(r);
            return (int)NRTGPU_OK;
          },
          [&](int qi) {
            const int kind = (*kinds)[(size_t)qi];
            if (kind < 0) return no_column(qi, terms[qi].field_id);
            if (wide && kind < kDocValuesInt64)
              return terms_count64_narrow(qi, terms[qi].field_id, count_multi[(size_t)qi] != 0, "nrtgpu_count_docset_terms_batch");
            if (!wide && kind >= kDocValuesInt64) return doc_values_wide(qi, terms[qi].field_id, kTermsCountWide);
            return (int)NRTGPU_OK;
          },
          [](int) { return (int)NRTGPU_OK; }))
    return rc;
  work->layout(n_queries, slots, cap);
  return NRTGPU_OK;
}
template <bool MULTI>
void launch_terms(hipStream_t st, const FinalScoreArgs& a, const void* const* d_extra) {
  const TermsWork* w = (const TermsWork*)a.own_user;
  char* d_own = (char*)a.own;
  launch_docset_terms_count(st, MULTI, a, (const DTermsQuery*)d_extra[0], (const DRangeQuery*)d_extra[1], (const DSortPart*)d_extra[2],
                            (const DSortPart*)d_extra[3], (DTermsState*)(d_own + w->o_states), (unsigned long long*)(d_own + w->o_tables),
                            (unsigned long long*)(d_own + w->o_out), (uint32_t)w->n_queries, w->out_cap);
}
template <bool MULTI>
void launch_terms64(hipStream_t st, const FinalScoreArgs& a, const void* const* d_extra) {
  const TermsWork64* w = (const TermsWork64*)a.own_user;
  DTermsState64* states;
  unsigned long long *keys, *out_codes;
  uint32_t *counts, *out_counts;
  terms64_regions(*w, (char*)a.own, &states, &keys, &counts, &out_codes, &out_counts);
  launch_docset_terms_count64(st, MULTI, a, (const DTermsQuery*)d_extra[0], (const DRangeQuery*)d_extra[1], (const DSort64Part*)d_extra[2],
                              (const DSortPart*)d_extra[3], states, keys, counts, out_codes, out_counts, (uint32_t)w->n_queries, w->out_cap);
}

// A numeric range facet (rangecount.cpp's records).  out: the batch entry's outputs, nullptr for the predicate.
int check_ranges(const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_docset_query* docsets, const nrtgpu_range_count* ranges,
                 const nrtgpu_range_counts* out, int32_t n_queries, DocsetCall* call, RangeWork* work) {
  if (int rc = docset_check(
          segs, n_segs, docsets, n_queries, call, [&](int qi) { return range_count_begin(segs, n_segs, ranges[qi], out ? &out[qi] : nullptr, qi, work); },
          [&](int qi) {
            if (work->kinds[(size_t)qi] < 0) return no_column(qi, ranges[qi].field_id);
            return range_count_column(*work, ranges, qi);
          },
          [](int) { return (int)NRTGPU_OK; }))
    return rc;
  work->layout(ranges, n_queries);
  work->seal();
  return NRTGPU_OK;
}
template <bool MULTI>
void launch_ranges(hipStream_t st, const FinalScoreArgs& a, const void* const* d_extra) {
  const RangeWork* w = (const RangeWork*)a.own_user;
  const char* d_plan = (const char*)d_extra[0];
  launch_docset_range_count(st, w->wide, MULTI, a, (const DRangeCountQuery*)d_plan, (const DRangeQuery*)d_extra[1], (const DSortPart*)d_extra[2],
                            (const DSortPart*)d_extra[3], d_plan + (size_t)w->n_queries * sizeof(DRangeCountQuery), (uint32_t*)a.own);
}

}  // namespace

extern "C" int nrtgpu_docset_sorted_supported(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_docset_query* d,
                                              const nrtgpu_field_sort* s) {
  return docset_supported(ctx, segs, n_segs, !d || !s, [&](DocsetCall* call) {
    std::vector<DSortQuery> records;
    std::vector<int> kinds;
    return check_sorted(segs, n_segs, d, s, 1, call, &records, &kinds);
  });
}

extern "C" int nrtgpu_search_docset_sorted_batch(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                                 const nrtgpu_docset_query* docsets, const nrtgpu_field_sort* sorts, int32_t n_queries,
                                                 nrtgpu_fielddocs* out) {
  if (int rc = final_score_enter(ctx, segs, n_segs, !docsets || !sorts || !out, &n_queries)) return rc;
  const double t0 = now_ms();
  SegReadLocks content(segs, n_segs);   // until this call's kernels have finished
  DocsetCall call;
  std::vector<DSortQuery> records;
  std::vector<int> kinds;
  if (int rc = check_sorted(segs, n_segs, docsets, sorts, n_queries, &call, &records, &kinds)) return rc;
  nrtgpu_topdocs* pages = reinterpret_cast<nrtgpu_topdocs*>(out);   // (the layout is the same: fieldsort.cpp's static_assert)
  if (int rc = docset_run(ctx, segs, doc_bases, n_segs, docsets, n_queries, call, t0, {records.data(), records.size() * sizeof(DSortQuery)},
                          [&](uint32_t q) { return sorts[q].field_id; }, false, {launch_sorted<false>, launch_sorted<true>}, pages, nullptr))
    return rc;
  field_sort_values(records, kinds, n_queries, out);
  return NRTGPU_OK;
}

extern "C" int nrtgpu_docset_sorted64_supported(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_docset_query* d,
                                                const nrtgpu_field_sort64* s) {
  return docset_supported(ctx, segs, n_segs, !d || !s, [&](DocsetCall* call) {
    std::vector<DSort64Query> records;
    std::vector<int> kinds;
    return check_sorted64(segs, nullptr, n_segs, true, d, s, 1, call, &records, &kinds);
  });
}

extern "C" int nrtgpu_search_docset_sorted64_batch(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                                   const nrtgpu_docset_query* docsets, const nrtgpu_field_sort64* sorts, int32_t n_queries,
                                                   nrtgpu_fielddocs64* out) {
  if (int rc = final_score_enter(ctx, segs, n_segs, !docsets || !sorts || !out, &n_queries)) return rc;
  const double t0 = now_ms();
  SegReadLocks content(segs, n_segs);   // until this call's kernels have finished
  DocsetCall call;
  std::vector<DSort64Query> records;
  std::vector<int> kinds;
  if (int rc = check_sorted64(segs, doc_bases, n_segs, false, docsets, sorts, n_queries, &call, &records, &kinds)) return rc;
  std::vector<int32_t> ks((size_t)n_queries);
  for (int qi = 0; qi < n_queries; ++qi) ks[(size_t)qi] = docsets[qi].k;
  Sort64Pages pages(ks.data(), out, n_queries);
  if (int rc = docset_run(ctx, segs, doc_bases, n_segs, docsets, n_queries, call, t0, {records.data(), records.size() * sizeof(DSort64Query)},
                          [&](uint32_t q) { return sorts[q].field_id; }, true, {launch_sorted64<false>, launch_sorted64<true>}, pages.pages.data(), nullptr))
    return rc;
  pages.decode(records, kinds, out);
  return NRTGPU_OK;
}

extern "C" int nrtgpu_count_docset_terms_supported(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_docset_query* d,
                                                   const nrtgpu_terms_count* t) {
  return docset_supported(ctx, segs, n_segs, !d || !t, [&](DocsetCall* call) {
    std::vector<DTermsQuery> records;
    std::vector<int> kinds;
    TermsWork work;
    return check_terms(segs, n_segs, d, t, (const nrtgpu_term_counts*)nullptr, 1, call, &records, &kinds, &work);
  });
}

extern "C" int nrtgpu_count_docset_terms_batch(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                               const nrtgpu_docset_query* docsets, const nrtgpu_terms_count* terms, int32_t n_queries,
                                               nrtgpu_term_counts* out) {
  if (int rc = final_score_enter(ctx, segs, n_segs, !docsets || !terms || !out, &n_queries)) return rc;
  const double t0 = now_ms();
  SegReadLocks content(segs, n_segs);   // until this call's kernels have finished
  DocsetCall call;
  std::vector<DTermsQuery> records;
  std::vector<int> kinds;
  TermsWork work;
  if (int rc = check_terms(segs, n_segs, docsets, terms, (const nrtgpu_term_counts*)out, n_queries, &call, &records, &kinds, &work)) return rc;
  std::vector<nrtgpu_topdocs> pages = no_pages(n_queries);
  const FinalScoreOwn own{work.bytes, terms_collect, &work};
  if (int rc = docset_run(ctx, segs, doc_bases, n_segs, docsets, n_queries, call, t0, {records.data(), records.size() * sizeof(DTermsQuery)},
                          [&](uint32_t q) { return terms[q].field_id; }, false, {launch_terms<false>, launch_terms<true>}, pages.data(), &own))
    return rc;
  return terms_unpack(work, kinds, pages.data(), n_queries, out);
}

extern "C" int nrtgpu_count_docset_terms64_supported(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_docset_query* d,
                                                     const nrtgpu_terms_count* t) {
  return docset_supported(ctx, segs, n_segs, !d || !t, [&](DocsetCall* call) {
    std::vector<DTermsQuery> records;
    std::vector<int> kinds;
    TermsWork64 work;
    return check_terms(segs, n_segs, d, t, (const nrtgpu_term_counts64*)nullptr, 1, call, &records, &kinds, &work);
  });
}

extern "C" int nrtgpu_count_docset_terms64_batch(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                                 const nrtgpu_docset_query* docsets, const nrtgpu_terms_count* terms, int32_t n_queries,
                                                 nrtgpu_term_counts64* out) {
  if (int rc = final_score_enter(ctx, segs, n_segs, !docsets || !terms || !out, &n_queries)) return rc;
  const double t0 = now_ms();
  SegReadLocks content(segs, n_segs);   // until this call's kernels have finished
  DocsetCall call;
  std::vector<DTermsQuery> records;
  std::vector<int> kinds;
  TermsWork64 work;
  if (int rc = check_terms(segs, n_segs, docsets, terms, (const nrtgpu_term_counts64*)out, n_queries, &call, &records, &kinds, &work)) return rc;
  std::vector<nrtgpu_topdocs> pages = no_pages(n_queries);
  const FinalScoreOwn own{work.bytes, terms64_collect, &work};
  if (int rc = docset_run(ctx, segs, doc_bases, n_segs, docsets, n_queries, call, t0, {records.data(), records.size() * sizeof(DTermsQuery)},
                          [&](uint32_t q) { return terms[q].field_id; }, true, {launch_terms64<false>, launch_terms64<true>}, pages.data(), &own))
    return rc;
  return terms64_unpack(work, kinds, pages.data(), n_queries, out);
}

extern "C" int nrtgpu_count_docset_ranges_supported(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_docset_query* d,
                                                    const nrtgpu_range_count* r) {
  return docset_supported(ctx, segs, n_segs, !d || !r, [&](DocsetCall* call) {
    RangeWork work;
    return check_ranges(segs, n_segs, d, r, nullptr, 1, call, &work);
  });
}

extern "C" int nrtgpu_count_docset_ranges_batch(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                                const nrtgpu_docset_query* docsets, const nrtgpu_range_count* ranges, int32_t n_queries,
                                                nrtgpu_range_counts* out) {
  if (int rc = final_score_enter(ctx, segs, n_segs, !docsets || !ranges || !out, &n_queries)) return rc;
  const double t0 = now_ms();
  SegReadLocks content(segs, n_segs);   // until this call's kernels have finished
  DocsetCall call;
  RangeWork work;
  if (int rc = check_ranges(segs, n_segs, docsets, ranges, out, n_queries, &call, &work)) return rc;
  std::vector<nrtgpu_topdocs> pages = no_pages(n_queries);
  const FinalScoreOwn own{work.bytes, range_collect, &work};
  if (int rc = docset_run(ctx, segs, doc_bases, n_segs, docsets, n_queries, call, t0, {work.plan_bytes.data(), work.plan_bytes.size()},
                          [&](uint32_t q) { return ranges[q].field_id; }, work.wide, {launch_ranges<false>, launch_ranges<true>}, pages.data(), &own))
    return rc;
  return range_unpack(work, ranges, pages.data(), n_queries, out);
}
