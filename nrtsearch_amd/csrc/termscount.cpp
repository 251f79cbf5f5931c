// termscount.cpp -- the terms aggregation (include/nrtgpu.h: nrtgpu_count_terms_batch): a text query's hits counted per distinct
// value of an int or float doc value column of the segment store.  The queries are planned as the sorted route plans them
// (fieldsort.cpp: plain SHOULD disjunctions through final_score_plan; what is a hit is decided by the route's own record), and the
// path from the plan to total_hits is finalscore.cpp's: the items report no candidates, so the shared merge and relation kernels
// return empty lists and the exact counts.  What is the route's own: one DTermsQuery per query and one DSortPart per part beside
// the plan, and in the workspace (FinalScoreOwn: zeroed per call) the queries' DTermsState records, their count tables and the
// call's compacted entries, which collect() copies back -- the states first, then only the entries that exist.  The entries of
// a query are sorted by code here (ascending code = ascending in the kind's order) and decoded with doc_value_bits.
#include <algorithm>
#include <cstddef>

#include "runtime_internal.h"

static_assert(sizeof(nrtgpu_terms_count) == 8, "nrtgpu_terms_count layout");
static_assert(sizeof(nrtgpu_term_counts) == 48 && offsetof(nrtgpu_term_counts, value_bits) == 8 && offsetof(nrtgpu_term_counts, counts) == 16 &&
                  offsetof(nrtgpu_term_counts, total_hits) == 24 && offsetof(nrtgpu_term_counts, hits_with_value) == 32 &&
                  offsetof(nrtgpu_term_counts, overflowed) == 40,
              "nrtgpu_term_counts layout");
static_assert(NRTGPU_MAX_TERM_BUCKETS == kTermsMaxBuckets, "NRTGPU_MAX_TERM_BUCKETS");

namespace nrtgpu {
namespace rt {

// ---- what the routes that fill count tables share (this file: a text query's hits; docset.cpp: a doc set) -----------------------
void TermsWork::layout(int32_t n, uint64_t slots, uint64_t cap) {
  Carver c;
  n_queries = n;
  o_states = c.take(((size_t)n + 1) * sizeof(DTermsState));
  o_tables = c.take((size_t)slots * 8);
  o_out = c.take((size_t)cap * 8);
  bytes = c.off;
  out_cap = (uint32_t)cap;   // (<= 2^24: half the slots)
}

// What the routes refuse of (terms[qi], out[qi]) as an invalid argument, the kind of the column over the leaves, and the query's
// record with its table laid out behind the earlier queries' (*slots, *cap: the call's running sums).
int terms_count_record(const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_terms_count& t, const nrtgpu_term_counts* out, int qi, uint64_t* slots,
                       uint64_t* cap, DTermsQuery* record, int* kind, bool* multi, uint64_t max_call_slots) {
  if (t.max_buckets < 1 || t.max_buckets > NRTGPU_MAX_TERM_BUCKETS)
    return fail(NRTGPU_ERR_INVALID_ARG, "query %d: max_buckets %d outside 1..%d", qi, t.max_buckets, NRTGPU_MAX_TERM_BUCKETS);
  if (out && (out->capacity < t.max_buckets || !out->value_bits || !out->counts))
    return fail(NRTGPU_ERR_INVALID_ARG, "query %d: an output of capacity %d (or NULL arrays) for max_buckets %d", qi, out->capacity, t.max_buckets);
  if (int rc = doc_values_kind(segs, n_segs, t.field_id, qi, kind, multi)) return rc;
  DTermsQuery r{};
  r.need = *multi ? kTermsQueryMulti : 0u;
  r.max_buckets = (uint32_t)t.max_buckets;
  r.table_shift = terms_table_shift(r.max_buckets);
  r.table_off = (uint32_t)*slots;
  *slots += 1ull << (32u - r.table_shift);
  *cap += r.max_buckets;
  if (*slots > max_call_slots)
    return fail(NRTGPU_ERR_INVALID_ARG, "query %d: the count tables of the call exceed the workspace bound of %llu slots (a query takes the power of two >= 2 x max_buckets)",
                qi, (unsigned long long)max_call_slots);
  *record = r;
  return NRTGPU_OK;
}

// Behind the wait: the states, then the entries that exist.
int terms_collect(nrtgpu_ctx* ctx, Slot* slot, const char* d_own, void* user) {
  TermsWork* w = (TermsWork*)user;
  const bool blocking = (ctx->cfg.flags & NRTGPU_FLAG_BLOCKING_WAIT) != 0;
  w->states.resize((size_t)w->n_queries + 1);
  HIP_TRY(hipMemcpyAsync(w->states.data(), d_own + w->o_states, w->states.size() * sizeof(DTermsState), hipMemcpyDeviceToHost, slot->stream));
  HIP_TRY(wait_for_stream(blocking, slot->stream, slot->ev_wait));
  const uint32_t n = std::min(w->states[(size_t)w->n_queries].claimed, w->out_cap);
  w->entries.resize(n);
  if (n != 0) {
    HIP_TRY(hipMemcpyAsync(w->entries.data(), d_own + w->o_out, (size_t)n * 8, hipMemcpyDeviceToHost, slot->stream));
    HIP_TRY(wait_for_stream(blocking, slot->stream, slot->ev_wait));
  }
  return NRTGPU_OK;
}


// The call's answers from what terms_collect brought back: a query's entries sorted by code (ascending code = ascending in the
// kind's order) and decoded with doc_value_bits.  pages: the merge's lists (empty; total_hits is read from them).
int terms_unpack(const TermsWork& work, const std::vector<int>& kinds, const nrtgpu_topdocs* pages, int32_t n_queries, nrtgpu_term_counts* out) {
  std::vector<uint64_t> mine;
  for (int qi = 0; qi < n_queries; ++qi) {
    nrtgpu_term_counts& o = out[qi];
    const DTermsState& st = work.states[(size_t)qi];
    o.total_hits = pages[(size_t)qi].total_hits;
    o.reserved = 0;
    o.overflowed = st.overflow != 0u ? 1 : 0;
    o.n_buckets = 0;
    o.hits_with_value = o.overflowed ? -1 : 0;
    if (o.overflowed) continue;
    const size_t b = st.out_base, n = st.n_out;
    if (b + n > work.entries.size() || (int64_t)n > (int64_t)o.capacity) return fail(NRTGPU_ERR_STATE, "terms count: query %d came back with %zu buckets at %zu", qi, n, b);
    mine.assign(work.entries.begin() + (ptrdiff_t)b, work.entries.begin() + (ptrdiff_t)(b + n));
    std::sort(mine.begin(), mine.end(), [](uint64_t x, uint64_t y) { return (uint32_t)x < (uint32_t)y; });   // codes are distinct
    for (size_t i = 0; i < n; ++i) {
      o.value_bits[i] = doc_value_bits(kinds[(size_t)qi], (uint32_t)mine[i]);
      o.counts[i] = (int32_t)(mine[i] >> 32);
      o.hits_with_value += o.counts[i];
    }
    o.n_buckets = (int32_t)n;
  }
  return NRTGPU_OK;
}

}  // namespace rt
}  // namespace nrtgpu

namespace {

// What the route refuses of a call before anything is planned (the segments' content is held); the records and the copies that
// are planned on the way.  out: the batch entry's outputs (their capacities), nullptr for the predicate.  *any_multi: some query
// counts a multi-valued column (the call launches bm25_terms_count_multi_kernel).
int check_call(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_bm25_query* queries, const nrtgpu_terms_count* terms,
               const nrtgpu_term_counts* out, int32_t n_queries, std::vector<DTermsQuery>* records, std::vector<int>* kinds, FlatQueries* flat,
               TermsWork* work, bool* any_multi) {
  *any_multi = false;
  flat->queries.reserve((size_t)n_queries);
  flat->terms.reserve((size_t)n_queries);
  records->reserve((size_t)n_queries);
  uint64_t slots = 0, cap = 0;
  for (int qi = 0; qi < n_queries; ++qi) {
    const nrtgpu_bm25_query& q = queries[qi];
    const nrtgpu_terms_count& t = terms[qi];
    if (int rc = validate_query(q, qi)) return rc;
    int kind = -1;
    bool multi = false;
    DTermsQuery r{};
    if (int rc = terms_count_record(segs, n_segs, t, out ? &out[qi] : nullptr, qi, &slots, &cap, &r, &kind, &multi)) return rc;
    kinds->push_back(kind);
    records->push_back(r);
    *any_multi = *any_multi || multi;
  }
  if (int rc = final_score_check_flags(ctx, "terms count")) return rc;
  for (int qi = 0; qi < n_queries; ++qi) {
    DTermsQuery& r = (*records)[(size_t)qi];
    uint32_t need = 0;
    if ((*kinds)[(size_t)qi] >= kDocValuesInt64) return doc_values_wide(qi, terms[qi].field_id, kTermsCountWide);
    if (int rc = doc_values_query(segs, n_segs, queries[qi], qi, (*kinds)[(size_t)qi], terms[qi].field_id, "a terms count", &need, flat)) return rc;
    r.need |= need;   // (beside kTermsQueryMulti)
  }
  for (int qi = 0; qi < n_queries; ++qi) flat->queries[(size_t)qi].terms = flat->terms[(size_t)qi].data();   // (the vectors have settled)
  work->layout(n_queries, slots, cap);
  return NRTGPU_OK;
}

}  // namespace

extern "C" int nrtgpu_count_terms_supported(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_bm25_query* q,
                                            const nrtgpu_terms_count* t) {
  if (int rc = final_score_enter(ctx, segs, n_segs, !q || !t, nullptr)) return rc;
  SegReadLocks content(segs, n_segs);
  std::vector<DTermsQuery> records;
  std::vector<int> kinds;
  FlatQueries flat;
  TermsWork work;
  bool any_multi = false;
  if (int rc = check_call(ctx, segs, n_segs, q, t, nullptr, 1, &records, &kinds, &flat, &work, &any_multi)) return rc;
  HostPlan hp;   // the planner is the predicate for the clauses, as in nrtgpu_query_supported
  return final_score_plan(ctx, segs, nullptr, n_segs, flat.queries.data(), 1, "terms count", hp);
}

extern "C" int nrtgpu_count_terms_batch(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                        const nrtgpu_bm25_query* queries, const nrtgpu_terms_count* terms, int32_t n_queries,
                                        nrtgpu_term_counts* out) {
  if (int rc = final_score_enter(ctx, segs, n_segs, !queries || !terms || !out, &n_queries)) return rc;
  const double t0 = now_ms();
  SegReadLocks content(segs, n_segs);   // until this call's kernels have finished
  std::vector<DTermsQuery> records;
  std::vector<int> kinds;
  FlatQueries flat;
  TermsWork work;
  bool any_multi = false;
  if (int rc = check_call(ctx, segs, n_segs, queries, terms, out, n_queries, &records, &kinds, &flat, &work, &any_multi)) return rc;
  HostPlan hp;
  if (int rc = final_score_plan(ctx, segs, doc_bases, n_segs, flat.queries.data(), n_queries, "terms count", hp)) return rc;
  std::vector<DSortPart> sparts;
  std::vector<int32_t> field_ids((size_t)n_queries);
  for (int qi = 0; qi < n_queries; ++qi) field_ids[(size_t)qi] = terms[qi].field_id;
  if (int rc = doc_values_parts(segs, n_segs, field_ids.data(), hp, "terms count", &sparts)) return rc;
  const PlanBytes extras[2] = {{records.data(), records.size() * sizeof(DTermsQuery)}, {sparts.data(), sparts.size() * sizeof(DSortPart)}};
  std::vector<nrtgpu_topdocs> pages((size_t)n_queries, nrtgpu_topdocs{});   // (no hits come back: the merge's lists are empty; total_hits is read from them)
  const FinalScoreOwn own{work.bytes, terms_collect, &work};
  // the dispatch: a call whose count columns are all single-valued launches what it always launched
  const FinalScoreLaunch single = [](hipStream_t st, const FinalScoreArgs& a, const void* const* d_extra) {
    const TermsWork* w = (const TermsWork*)a.own_user;
    char* d_own = (char*)a.own;
    launch_bm25_terms_count(st, a, (const DTermsQuery*)d_extra[0], (const DSortPart*)d_extra[1], (DTermsState*)(d_own + w->o_states),
                            (unsigned long long*)(d_own + w->o_tables), (unsigned long long*)(d_own + w->o_out), (uint32_t)w->n_queries, w->out_cap);
  };
  const FinalScoreLaunch multi = [](hipStream_t st, const FinalScoreArgs& a, const void* const* d_extra) {
    const TermsWork* w = (const TermsWork*)a.own_user;
    char* d_own = (char*)a.own;
    launch_bm25_terms_count_multi(st, a, (const DTermsQuery*)d_extra[0], (const DSortPart*)d_extra[1], (DTermsState*)(d_own + w->o_states),
                                  (unsigned long long*)(d_own + w->o_tables), (unsigned long long*)(d_own + w->o_out), (uint32_t)w->n_queries, w->out_cap);
  };
  if (int rc = final_score_run(ctx, hp, queries, n_queries, pages.data(), t0, extras, 2, any_multi ? multi : single, &own)) return rc;
  return terms_unpack(work, kinds, pages.data(), n_queries, out);
}
