// termscount64.cpp -- the terms aggregation over a 64-bit column (include/nrtgpu.h: nrtgpu_count_terms64_batch,
// nrtgpu_terms_home_slots64): a text query's hits counted per distinct value of a LONG / DATE_TIME / DOUBLE doc value column
// (segment.cpp: nrtgpu_segment_add_doc_values64).  The host path is termscount.cpp's -- terms_count_record's checks, the flat
// copies planned through final_score_plan, doc_values_part_leaves' walk, final_score_run with the route's own workspace -- with
// three things of its own: the workspace holds DTermsState64 records and the tables as a key array and a count array (plan.h),
// collect() brings back codes and counts as two lists, and a query's entries are decoded with doc_value_bits64.  What the doc-set
// form (docset.cpp) shares is declared in runtime_internal.h.
#include <algorithm>
#include <cstddef>
#include <numeric>

#include "runtime_internal.h"

static_assert(sizeof(nrtgpu_term_counts64) == 48 && offsetof(nrtgpu_term_counts64, value_bits) == 8 && offsetof(nrtgpu_term_counts64, counts) == 16 &&
                  offsetof(nrtgpu_term_counts64, total_hits) == 24 && offsetof(nrtgpu_term_counts64, hits_with_value) == 32 &&
                  offsetof(nrtgpu_term_counts64, overflowed) == 40,
              "nrtgpu_term_counts64 layout");
static_assert(sizeof(nrtgpu_term_counts64) == sizeof(nrtgpu_term_counts) && offsetof(nrtgpu_term_counts64, capacity) == offsetof(nrtgpu_term_counts, capacity) &&
                  offsetof(nrtgpu_term_counts64, value_bits) == offsetof(nrtgpu_term_counts, value_bits) &&
                  offsetof(nrtgpu_term_counts64, counts) == offsetof(nrtgpu_term_counts, counts),
              "terms_count_record reads an output of either width");
static_assert(NRTGPU_TERMS64_LDS_SLOTS == kTerms64LdsSlots, "NRTGPU_TERMS64_LDS_SLOTS");
static_assert(NRTGPU_TERMS64_MAX_CALL_SLOTS == kTerms64MaxCallSlots, "NRTGPU_TERMS64_MAX_CALL_SLOTS");

extern "C" int nrtgpu_terms_home_slots64(int32_t kind, uint64_t value_bits, int32_t max_buckets, uint32_t* lds_slot, uint32_t* table_slot) {
  if (!lds_slot || !table_slot) return fail(NRTGPU_ERR_INVALID_ARG, "NULL argument");
  if (kind != NRTGPU_DOCVALUES_INT64 && kind != NRTGPU_DOCVALUES_FLOAT64) return fail(NRTGPU_ERR_INVALID_ARG, "64-bit doc values kind %d outside 2..3", kind);
  if (max_buckets < 1 || max_buckets > NRTGPU_MAX_TERM_BUCKETS)
    return fail(NRTGPU_ERR_INVALID_ARG, "max_buckets %d outside 1..%d", max_buckets, NRTGPU_MAX_TERM_BUCKETS);
  const uint64_t code = doc_value_code64(kind, value_bits);
  const uint32_t shift = terms_table_shift((uint32_t)max_buckets);
  *lds_slot = terms_home_slot64(code, (uint32_t)kTerms64LdsShift);
  *table_slot = terms_home_slot64(code, shift) & ((1u << (32u - shift)) - 1u);
  return NRTGPU_OK;
}

namespace nrtgpu {
namespace rt {

// ---- what the routes that fill 64-bit count tables share (this file: a text query's hits; docset.cpp: a doc set) ----------------
void TermsWork64::layout(int32_t n, uint64_t slots, uint64_t cap) {
  Carver c;
  n_queries = n;
  o_states = c.take(((size_t)n + 1) * sizeof(DTermsState64));
  o_keys = c.take((size_t)slots * 8);
  o_counts = c.take((size_t)slots * 4);
  o_out_codes = c.take((size_t)cap * 8);
  o_out_counts = c.take((size_t)cap * 4);
  bytes = c.off;
  out_cap = (uint32_t)cap;
}

int terms_count64_record(const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_terms_count& t, const nrtgpu_term_counts64* out, int qi, uint64_t* slots,
                         uint64_t* cap, DTermsQuery* record, int* kind, bool* multi) {
  // (capacity and the arrays lie where they lie in nrtgpu_term_counts: the static_assert above)
  return terms_count_record(segs, n_segs, t, reinterpret_cast<const nrtgpu_term_counts*>(out), qi, slots, cap, record, kind, multi, kTerms64MaxCallSlots);
}

int terms_count64_narrow(int qi, int32_t field_id, bool multi, const char* entry32) {
  return fail(NRTGPU_ERR_UNSUPPORTED, "query %d: the doc values of field %d are a %s column: count it with %s", qi, field_id,
              multi ? "multi-valued 32-bit" : "32-bit", entry32);
}

// Behind the wait: the states, then the entries that exist.
int terms64_collect(nrtgpu_ctx* ctx, Slot* slot, const char* d_own, void* user) {
  TermsWork64* w = (TermsWork64*)user;
  const bool blocking = (ctx->cfg.flags & NRTGPU_FLAG_BLOCKING_WAIT) != 0;
  w->states.resize((size_t)w->n_queries + 1);
  HIP_TRY(hipMemcpyAsync(w->states.data(), d_own + w->o_states, w->states.size() * sizeof(DTermsState64), hipMemcpyDeviceToHost, slot->stream));
  HIP_TRY(wait_for_stream(blocking, slot->stream, slot->ev_wait));
  const uint32_t n = std::min(w->states[(size_t)w->n_queries].claimed, w->out_cap);
  w->codes.resize(n);
  w->counts.resize(n);
  if (n != 0) {
    HIP_TRY(hipMemcpyAsync(w->codes.data(), d_own + w->o_out_codes, (size_t)n * 8, hipMemcpyDeviceToHost, slot->stream));
    HIP_TRY(hipMemcpyAsync(w->counts.data(), d_own + w->o_out_counts, (size_t)n * 4, hipMemcpyDeviceToHost, slot->stream));
    HIP_TRY(wait_for_stream(blocking, slot->stream, slot->ev_wait));
  }
  return NRTGPU_OK;
}

// The call's answers from what terms64_collect brought back: a query's entries sorted by code (ascending code = ascending in the
// kind's order) and decoded with doc_value_bits64.  pages: the merge's lists (empty; total_hits is read from them).
int terms64_unpack(const TermsWork64& work, const std::vector<int>& kinds, const nrtgpu_topdocs* pages, int32_t n_queries, nrtgpu_term_counts64* out) {
  std::vector<uint32_t> order;
  for (int qi = 0; qi < n_queries; ++qi) {
    nrtgpu_term_counts64& o = out[qi];
    const DTermsState64& st = work.states[(size_t)qi];
    o.total_hits = pages[(size_t)qi].total_hits;
    o.reserved = 0;
    o.overflowed = st.overflow != 0u ? 1 : 0;
    o.n_buckets = 0;
    o.hits_with_value = o.overflowed ? -1 : 0;
    if (o.overflowed) continue;
    const size_t b = st.out_base, n = st.n_out;
    if (b + n > work.codes.size() || (int64_t)n > (int64_t)o.capacity) return fail(NRTGPU_ERR_STATE, "terms count: query %d came back with %zu buckets at %zu", qi, n, b);
    order.resize(n);
    std::iota(order.begin(), order.end(), (uint32_t)b);
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return work.codes[x] < work.codes[y]; });   // codes are distinct
    for (size_t i = 0; i < n; ++i) {
      o.value_bits[i] = doc_value_bits64(kinds[(size_t)qi], work.codes[order[i]]);
      o.counts[i] = (int32_t)work.counts[order[i]];
      o.hits_with_value += o.counts[i];
    }
    o.n_buckets = (int32_t)n;
  }
  return NRTGPU_OK;
}

// the route's scorer arguments out of the workspace (own: FinalScoreArgs.own)
void terms64_regions(const TermsWork64& w, char* d_own, DTermsState64** states, unsigned long long** keys, uint32_t** counts, unsigned long long** out_codes,
                     uint32_t** out_counts) {
  *states = (DTermsState64*)(d_own + w.o_states);
  *keys = (unsigned long long*)(d_own + w.o_keys);
  *counts = (uint32_t*)(d_own + w.o_counts);
  *out_codes = (unsigned long long*)(d_own + w.o_out_codes);
  *out_counts = (uint32_t*)(d_own + w.o_out_counts);
}

}  // namespace rt
}  // namespace nrtgpu

namespace {

// What the route refuses of a call before anything is planned (termscount.cpp: check_call, with the narrow column's refusal where
// that one refuses the wide one).  out: the batch entry's outputs (their capacities), nullptr for the predicate.
int check_call64(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_bm25_query* queries, const nrtgpu_terms_count* terms,
                 const nrtgpu_term_counts64* out, int32_t n_queries, std::vector<DTermsQuery>* records, std::vector<int>* kinds, FlatQueries* flat,
                 TermsWork64* work) {
  flat->queries.reserve((size_t)n_queries);
  flat->terms.reserve((size_t)n_queries);
  records->reserve((size_t)n_queries);
  std::vector<char> multis;
  uint64_t slots = 0, cap = 0;
  for (int qi = 0; qi < n_queries; ++qi) {
    if (int rc = validate_query(queries[qi], qi)) return rc;
    int kind = -1;
    bool multi = false;
    DTermsQuery r{};
    if (int rc = terms_count64_record(segs, n_segs, terms[qi], out ? &out[qi] : nullptr, qi, &slots, &cap, &r, &kind, &multi)) return rc;
    r.need = 0u;   // (no multi-valued 64-bit column exists: the word is the clause count alone)
    kinds->push_back(kind);
    multis.push_back(multi ? 1 : 0);
    records->push_back(r);
  }
  if (int rc = final_score_check_flags(ctx, "terms count")) return rc;
  for (int qi = 0; qi < n_queries; ++qi) {
    const int kind = (*kinds)[(size_t)qi];
    uint32_t need = 0;
    if (kind >= 0 && kind < kDocValuesInt64) return terms_count64_narrow(qi, terms[qi].field_id, multis[(size_t)qi] != 0, "nrtgpu_count_terms_batch");
    if (int rc = doc_values_query(segs, n_segs, queries[qi], qi, kind, terms[qi].field_id, "a terms count", &need, flat)) return rc;
    (*records)[(size_t)qi].need = need;
  }
  for (int qi = 0; qi < n_queries; ++qi) flat->queries[(size_t)qi].terms = flat->terms[(size_t)qi].data();   // (the vectors have settled)
  work->layout(n_queries, slots, cap);
  return NRTGPU_OK;
}

}  // namespace

extern "C" int nrtgpu_count_terms64_supported(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_bm25_query* q,
                                              const nrtgpu_terms_count* t) {
  if (int rc = final_score_enter(ctx, segs, n_segs, !q || !t, nullptr)) return rc;
  SegReadLocks content(segs, n_segs);
  std::vector<DTermsQuery> records;
  std::vector<int> kinds;
  FlatQueries flat;
  TermsWork64 work;
  if (int rc = check_call64(ctx, segs, n_segs, q, t, nullptr, 1, &records, &kinds, &flat, &work)) return rc;
  HostPlan hp;   // the planner is the predicate for the clauses, as in nrtgpu_query_supported
  return final_score_plan(ctx, segs, nullptr, n_segs, flat.queries.data(), 1, "terms count", hp);
}

extern "C" int nrtgpu_count_terms64_batch(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                          const nrtgpu_bm25_query* queries, const nrtgpu_terms_count* terms, int32_t n_queries,
                                          nrtgpu_term_counts64* out) {
  if (int rc = final_score_enter(ctx, segs, n_segs, !queries || !terms || !out, &n_queries)) return rc;
  const double t0 = now_ms();
  SegReadLocks content(segs, n_segs);   // until this call's kernels have finished
  std::vector<DTermsQuery> records;
  std::vector<int> kinds;
  FlatQueries flat;
  TermsWork64 work;
  if (int rc = check_call64(ctx, segs, n_segs, queries, terms, out, n_queries, &records, &kinds, &flat, &work)) return rc;
  HostPlan hp;
  if (int rc = final_score_plan(ctx, segs, doc_bases, n_segs, flat.queries.data(), n_queries, "terms count", hp)) return rc;
  std::vector<int32_t> leaves;
  if (int rc = doc_values_part_leaves(segs, n_segs, hp, "terms count", &leaves)) return rc;
  std::vector<DSort64Part> sparts(hp.parts.size(), DSort64Part{nullptr, nullptr});
  for (const DItem& it : hp.items)
    for (uint32_t pi = 0; pi < it.n_parts; ++pi) sparts[it.part_begin + pi] = doc_values_column64(segs[leaves[it.part_begin + pi]], terms[it.query].field_id);
  const PlanBytes extras[2] = {{records.data(), records.size() * sizeof(DTermsQuery)}, {sparts.data(), sparts.size() * sizeof(DSort64Part)}};
  std::vector<nrtgpu_topdocs> pages((size_t)n_queries, nrtgpu_topdocs{});   // (no hits come back: the merge's lists are empty; total_hits is read from them)
  const FinalScoreOwn own{work.bytes, terms64_collect, &work};
  const FinalScoreLaunch launch = [](hipStream_t st, const FinalScoreArgs& a, const void* const* d_extra) {
    const TermsWork64* w = (const TermsWork64*)a.own_user;
    DTermsState64* states;
    unsigned long long *keys, *out_codes;
    uint32_t *counts, *out_counts;
    terms64_regions(*w, (char*)a.own, &states, &keys, &counts, &out_codes, &out_counts);
    launch_bm25_terms_count64(st, a, (const DTermsQuery*)d_extra[0], (const DSort64Part*)d_extra[1], states, keys, counts, out_codes, out_counts,
                              (uint32_t)w->n_queries, w->out_cap);
  };
  if (int rc = final_score_run(ctx, hp, queries, n_queries, pages.data(), t0, extras, 2, launch, &own)) return rc;
  return terms64_unpack(work, kinds, pages.data(), n_queries, out);
}
