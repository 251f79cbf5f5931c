// fieldsort64.cpp -- sort by a 64-bit field (include/nrtgpu.h: nrtgpu_search_sorted64_batch, nrtgpu_sort_key64): a text query's
// hits ordered by a LONG / DATE_TIME / DOUBLE doc value column (segment.cpp: nrtgpu_segment_add_doc_values64).  The host path is
// fieldsort.cpp's -- the same checks, the same flat copies planned through final_score_plan, doc_values_part_leaves' walk,
// final_score_run -- with three things of its own: the per-query record (plan.h: DSort64Query) carries the WINDOW of the column's
// codes over the call's leaves and the bits the call's docids need, a sort whose window does not fit the key is refused here, and
// the pages come back through internal nrtgpu_topdocs (unpack_topdocs is a bit copy: key = high << 32 | (0xFFFFFFFF - doc)) whose
// keys are decoded into the caller's nrtgpu_fielddocs64.  What the doc-set form (docset.cpp) shares is declared in
// runtime_internal.h.
#include <cstddef>

#include "runtime_internal.h"

static_assert(sizeof(nrtgpu_field_sort64) == 32 && offsetof(nrtgpu_field_sort64, missing_bits) == 8 && offsetof(nrtgpu_field_sort64, after_bits) == 24,
              "nrtgpu_field_sort64 layout");
static_assert(sizeof(nrtgpu_fielddocs64) == 40 && offsetof(nrtgpu_fielddocs64, value_bits) == 16 && offsetof(nrtgpu_fielddocs64, total_hits) == 24,
              "nrtgpu_fielddocs64 layout");
static_assert(NRTGPU_DOCVALUES_INT64 == kDocValuesInt64 && NRTGPU_DOCVALUES_FLOAT64 == kDocValuesFloat64, "NRTGPU_DOCVALUES_*64");

extern "C" int nrtgpu_sort_key64(int32_t kind, int32_t reverse, uint64_t lo_bits, uint64_t hi_bits, uint64_t missing_bits, int32_t doc_bits,
                                 int32_t has_value, uint64_t value_bits, int32_t global_doc, uint64_t* out_key) {
  if (!out_key) return fail(NRTGPU_ERR_INVALID_ARG, "NULL argument");
  if (kind != NRTGPU_DOCVALUES_INT64 && kind != NRTGPU_DOCVALUES_FLOAT64) return fail(NRTGPU_ERR_INVALID_ARG, "64-bit doc values kind %d outside 2..3", kind);
  if (reverse != 0 && reverse != 1) return fail(NRTGPU_ERR_INVALID_ARG, "reverse %d outside 0..1", reverse);
  if (has_value != 0 && has_value != 1) return fail(NRTGPU_ERR_INVALID_ARG, "has_value %d outside 0..1", has_value);
  if (doc_bits < 1 || doc_bits > 31) return fail(NRTGPU_ERR_INVALID_ARG, "doc_bits %d outside 1..31", doc_bits);
  if (global_doc < 0 || (uint32_t)global_doc > (1u << doc_bits) - 1u) return fail(NRTGPU_ERR_INVALID_ARG, "global_doc %d outside [0, 2^%d)", global_doc, doc_bits);
  const uint64_t lo = doc_value_code64(kind, lo_bits), hi = doc_value_code64(kind, hi_bits);
  if (lo > hi) return fail(NRTGPU_ERR_INVALID_ARG, "lo sorts behind hi in the kind's order");
  const uint64_t code = doc_value_code64(kind, has_value ? value_bits : missing_bits);
  if (has_value && (code < lo || code > hi)) return fail(NRTGPU_ERR_INVALID_ARG, "a value outside [lo, hi]");
  const uint64_t span = hi - lo;
  if (!sort64_fits(span, (uint32_t)doc_bits))
    return fail(NRTGPU_ERR_UNSUPPORTED, "span needs %d bits, %d-bit docids leave %d", sort64_value_bits(span), doc_bits, 64 - doc_bits);
  *out_key = sort_key64((uint32_t)reverse, lo, span, (uint32_t)doc_bits, code, (uint32_t)global_doc);
  return NRTGPU_OK;
}

namespace nrtgpu {
namespace rt {

int field_sort64_narrow(int qi, int32_t field_id, bool multi, const char* entry32) {
  return fail(NRTGPU_ERR_UNSUPPORTED, "query %d: the doc values of field %d are a %s column: sort by it with %s", qi, field_id,
              multi ? "multi-valued 32-bit" : "32-bit", entry32);
}

int sort64_doc_bits(const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs, bool in_order, uint32_t* db) {
  uint64_t D = 1, next = 0;
  for (int32_t si = 0; si < n_segs; ++si) {
    const uint64_t base = doc_bases ? (uint64_t)(uint32_t)std::max(doc_bases[si], 0) : in_order ? next : 0ull;
    const uint64_t end = base + (uint64_t)segs[si]->max_doc;
    next = end;
    D = std::max(D, end);
  }
  if (D > (1ull << 31))
    return fail(NRTGPU_ERR_UNSUPPORTED, "the leaves of the call reach global docid %llu: docids stay below 2^31", (unsigned long long)(D - 1));
  uint32_t bits = 0;
  for (uint64_t v = D - 1; v != 0; v >>= 1) ++bits;
  *db = std::max(bits, 1u);
  return NRTGPU_OK;
}

int field_sort64_record(const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_field_sort64& s, int kind, uint32_t db, int qi, DSort64Query* r) {
  r->reverse = (uint32_t)s.reverse;
  r->missing_code = doc_value_code64(kind, s.missing_bits);
  r->has_after = (uint32_t)s.has_after;
  r->after_code = s.has_after ? doc_value_code64(kind, s.after_bits) : 0ull;
  r->after_doc = s.has_after ? (uint32_t)s.after_doc : 0u;
  r->db = db;
  uint64_t lo = r->missing_code, hi = r->missing_code;   // (no leaf holds a value: every doc sorts as the missing value)
  bool any = false;
  for (int32_t si = 0; si < n_segs; ++si) {
    const auto fit = segs[si]->fields.find(s.field_id);
    if (fit == segs[si]->fields.end() || fit->second.dv_kind != kind || fit->second.dv_n <= 0) continue;
    lo = any ? std::min(lo, fit->second.dv_min_code) : fit->second.dv_min_code;
    hi = any ? std::max(hi, fit->second.dv_max_code) : fit->second.dv_max_code;
    any = true;
  }
  r->lo = lo;
  r->span = hi - lo;
  if (!sort64_fits(r->span, db))
    return fail(NRTGPU_ERR_UNSUPPORTED, "query %d: the sort by field %d does not fit the top-k's 64-bit keys: span needs %d bits, %u-bit docids leave %u", qi,
                s.field_id, sort64_value_bits(r->span), db, 64u - db);
  return NRTGPU_OK;
}

DSort64Part doc_values_column64(const nrtgpu_seg* seg, int32_t field_id) {
  const auto fit = seg->fields.find(field_id);
  if (fit == seg->fields.end() || fit->second.dv_kind < kDocValuesInt64) return DSort64Part{nullptr, nullptr};
  return DSort64Part{fit->second.d_dv_code64, fit->second.d_dv_has};
}

Sort64Pages::Sort64Pages(const int32_t* ks, const nrtgpu_fielddocs64* out, int32_t n_queries) : pages((size_t)n_queries, nrtgpu_topdocs{}) {
  size_t total = 0;
  std::vector<size_t> at((size_t)n_queries);
  for (int qi = 0; qi < n_queries; ++qi) {
    at[(size_t)qi] = total;
    total += (size_t)std::max(out[qi].capacity > 0 ? out[qi].capacity : ks[qi], 0);
  }
  docs.resize(total);
  highs.resize(total);
  for (int qi = 0; qi < n_queries; ++qi) {
    pages[(size_t)qi].capacity = out[qi].capacity;   // (unpack_topdocs: 0 = the query's k)
    pages[(size_t)qi].docs = docs.data() + at[(size_t)qi];
    pages[(size_t)qi].scores = highs.data() + at[(size_t)qi];
  }
}

void Sort64Pages::decode(const std::vector<DSort64Query>& records, const std::vector<int>& kinds, nrtgpu_fielddocs64* out) const {
  for (size_t qi = 0; qi < pages.size(); ++qi) {
    const nrtgpu_topdocs& p = pages[qi];
    const DSort64Query& r = records[qi];
    nrtgpu_fielddocs64& o = out[qi];
    o.n_hits = p.n_hits;
    o.total_hits = p.total_hits;
    o.total_hits_is_lower_bound = p.total_hits_is_lower_bound;
    for (int32_t i = 0; i < p.n_hits; ++i) {
      uint32_t high;
      memcpy(&high, &p.scores[i], 4);
      const uint64_t key = ((uint64_t)high << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)p.docs[i]);   // unpack_topdocs' bit copy, undone
      uint32_t doc;
      uint64_t u;
      sort_key64_decode(r.reverse, r.span, r.db, key, &doc, &u);
      if (o.docs) o.docs[i] = (int32_t)doc;
      if (o.value_bits) o.value_bits[i] = doc_value_bits64(kinds[qi], (u == 0ull || u == r.span + 2ull) ? r.missing_code : r.lo + (u - 1ull));
    }
  }
}

}  // namespace rt
}  // namespace nrtgpu

namespace {

// What the route refuses of a call before anything is planned (fieldsort.cpp: check_call, with the 64-bit column's own checks);
// in_order: the predicate's doc bases.
int check_call64(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs, bool in_order, const nrtgpu_bm25_query* queries,
                 const nrtgpu_field_sort64* sorts, int32_t n_queries, std::vector<DSort64Query>* records, std::vector<int>* kinds, FlatQueries* flat) {
  flat->queries.reserve((size_t)n_queries);
  flat->terms.reserve((size_t)n_queries);
  std::vector<char> multi;
  for (int qi = 0; qi < n_queries; ++qi) {
    const nrtgpu_bm25_query& q = queries[qi];
    if (int rc = validate_query(q, qi)) return rc;
    if (int rc = field_sort_check(sorts[qi], qi)) return rc;
    if (q.has_after != 0) return fail(NRTGPU_ERR_INVALID_ARG, "query %d: the query's has_after must be 0 (the cursor of a sorted search lives in the sort)", qi);
    int kind = -1;
    bool m = false;
    if (int rc = doc_values_kind(segs, n_segs, sorts[qi].field_id, qi, &kind, &m)) return rc;
    kinds->push_back(kind);
    multi.push_back(m ? 1 : 0);
  }
  if (int rc = final_score_check_flags(ctx, "sorted")) return rc;
  uint32_t db = 1;
  for (int qi = 0; qi < n_queries; ++qi) {
    const nrtgpu_field_sort64& s = sorts[qi];
    const int kind = (*kinds)[(size_t)qi];
    DSort64Query r{};
    if (kind >= 0 && kind < kDocValuesInt64) return field_sort64_narrow(qi, s.field_id, multi[(size_t)qi] != 0, "nrtgpu_search_sorted_batch");
    if (int rc = doc_values_query(segs, n_segs, queries[qi], qi, kind, s.field_id, "a sort", &r.need, flat)) return rc;
    if (qi == 0)
      if (int rc = sort64_doc_bits(segs, doc_bases, n_segs, in_order, &db)) return rc;
    if (int rc = field_sort64_record(segs, n_segs, s, kind, db, qi, &r)) return rc;
    records->push_back(r);
  }
  for (int qi = 0; qi < n_queries; ++qi) flat->queries[(size_t)qi].terms = flat->terms[(size_t)qi].data();   // (the vectors have settled)
  return NRTGPU_OK;
}

}  // namespace

extern "C" int nrtgpu_sorted64_supported(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_bm25_query* q,
                                         const nrtgpu_field_sort64* s) {
  if (int rc = final_score_enter(ctx, segs, n_segs, !q || !s, nullptr)) return rc;
  SegReadLocks content(segs, n_segs);
  std::vector<DSort64Query> records;
  std::vector<int> kinds;
  FlatQueries flat;
  if (int rc = check_call64(ctx, segs, nullptr, n_segs, true, q, s, 1, &records, &kinds, &flat)) return rc;
  HostPlan hp;   // the planner is the predicate for the clauses, as in nrtgpu_query_supported
  return final_score_plan(ctx, segs, nullptr, n_segs, flat.queries.data(), 1, "sorted", hp);
}

extern "C" int nrtgpu_search_sorted64_batch(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                            const nrtgpu_bm25_query* queries, const nrtgpu_field_sort64* sorts, int32_t n_queries,
                                            nrtgpu_fielddocs64* out) {
  if (int rc = final_score_enter(ctx, segs, n_segs, !queries || !sorts || !out, &n_queries)) return rc;
  const double t0 = now_ms();
  SegReadLocks content(segs, n_segs);   // until this call's kernels have finished
  std::vector<DSort64Query> records;
  std::vector<int> kinds;
  FlatQueries flat;
  records.reserve((size_t)n_queries);
  if (int rc = check_call64(ctx, segs, doc_bases, n_segs, false, queries, sorts, n_queries, &records, &kinds, &flat)) return rc;
  HostPlan hp;
  if (int rc = final_score_plan(ctx, segs, doc_bases, n_segs, flat.queries.data(), n_queries, "sorted", hp)) return rc;
  std::vector<int32_t> leaves;
  if (int rc = doc_values_part_leaves(segs, n_segs, hp, "sorted", &leaves)) return rc;
  std::vector<DSort64Part> sparts(hp.parts.size(), DSort64Part{nullptr, nullptr});
  for (const DItem& it : hp.items)
    for (uint32_t pi = 0; pi < it.n_parts; ++pi) sparts[it.part_begin + pi] = doc_values_column64(segs[leaves[it.part_begin + pi]], sorts[it.query].field_id);
  const PlanBytes extras[2] = {{records.data(), records.size() * sizeof(DSort64Query)}, {sparts.data(), sparts.size() * sizeof(DSort64Part)}};
  std::vector<int32_t> ks((size_t)n_queries);
  for (int qi = 0; qi < n_queries; ++qi) ks[(size_t)qi] = queries[qi].k;
  Sort64Pages pages(ks.data(), out, n_queries);
  if (int rc = final_score_run(ctx, hp, queries, n_queries, pages.pages.data(), t0, extras, 2, [](hipStream_t st, const FinalScoreArgs& a, const void* const* d_extra) {
        launch_bm25_field_sort64(st, a, (const DSort64Query*)d_extra[0], (const DSort64Part*)d_extra[1]);
      }))
    return rc;
  pages.decode(records, kinds, out);
  return NRTGPU_OK;
}
