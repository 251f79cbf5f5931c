// rangecount.cpp -- numeric range facets (include/nrtgpu.h: nrtgpu_count_ranges_batch, nrtgpu_range_cuts, nrtgpu_range_interval):
// a text query's hits counted per requested value range of a single-valued doc value column of any of the four kinds.  The host
// path is termscount.cpp's -- the same checks in the same order, the flat copies planned through final_score_plan,
// doc_values_part_leaves' walk, final_score_run with workspace bytes of the route's own (FinalScoreOwn: zeroed per call by the
// memset that zeroes the per-slice sums) -- with a far smaller aggregation state: per query the cut points of its ranges (plan.h:
// range_cuts) and n_cuts + 1 uint32 interval counters.  There is no overflow state, no compaction kernel and no bucket bound:
// collect() copies exactly the counters that exist, and the roll-up here sums, per range, the counters of the intervals it covers
// (exact integer sums).  What the doc-set form (docset.cpp) shares is declared in runtime_internal.h.
#include <cstddef>

#include "runtime_internal.h"

static_assert(sizeof(nrtgpu_value_range) == 16, "nrtgpu_value_range layout");
static_assert(sizeof(nrtgpu_range_count) == 16 && offsetof(nrtgpu_range_count, ranges) == 8, "nrtgpu_range_count layout");
static_assert(sizeof(nrtgpu_range_counts) == 32 && offsetof(nrtgpu_range_counts, capacity) == 8 && offsetof(nrtgpu_range_counts, total_hits) == 16 &&
                  offsetof(nrtgpu_range_counts, hits_with_value) == 24,
              "nrtgpu_range_counts layout");
static_assert(NRTGPU_MAX_COUNT_RANGES == kMaxCountRanges, "NRTGPU_MAX_COUNT_RANGES");

namespace {

bool kind_ok(int32_t kind) { return kind >= kDocValuesInt32 && kind <= kDocValuesFloat64; }
bool kind_wide(int kind) { return kind >= kDocValuesInt64; }
uint64_t code_of(int kind, uint64_t bits) { return kind_wide(kind) ? doc_value_code64(kind, bits) : (uint64_t)doc_value_code(kind, (uint32_t)bits); }

// the codes of a range list and its cuts (as 64-bit words, whatever the kind's width)
uint32_t cuts_of(int kind, const nrtgpu_value_range* ranges, int32_t n_ranges, uint64_t* lo, uint64_t* hi, uint64_t* cuts) {
  for (int32_t i = 0; i < n_ranges; ++i) {
    lo[i] = code_of(kind, ranges[i].lower_bits);
    hi[i] = code_of(kind, ranges[i].upper_bits);
  }
  return range_cuts(lo, hi, (uint32_t)n_ranges, range_greatest_code(kind), cuts);
}

}  // namespace

extern "C" int nrtgpu_range_cuts(int32_t kind, const nrtgpu_value_range* ranges, int32_t n_ranges, uint64_t* out_cuts, int32_t* out_n_cuts) {
  if (!out_cuts || !out_n_cuts || (n_ranges > 0 && !ranges)) return fail(NRTGPU_ERR_INVALID_ARG, "NULL argument");
  if (!kind_ok(kind)) return fail(NRTGPU_ERR_INVALID_ARG, "doc values kind %d outside 0..3", kind);
  if (n_ranges < 0 || n_ranges > NRTGPU_MAX_COUNT_RANGES) return fail(NRTGPU_ERR_INVALID_ARG, "n_ranges %d outside 0..%d", n_ranges, NRTGPU_MAX_COUNT_RANGES);
  for (int32_t i = 0; i < n_ranges; ++i)
    if (!kind_wide(kind) && ((ranges[i].lower_bits | ranges[i].upper_bits) >> 32) != 0ull)
      return fail(NRTGPU_ERR_INVALID_ARG, "range %d: a bound of a 32-bit kind with a non-zero high word", i);
  uint64_t lo[kMaxCountRanges], hi[kMaxCountRanges];
  *out_n_cuts = (int32_t)cuts_of(kind, ranges, n_ranges, lo, hi, out_cuts);
  return NRTGPU_OK;
}

extern "C" int nrtgpu_range_interval(int32_t kind, const uint64_t* cuts, int32_t n_cuts, uint64_t value_bits, int32_t* out_interval) {
  if (!out_interval || (n_cuts > 0 && !cuts)) return fail(NRTGPU_ERR_INVALID_ARG, "NULL argument");
  if (!kind_ok(kind)) return fail(NRTGPU_ERR_INVALID_ARG, "doc values kind %d outside 0..3", kind);
  if (n_cuts < 0 || n_cuts > kMaxRangeCuts) return fail(NRTGPU_ERR_INVALID_ARG, "n_cuts %d outside 0..%d", n_cuts, kMaxRangeCuts);
  if (!kind_wide(kind) && (value_bits >> 32) != 0ull) return fail(NRTGPU_ERR_INVALID_ARG, "a value of a 32-bit kind with a non-zero high word");
  *out_interval = (int32_t)range_interval(cuts, (uint32_t)n_cuts, code_of(kind, value_bits));
  return NRTGPU_OK;
}

namespace nrtgpu {
namespace rt {

// ---- what the routes that count ranges share (this file: a text query's hits; docset.cpp: a doc set) ----------------------------
int range_count_begin(const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_range_count& r, const nrtgpu_range_counts* out, int qi, RangeWork* work) {
  if (r.n_ranges < 1 || r.n_ranges > NRTGPU_MAX_COUNT_RANGES)
    return fail(NRTGPU_ERR_INVALID_ARG, "query %d: n_ranges %d outside 1..%d", qi, r.n_ranges, NRTGPU_MAX_COUNT_RANGES);
  if (!r.ranges) return fail(NRTGPU_ERR_INVALID_ARG, "query %d: ranges is NULL", qi);
  if (out && (out->capacity < r.n_ranges || !out->counts))
    return fail(NRTGPU_ERR_INVALID_ARG, "query %d: an output of capacity %d (or NULL counts) for %d ranges", qi, out->capacity, r.n_ranges);
  if (out && out->reserved != 0) return fail(NRTGPU_ERR_INVALID_ARG, "query %d: the output's reserved must be 0", qi);
  int kind = -1;
  bool multi = false;
  if (int rc = doc_values_kind(segs, n_segs, r.field_id, qi, &kind, &multi)) return rc;
  if (kind >= 0 && !kind_wide(kind))
    for (int32_t i = 0; i < r.n_ranges; ++i)
      if (((r.ranges[i].lower_bits | r.ranges[i].upper_bits) >> 32) != 0ull)
        return fail(NRTGPU_ERR_INVALID_ARG, "query %d: range %d: a bound with a non-zero high word over the 32-bit column of field %d", qi, i, r.field_id);
  work->kinds.push_back(kind);
  work->multi.push_back(multi ? 1 : 0);
  return NRTGPU_OK;
}

int range_count_column(const RangeWork& work, const nrtgpu_range_count* ranges, int qi) {
  const int kind = work.kinds[(size_t)qi];
  if (kind < 0) return NRTGPU_OK;   // (the caller's "resident on no leaf" follows)
  if (work.multi[(size_t)qi] != 0)
    return fail(NRTGPU_ERR_UNSUPPORTED, "query %d: the doc values of field %d are multi-valued: a range facet over such a column counts a doc once per range, "
                "which the interval counters do not do", qi, ranges[qi].field_id);
  for (int other = 0; other < qi; ++other)
    if (work.kinds[(size_t)other] >= 0 && kind_wide(work.kinds[(size_t)other]) != kind_wide(kind))
      return fail(NRTGPU_ERR_UNSUPPORTED, "query %d: the column of field %d is a %d-bit one, query %d counts a %d-bit one: split the batch by column width", qi,
                  ranges[qi].field_id, kind_wide(kind) ? 64 : 32, other, kind_wide(kind) ? 32 : 64);
  return NRTGPU_OK;
}

void RangeWork::layout(const nrtgpu_range_count* ranges, int32_t n) {
  n_queries = n;
  wide = n > 0 && kind_wide(kinds[0]);
  records.assign((size_t)n, DRangeCountQuery{});
  std::vector<uint64_t> cuts;
  uint64_t lo[kMaxCountRanges], hi[kMaxCountRanges], mine[kMaxRangeCuts];
  uint32_t n_counters = 0;
  for (int qi = 0; qi < n; ++qi) {
    const uint32_t nc = cuts_of(kinds[(size_t)qi], ranges[qi].ranges, ranges[qi].n_ranges, lo, hi, mine);
    DRangeCountQuery& r = records[(size_t)qi];
    r.n_cuts = nc;
    r.cut_off = (uint32_t)cuts.size();
    r.counter_off = n_counters;
    cuts.insert(cuts.end(), mine, mine + nc);
    n_counters += nc + 1u;
  }
  // the plan's bytes: the records, then the call's cut array at the column width
  const size_t cut_bytes = cuts.size() * (wide ? 8 : 4);
  plan_bytes.assign((size_t)n * sizeof(DRangeCountQuery) + cut_bytes, 0);
  if (cut_bytes == 0) {   // every range of the call is empty: no cut, one counter per query
  } else if (wide) {
    memcpy(plan_bytes.data() + (size_t)n * sizeof(DRangeCountQuery), cuts.data(), cut_bytes);
  } else {
    std::vector<uint32_t> narrow(cuts.begin(), cuts.end());
    memcpy(plan_bytes.data() + (size_t)n * sizeof(DRangeCountQuery), narrow.data(), cut_bytes);
  }
  counters.assign(n_counters, 0u);
  bytes = (size_t)n_counters * 4;
}

// the interval of a code among query r's cuts, read where they lie in plan_bytes at the call's width
uint32_t RangeWork::interval_of(const DRangeCountQuery& r, uint64_t code) const {
  const char* const cut_bytes = plan_bytes.data() + (size_t)n_queries * sizeof(DRangeCountQuery);
  return wide ? range_interval((const uint64_t*)cut_bytes + r.cut_off, r.n_cuts, code)
              : range_interval((const uint32_t*)cut_bytes + r.cut_off, r.n_cuts, (uint32_t)code);
}

void RangeWork::seal() { memcpy(plan_bytes.data(), records.data(), records.size() * sizeof(DRangeCountQuery)); }

// Behind the wait: exactly the counters that exist.
int range_collect(nrtgpu_ctx* ctx, Slot* slot, const char* d_own, void* user) {
  RangeWork* w = (RangeWork*)user;
  if (w->counters.empty()) return NRTGPU_OK;
  const bool blocking = (ctx->cfg.flags & NRTGPU_FLAG_BLOCKING_WAIT) != 0;
  HIP_TRY(hipMemcpyAsync(w->counters.data(), d_own, w->counters.size() * 4, hipMemcpyDeviceToHost, slot->stream));
  HIP_TRY(wait_for_stream(blocking, slot->stream, slot->ev_wait));
  return NRTGPU_OK;
}

// The roll-up: counts[i] = the sum of the interval counters over [interval(lo_i), interval(hi_i)]; hits_with_value = the sum of
// all of the query's counters (a valued hit lies in exactly one interval).
int range_unpack(const RangeWork& work, const nrtgpu_range_count* ranges, const nrtgpu_topdocs* pages, int32_t n_queries, nrtgpu_range_counts* out) {
  for (int qi = 0; qi < n_queries; ++qi) {
    nrtgpu_range_counts& o = out[qi];
    const DRangeCountQuery& r = work.records[(size_t)qi];
    const int kind = work.kinds[(size_t)qi];
    const uint32_t* const c = work.counters.data() + r.counter_off;
    o.total_hits = pages[(size_t)qi].total_hits;
    o.hits_with_value = 0;
    for (uint32_t i = 0; i <= r.n_cuts; ++i) o.hits_with_value += (int64_t)c[i];
    for (int32_t i = 0; i < ranges[qi].n_ranges; ++i) {
      const uint64_t lo = code_of(kind, ranges[qi].ranges[i].lower_bits), hi = code_of(kind, ranges[qi].ranges[i].upper_bits);
      int64_t sum = 0;
      if (lo <= hi) {
        for (uint32_t iv = work.interval_of(r, lo), last = work.interval_of(r, hi); iv <= last; ++iv) sum += (int64_t)c[iv];
      }
      o.counts[i] = sum;
    }
  }
  return NRTGPU_OK;
}

// the count column of one leaf as the kernels read it: DSortPart.code is the column of the call's width
DSortPart range_count_column_of(const nrtgpu_seg* seg, int32_t field_id, bool wide) {
  if (!wide) return doc_values_column(seg, field_id);
  const DSort64Part p = doc_values_column64(seg, field_id);
  return DSortPart{(const uint32_t*)p.code64, p.has};
}

}  // namespace rt
}  // namespace nrtgpu

namespace {

// What the route refuses of a call before anything is planned (termscount.cpp: check_call, with the range list's own checks).
// out: the batch entry's outputs, nullptr for the predicate.
int check_call(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_bm25_query* queries, const nrtgpu_range_count* ranges,
               const nrtgpu_range_counts* out, int32_t n_queries, FlatQueries* flat, RangeWork* work) {
  flat->queries.reserve((size_t)n_queries);
  flat->terms.reserve((size_t)n_queries);
  for (int qi = 0; qi < n_queries; ++qi) {
    if (int rc = validate_query(queries[qi], qi)) return rc;
    if (int rc = range_count_begin(segs, n_segs, ranges[qi], out ? &out[qi] : nullptr, qi, work)) return rc;
  }
  if (int rc = final_score_check_flags(ctx, "range count")) return rc;
  std::vector<uint32_t> need((size_t)n_queries, 0u);
  for (int qi = 0; qi < n_queries; ++qi) {
    if (int rc = range_count_column(*work, ranges, qi)) return rc;
    if (int rc = doc_values_query(segs, n_segs, queries[qi], qi, work->kinds[(size_t)qi], ranges[qi].field_id, "a range count", &need[(size_t)qi], flat)) return rc;
  }
  for (int qi = 0; qi < n_queries; ++qi) flat->queries[(size_t)qi].terms = flat->terms[(size_t)qi].data();   // (the vectors have settled)
  work->layout(ranges, n_queries);
  for (int qi = 0; qi < n_queries; ++qi) work->records[(size_t)qi].need = need[(size_t)qi];
  work->seal();
  return NRTGPU_OK;
}

}  // namespace

extern "C" int nrtgpu_count_ranges_supported(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_bm25_query* q,
                                             const nrtgpu_range_count* r) {
  if (int rc = final_score_enter(ctx, segs, n_segs, !q || !r, nullptr)) return rc;
  SegReadLocks content(segs, n_segs);
  FlatQueries flat;
  RangeWork work;
  if (int rc = check_call(ctx, segs, n_segs, q, r, nullptr, 1, &flat, &work)) return rc;
  HostPlan hp;   // the planner is the predicate for the clauses, as in nrtgpu_query_supported
  return final_score_plan(ctx, segs, nullptr, n_segs, flat.queries.data(), 1, "range count", hp);
}

extern "C" int nrtgpu_count_ranges_batch(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                         const nrtgpu_bm25_query* queries, const nrtgpu_range_count* ranges, int32_t n_queries,
                                         nrtgpu_range_counts* out) {
  if (int rc = final_score_enter(ctx, segs, n_segs, !queries || !ranges || !out, &n_queries)) return rc;
  const double t0 = now_ms();
  SegReadLocks content(segs, n_segs);   // until this call's kernels have finished
  FlatQueries flat;
  RangeWork work;
  if (int rc = check_call(ctx, segs, n_segs, queries, ranges, out, n_queries, &flat, &work)) return rc;
  HostPlan hp;
  if (int rc = final_score_plan(ctx, segs, doc_bases, n_segs, flat.queries.data(), n_queries, "range count", hp)) return rc;
  std::vector<int32_t> leaves;
  if (int rc = doc_values_part_leaves(segs, n_segs, hp, "range count", &leaves)) return rc;
  std::vector<DSortPart> sparts(hp.parts.size(), DSortPart{nullptr, nullptr});
  for (const DItem& it : hp.items)
    for (uint32_t pi = 0; pi < it.n_parts; ++pi)
      sparts[it.part_begin + pi] = range_count_column_of(segs[leaves[it.part_begin + pi]], ranges[it.query].field_id, work.wide);
  const PlanBytes extras[2] = {{work.plan_bytes.data(), work.plan_bytes.size()}, {sparts.data(), sparts.size() * sizeof(DSortPart)}};
  std::vector<nrtgpu_topdocs> pages((size_t)n_queries, nrtgpu_topdocs{});   // (no hits come back: the merge's lists are empty; total_hits is read from them)
  const FinalScoreOwn own{work.bytes, range_collect, &work};
  const FinalScoreLaunch launch = [](hipStream_t st, const FinalScoreArgs& a, const void* const* d_extra) {
    const RangeWork* w = (const RangeWork*)a.own_user;
    const char* d_plan = (const char*)d_extra[0];
    launch_bm25_range_count(st, w->wide, a, (const DRangeCountQuery*)d_plan, (const DSortPart*)d_extra[1],
                            d_plan + (size_t)w->n_queries * sizeof(DRangeCountQuery), (uint32_t*)a.own);
  };
  if (int rc = final_score_run(ctx, hp, queries, n_queries, pages.data(), t0, extras, 2, launch, &own)) return rc;
  return range_unpack(work, ranges, pages.data(), n_queries, out);
}
