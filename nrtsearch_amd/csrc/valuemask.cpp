// valuemask.cpp -- filter masks built on the device from doc value columns (include/nrtgpu.h: nrtgpu_segment_set_mask_from_values,
// nrtgpu_segment_set_mask_from_values64 over 64-bit columns, nrtgpu_segment_get_mask).  The host side of valuemask.hip: the checks, the clauses as DValueClause records over the leaf's resident
// columns (plan.h), the IN_SET values as sorted duplicate-free codes, one launch, the words copied back into seg->masks -- from
// there on the mask is one that nrtgpu_segment_set_mask registered: the accept sets, their cache and every residency check are
// segment.cpp's and read the host copy.  Nothing stays resident: the call's device buffer is freed before it returns.
#include <cstddef>

#include "runtime_internal.h"

static_assert(sizeof(nrtgpu_value_clause) == 32 && offsetof(nrtgpu_value_clause, lower_bits) == 8 && offsetof(nrtgpu_value_clause, n_values) == 16 &&
                  offsetof(nrtgpu_value_clause, value_bits) == 24,
              "nrtgpu_value_clause layout");
static_assert(NRTGPU_MAX_SET_VALUES == kMaxSetValues, "NRTGPU_MAX_SET_VALUES");
static_assert(NRTGPU_MAX_RANGES == kMaxRanges, "NRTGPU_MAX_RANGES");

namespace {

// What the builder refuses of clauses[i] as an invalid argument, the header's table in its order.
int check_clause(const nrtgpu_value_clause& c, int i) {
  if (c.kind < NRTGPU_CLAUSE_RANGE || c.kind > NRTGPU_CLAUSE_IN_SET) return fail(NRTGPU_ERR_INVALID_ARG, "clause %d: kind %d outside 0..2", i, c.kind);
  if (c.reserved != 0) return fail(NRTGPU_ERR_INVALID_ARG, "clause %d: reserved must be 0", i);
  if (c.kind == NRTGPU_CLAUSE_IN_SET) {
    if (c.n_values < 1 || c.n_values > NRTGPU_MAX_SET_VALUES)
      return fail(NRTGPU_ERR_INVALID_ARG, "clause %d: n_values %d outside 1..%d", i, c.n_values, NRTGPU_MAX_SET_VALUES);
    if (!c.value_bits) return fail(NRTGPU_ERR_INVALID_ARG, "clause %d: value_bits is NULL with n_values %d", i, c.n_values);
  } else if (c.n_values != 0 || c.value_bits) {
    return fail(NRTGPU_ERR_INVALID_ARG, "clause %d: a range / exists clause takes no values (n_values %d)", i, c.n_values);
  }
  return NRTGPU_OK;
}

struct DeviceBuffer {   // the call's one allocation
  void* p = nullptr;
  ~DeviceBuffer() {
    if (p) (void)hipFree(p);
  }
};
struct TimingEvents {   // nrtgpu_config.collect_timing: the kernel's own time
  hipEvent_t a = nullptr, b = nullptr;
  ~TimingEvents() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
};

size_t pad256(size_t n) { return (n + 255) & ~(size_t)255; }

// From "the clauses' records exist" to "the mask is registered": one buffer -- the records, the code sets, the words -- one
// launch (launch(records, sets, words, n_words) on the device's addresses), the words back, the mask under mask_id.  The caller
// holds the segment's write lock.
template <class Launch>
int build_mask(nrtgpu_seg* seg, int32_t mask_id, const void* records, size_t record_bytes, const std::vector<uint32_t>& sets, Launch launch,
               int64_t* out_count, double t0) {
  HIP_TRY(hipSetDevice(seg->ctx->device));
  const size_t need = (size_t)(seg->max_doc + 63) / 64;
  const size_t o_sets = pad256(record_bytes), o_words = o_sets + pad256(sets.size() * 4), bytes = o_words + need * 8;
  DeviceBuffer buf;
  HIP_TRY(hipMalloc(&buf.p, bytes));
  char* const d = (char*)buf.p;
  std::vector<char> head(o_words, 0);
  memcpy(head.data(), records, record_bytes);
  if (!sets.empty()) memcpy(head.data() + o_sets, sets.data(), sets.size() * 4);
  HIP_TRY(hipMemcpy(d, head.data(), o_words, hipMemcpyHostToDevice));
  const bool timing = seg->ctx->cfg.collect_timing != 0;
  TimingEvents ev;
  if (timing) {
    HIP_TRY(hipEventCreate(&ev.a));
    HIP_TRY(hipEventCreate(&ev.b));
    HIP_TRY(hipEventRecord(ev.a, nullptr));
  }
  launch((const void*)d, (const uint32_t*)(d + o_sets), (uint64_t*)(d + o_words), (uint32_t)need);
  HIP_TRY(hipGetLastError());
  if (timing) HIP_TRY(hipEventRecord(ev.b, nullptr));
  std::vector<uint64_t> words(need);
  HIP_TRY(hipMemcpy(words.data(), d + o_words, need * 8, hipMemcpyDeviceToHost));   // (behind the kernel: the same stream)
  float kernel_ms = 0.f;
  if (timing) {
    HIP_TRY(hipEventSynchronize(ev.b));
    (void)hipEventElapsedTime(&kernel_ms, ev.a, ev.b);
  }

  int64_t n_set = 0;   // (the kernel leaves the bits at or beyond max_doc 0)
  for (size_t i = 0; i < need; ++i) n_set += __builtin_popcountll(words[i]);
  drop_accept_sets(seg);   // the sets that were combined from the mask this one replaces
  seg->masks[mask_id] = std::move(words);
  if (out_count) *out_count = n_set;
  {   // what this call cost, for the calling thread (nrtgpu_last_diagnostics)
    nrtgpu_diagnostics diag{};
    diag.total_ms = now_ms() - t0;
    diag.device_ms = (double)kernel_ms;
    g_diag = diag;
  }
  return NRTGPU_OK;
}

}  // namespace

extern "C" int nrtgpu_segment_set_mask_from_values(nrtgpu_seg* seg, int32_t mask_id, const nrtgpu_value_clause* clauses, int32_t n_clauses,
                                                   int64_t* out_count) {
  if (!seg || !clauses) return fail(NRTGPU_ERR_INVALID_ARG, "NULL argument");
  if (mask_id <= 0) return fail(NRTGPU_ERR_INVALID_ARG, "mask id must be > 0, got %d", mask_id);
  if (n_clauses < 1 || n_clauses > NRTGPU_MAX_RANGES) return fail(NRTGPU_ERR_INVALID_ARG, "n_clauses %d outside 1..%d", n_clauses, NRTGPU_MAX_RANGES);
  for (int i = 0; i < n_clauses; ++i)
    if (int rc = check_clause(clauses[i], i)) return rc;
  const double t0 = now_ms();
  SegWriteLock content(seg);  // nrtgpu_segment_set_mask's: waits for the searches running over this segment; later ones wait for it
  if (!seg->sealed) return fail(NRTGPU_ERR_STATE, "segment is not sealed");

  // ---- the clauses over the leaf's resident columns; the IN_SET values as codes, sorted, without duplicates
  DValueClause records[kMaxRanges] = {};
  std::vector<uint32_t> sets;
  for (int i = 0; i < n_clauses; ++i) {
    const nrtgpu_value_clause& c = clauses[i];
    const auto fit = seg->fields.find(c.field_id);
    if (fit == seg->fields.end() || fit->second.dv_kind < 0)
      return fail(NRTGPU_ERR_UNSUPPORTED, "clause %d: the segment holds no doc values of field %d", i, c.field_id);
    const FieldData& f = fit->second;
    if (f.dv_kind >= kDocValuesInt64)
      return fail(NRTGPU_ERR_UNSUPPORTED, "clause %d: the doc values of field %d are a 64-bit column: build the mask with nrtgpu_segment_set_mask_from_values64", i,
                  c.field_id);
    DValueClause& r = records[i];
    r.code = f.d_dv_code;
    r.multi = f.d_dv_start != nullptr ? 1u : 0u;
    r.has = r.multi != 0u ? (const void*)f.d_dv_start : (const void*)f.d_dv_has;
    if (c.kind == NRTGPU_CLAUSE_RANGE) {
      r.lo_code = doc_value_code(f.dv_kind, c.lower_bits);
      r.hi_code = doc_value_code(f.dv_kind, c.upper_bits);
    } else if (c.kind == NRTGPU_CLAUSE_EXISTS) {   // the range of every code
      r.lo_code = 0u;
      r.hi_code = 0xFFFFFFFFu;
    } else {
      std::vector<uint32_t> codes((size_t)c.n_values);
      for (int32_t v = 0; v < c.n_values; ++v) codes[(size_t)v] = doc_value_code(f.dv_kind, c.value_bits[v]);
      std::sort(codes.begin(), codes.end());
      codes.erase(std::unique(codes.begin(), codes.end()), codes.end());
      r.set_off = (uint32_t)sets.size();
      r.set_len = (uint32_t)codes.size();
      r.lo_code = codes.front();
      r.hi_code = codes.back();
      sets.insert(sets.end(), codes.begin(), codes.end());
    }
  }

  return build_mask(seg, mask_id, records, sizeof(records), sets,
                    [&](const void* d_records, const uint32_t* d_sets, uint64_t* d_words, uint32_t n_words) {
                      launch_value_mask(nullptr, (const DValueClause*)d_records, (uint32_t)n_clauses, d_sets, (uint32_t)sets.size(), d_words, n_words,
                                        (uint32_t)seg->max_doc);
                    },
                    out_count, t0);
}

static_assert(sizeof(nrtgpu_value_clause64) == 32 && offsetof(nrtgpu_value_clause64, lower_bits) == 8 && offsetof(nrtgpu_value_clause64, reserved) == 24,
              "nrtgpu_value_clause64 layout");

extern "C" int nrtgpu_range_accepts64(int32_t kind, uint64_t lower_bits, uint64_t upper_bits, uint64_t value_bits, int32_t* out) {
  if (!out) return fail(NRTGPU_ERR_INVALID_ARG, "NULL argument");
  if (kind != NRTGPU_DOCVALUES_INT64 && kind != NRTGPU_DOCVALUES_FLOAT64) return fail(NRTGPU_ERR_INVALID_ARG, "64-bit doc values kind %d outside 2..3", kind);
  *out = range_accepts_code64(doc_value_code64(kind, lower_bits), doc_value_code64(kind, upper_bits), doc_value_code64(kind, value_bits)) ? 1 : 0;
  return NRTGPU_OK;
}

// The builder above over 64-bit columns: range and exists clauses (value_mask64_kernel), the same checks in the same order.
extern "C" int nrtgpu_segment_set_mask_from_values64(nrtgpu_seg* seg, int32_t mask_id, const nrtgpu_value_clause64* clauses, int32_t n_clauses,
                                                     int64_t* out_count) {
  if (!seg || !clauses) return fail(NRTGPU_ERR_INVALID_ARG, "NULL argument");
  if (mask_id <= 0) return fail(NRTGPU_ERR_INVALID_ARG, "mask id must be > 0, got %d", mask_id);
  if (n_clauses < 1 || n_clauses > NRTGPU_MAX_RANGES) return fail(NRTGPU_ERR_INVALID_ARG, "n_clauses %d outside 1..%d", n_clauses, NRTGPU_MAX_RANGES);
  for (int i = 0; i < n_clauses; ++i) {
    if (clauses[i].kind != NRTGPU_CLAUSE_RANGE && clauses[i].kind != NRTGPU_CLAUSE_EXISTS)
      return fail(NRTGPU_ERR_INVALID_ARG, "clause %d: kind %d outside 0..1 (a 64-bit clause is a range or an exists clause)", i, clauses[i].kind);
    if (clauses[i].reserved != 0) return fail(NRTGPU_ERR_INVALID_ARG, "clause %d: reserved must be 0", i);
  }
  const double t0 = now_ms();
  SegWriteLock content(seg);
  if (!seg->sealed) return fail(NRTGPU_ERR_STATE, "segment is not sealed");
  DValueClause64 records[kMaxRanges] = {};
  for (int i = 0; i < n_clauses; ++i) {
    const nrtgpu_value_clause64& c = clauses[i];
    const auto fit = seg->fields.find(c.field_id);
    if (fit == seg->fields.end() || fit->second.dv_kind < 0)
      return fail(NRTGPU_ERR_UNSUPPORTED, "clause %d: the segment holds no doc values of field %d", i, c.field_id);
    const FieldData& f = fit->second;
    if (f.dv_kind < kDocValuesInt64)
      return fail(NRTGPU_ERR_UNSUPPORTED, "clause %d: the doc values of field %d are a 32-bit column: build the mask with nrtgpu_segment_set_mask_from_values", i,
                  c.field_id);
    DValueClause64& r = records[i];
    r.code64 = f.d_dv_code64;
    r.has = f.d_dv_has;
    r.lo_code = c.kind == NRTGPU_CLAUSE_RANGE ? doc_value_code64(f.dv_kind, c.lower_bits) : 0ull;   // (exists: the range of every code)
    r.hi_code = c.kind == NRTGPU_CLAUSE_RANGE ? doc_value_code64(f.dv_kind, c.upper_bits) : ~0ull;
  }
  const std::vector<uint32_t> no_sets;
  return build_mask(seg, mask_id, records, sizeof(records), no_sets,
                    [&](const void* d_records, const uint32_t*, uint64_t* d_words, uint32_t n_words) {
                      launch_value_mask64(nullptr, (const DValueClause64*)d_records, (uint32_t)n_clauses, d_words, n_words, (uint32_t)seg->max_doc);
                    },
                    out_count, t0);
}

extern "C" int nrtgpu_segment_get_mask(const nrtgpu_seg* seg, int32_t mask_id, uint64_t* bits, int32_t n_words) {
  if (!seg || !bits) return fail(NRTGPU_ERR_INVALID_ARG, "NULL argument");
  if (mask_id <= 0) return fail(NRTGPU_ERR_INVALID_ARG, "mask id must be > 0, got %d", mask_id);
  const int32_t need = (seg->max_doc + 63) / 64;
  if (n_words < need) return fail(NRTGPU_ERR_INVALID_ARG, "mask %d: room for %d words, %d needed", mask_id, n_words, need);
  const nrtgpu_seg* held = seg;
  SegReadLocks content(&held, 1);   // (a set_mask on another thread does not rewrite the words under the copy)
  const auto m = seg->masks.find(mask_id);
  if (m == seg->masks.end()) return fail(NRTGPU_ERR_UNSUPPORTED, "mask %d is not resident on the segment", mask_id);
  memcpy(bits, m->second.data(), (size_t)need * 8);
  return NRTGPU_OK;
}
