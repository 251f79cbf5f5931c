// vectors.cpp -- exact vector search (the knn request path and ExactVectorQuery) and the vector rescorer.
#include "runtime_internal.h"

// ------------------------------------------------------------------------------------------------
// What the float and the byte entries share before anything is launched (runtime_internal.h): the checks, the accept table, the
// query statistics, turn-taking, the statistics and the unpacking
// ------------------------------------------------------------------------------------------------
int nrtgpu::rt::knn_check_scalars(bool bad_count, int32_t k, int32_t dim, int32_t sim, const float* byte_boost) {
  if (bad_count || k <= 0 || dim <= 0 || sim < 0 || sim > 3) return fail(NRTGPU_ERR_INVALID_ARG, "bad knn arguments");
  if (byte_boost)
    if (int rc = knn_check_byte_boost(*byte_boost)) return rc;
  if (k > NRTGPU_MAX_K) return fail(NRTGPU_ERR_UNSUPPORTED, "k %d > %d", k, NRTGPU_MAX_K);
  if (dim > 2048) return fail(NRTGPU_ERR_UNSUPPORTED, "vector dimension %d (device path takes <= 2048)", dim);
  return NRTGPU_OK;
}
int nrtgpu::rt::knn_check_byte_boost(float boost) {
  if (!(boost >= 0.0f) || !(boost < INFINITY)) return fail(NRTGPU_ERR_INVALID_ARG, "byte vector search: a finite boost >= 0 expected");
  return NRTGPU_OK;
}

int nrtgpu::rt::knn_check_field(bool bytes, int si, int32_t field_id, const FieldData& f, int32_t dim, const char* hint, bool* has_rows) {
  if (has_rows) *has_rows = false;
  if (!bytes) {
    if (f.byte_rows) return fail(NRTGPU_ERR_INVALID_ARG, "segment %d: field %d holds byte (int8) vectors: %s", si, field_id, hint);
    if (!f.d_vectors) return NRTGPU_OK;
  } else {
    if (!f.byte_rows && (f.d_vectors || f.dim > 0))
      return fail(NRTGPU_ERR_INVALID_ARG, "segment %d: field %d holds float (fp32) vectors: %s", si, field_id, hint);
    if (!f.byte_rows) return NRTGPU_OK;
  }
  if (dim != 0 && f.dim_user != dim)
    return fail(NRTGPU_ERR_INVALID_ARG, "segment %d: field %d has dimension %d, query has %d", si, field_id, f.dim_user, dim);
  if (has_rows) *has_rows = bytes ? (f.d_btiles && f.n_vec > 0) : true;
  return NRTGPU_OK;
}
int nrtgpu::rt::knn_check_leaves(const nrtgpu_seg* const* segs, int32_t n_segs, int32_t field_id, bool bytes, int32_t dim, const char* hint) {
  for (int si = 0; si < n_segs; ++si) {
    auto fit = segs[si]->fields.find(field_id);
    if (fit != segs[si]->fields.end())
      if (int rc = knn_check_field(bytes, si, field_id, fit->second, dim, hint)) return rc;
  }
  return NRTGPU_OK;
}

// (nrtgpu_search_hybrid_batch refuses byte fields itself, before it plans, and pads here afterwards: search.cpp)
int nrtgpu::rt::pad_query_vectors(const nrtgpu_seg* const* segs, int32_t n_segs, int32_t field_id, const float* queries, int32_t n,
                                  int32_t dim_user, PaddedQueries* out) {
  int32_t dim_dev = (dim_user + 15) & ~15;
  for (int si = 0; si < n_segs; ++si) {
    if (!segs[si]) continue;
    auto fit = segs[si]->fields.find(field_id);
    if (fit == segs[si]->fields.end()) continue;
    bool has_rows = false;
    if (int rc = knn_check_field(false, si, field_id, fit->second, dim_user, kHintSearchBytes, &has_rows)) return rc;
    if (has_rows) dim_dev = fit->second.dim;
  }
  out->dim = dim_dev;
  if (dim_dev == dim_user) {
    out->p = queries;
    return NRTGPU_OK;
  }
  out->buf.assign((size_t)n * (size_t)dim_dev, 0.0f);
  for (int32_t q = 0; q < n; ++q) memcpy(out->buf.data() + (size_t)q * dim_dev, queries + (size_t)q * dim_user, (size_t)dim_user * 4);
  out->p = out->buf.data();
  return NRTGPU_OK;
}

int nrtgpu::rt::knn_stage_accept_table(const KnnCall& c, int q0, int nq, const uint64_t** table) {
  memset(table, 0, (size_t)std::max(c.n_segs, 1) * kKnnAcceptCols * sizeof(uint64_t*));
  return knn_walk_leaves(c, -1, [&](const KnnLeaf& at) -> int {
    const uint64_t** row = table + (size_t)at.index * kKnnAcceptCols;
    for (int q = 0; q < nq; ++q) {
      const int32_t mask = c.ask.mask(q0 + q);
      row[q] = at.seg->d_live;
      if (mask == 0) continue;
      int same = -1;
      for (int p = 0; p < q && same < 0; ++p)
        if (c.ask.mask(q0 + p) == mask) same = p;
      if (same >= 0) row[q] = row[same];
      else if (int rc = accept_set_of(at.seg, mask, 0, &row[q])) return rc;
    }
    return NRTGPU_OK;
  });
}

// (0.11 ms -> 0.035 ms per 64-query panel of 768 dimensions against one query after the other: a pass's staging is host time no
// kernel runs under for one caller)
template <bool kAll>
static void query_stats_walk(const float* queries, int nq, int dim, float* norm2, float* max_abs, double* l1) {
  for (int qb = 0; qb < nq; qb += 8) {
    const int nb = std::min(8, nq - qb);
    float s2[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, mx[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    double a1[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const float* qv0 = queries + (size_t)qb * dim;
    {
#pragma clang fp contract(off)   // (x * x rounded, then added: never one fused operation, whatever the build's flags)
      auto walk = [&](const int n) {
        for (int d = 0; d < dim; ++d)
          for (int j = 0; j < n; ++j) {
            const float x = qv0[(size_t)j * dim + d];
            const float p2 = x * x;
            s2[j] = s2[j] + p2;
            if (kAll) {
              mx[j] = std::max(mx[j], std::fabs(x));
              a1[j] += std::fabs((double)x);
            }
          }
      };
      if (nb == 8) walk(8);   // (a constant trip count: unrolled, the eight sums in registers)
      else walk(nb);
    }
    for (int j = 0; j < nb; ++j) {
      norm2[qb + j] = s2[j];
      if (kAll) {
        max_abs[qb + j] = mx[j];
        l1[qb + j] = a1[j];
      }
    }
  }
}
void nrtgpu::rt::knn_query_stats(const float* queries, int nq, int dim, float* norm2, float* max_abs, double* l1) {
  if (max_abs && l1) query_stats_walk<true>(queries, nq, dim, norm2, max_abs, l1);
  else query_stats_walk<false>(queries, nq, dim, norm2, nullptr, nullptr);
}

int nrtgpu::rt::KnnRun::take_turn() {
  std::lock_guard<std::mutex> gpu(ctx->gpu_mu);
  if (ctx->last_turn) HIP_TRY(hipStreamWaitEvent(slot->stream, ctx->last_turn, 0));
  return NRTGPU_OK;
}
int nrtgpu::rt::KnnRun::end_turn() {
  std::lock_guard<std::mutex> gpu(ctx->gpu_mu);
  HIP_TRY(hipEventRecord(slot->ev_turn, slot->stream));
  ctx->last_knn_turn = slot->ev_turn;
  return NRTGPU_OK;
}
void nrtgpu::rt::KnnRun::add_stats(int64_t rows, int64_t sketch_launches, bool second_pass) {
  double ms = 0.0;
  for (size_t i = 0; i + 1 < n_ev; i += 2) {
    float one = 0.f;
    (void)hipEventElapsedTime(&one, slot->round_ev[i], slot->round_ev[i + 1]);
    ms += (double)one;
  }
  std::lock_guard<std::mutex> lk(ctx->stats_mu);
  ctx->stats.knn_panels += 1;
  ctx->stats.knn_score_launches += (int64_t)(n_ev / 2);
  ctx->stats.knn_score_ms += ms;
  ctx->stats.knn_rows += rows;
  ctx->stats.knn_second_passes += second_pass ? 1 : 0;
  ctx->stats.knn_sketch_launches += sketch_launches;
  n_ev = 0;
}
void nrtgpu::rt::knn_unpack_topdocs(const uint64_t* keys, const uint32_t* counts, uint32_t k_stride, int nq, bool clamp_to_k, int64_t total,
                                    bool knn_request, const KnnAsk& ask, nrtgpu_topdocs* out) {
  for (int q = 0; q < nq; ++q) {
    nrtgpu_topdocs* o = &out[q];
    // (a member of a pass searched with the largest k of its members takes the first k of its own: a prefix of a sorted list)
    const int32_t k = ask.k(q);
    const float boost = ask.boost(q);
    const int32_t cap = o->capacity > 0 ? o->capacity : k;
    const int32_t m = std::min<int32_t>((int32_t)(clamp_to_k || ask.stride ? std::min<uint32_t>(counts[q], (uint32_t)k) : counts[q]), cap);
    for (int32_t i = 0; i < m; ++i) {
      if (o->docs) o->docs[i] = (int32_t)key_doc(keys[(size_t)q * k_stride + i]);
      if (o->scores) o->scores[i] = key_score(keys[(size_t)q * k_stride + i]);
    }
    o->n_hits = m;
    o->total_hits = total;   // every live doc with a vector matches an exact vector query
    o->total_hits_is_lower_bound = 0;
    if (knn_request) {
      o->total_hits = m;  // the rewritten knn query matches exactly the docs it returns
      if (boost != 1.0f && o->scores) {
        for (int32_t i = 0; i < m; ++i) o->scores[i] = o->scores[i] * boost;
        // distinct scores can round to one product: restore (score desc, doc asc) among equals
        if (o->docs)
          for (int32_t i = 1; i < m; ++i)
            for (int32_t j = i; j > 0 && o->scores[j - 1] == o->scores[j] && o->docs[j - 1] > o->docs[j]; --j) std::swap(o->docs[j - 1], o->docs[j]);
      }
    }
  }
}

float nrtgpu::rt::float_qnorm2(const float* q, int dim) {
  float qn = 0.f;
  for (int d = 0; d < dim; ++d) {
    volatile float p2 = q[d] * q[d];   // (rounded, then added: no build flag can fuse the two)
    qn = qn + p2;
  }
  return qn;
}

// A slot of the rescoring kernels' leaf table: DVecSeg and DByteVecSeg (plan.h) are this layout with their own pointer types.
struct VecLeafSlot {
  const void *rows, *vnorm2;
  const int32_t* ord_to_doc;
  int32_t doc_base, max_doc, n_vec, pad;
};
#define SAME_SLOT(m) (offsetof(VecLeafSlot, m) == offsetof(DVecSeg, m) && offsetof(VecLeafSlot, m) == offsetof(DByteVecSeg, m))
static_assert(sizeof(VecLeafSlot) == sizeof(DVecSeg) && sizeof(VecLeafSlot) == sizeof(DByteVecSeg), "one leaf table slot serves both element types");
static_assert(offsetof(VecLeafSlot, rows) == offsetof(DVecSeg, vecs) && offsetof(VecLeafSlot, rows) == offsetof(DByteVecSeg, tiles) &&
              SAME_SLOT(vnorm2) && SAME_SLOT(ord_to_doc) && SAME_SLOT(doc_base) && SAME_SLOT(max_doc) &&
              SAME_SLOT(n_vec), "leaf table layout");
#undef SAME_SLOT

int nrtgpu::rt::stage_rescore_inputs(const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs, int32_t field_id, bool bytes,
                                     int32_t sim, const void* queries, int32_t n, int32_t dim, void* leaves, void* staged, void* qnorm2) {
  for (int si = 0; leaves && si < n_segs; ++si) {
    VecLeafSlot v{};
    auto fit = segs[si]->fields.find(field_id);
    if (fit != segs[si]->fields.end()) {
      const FieldData& f = fit->second;
      if (bytes ? (f.byte_rows && f.d_btiles && f.n_vec > 0) : f.d_vectors != nullptr) {
        v.rows = bytes ? f.d_btiles : (const void*)f.d_vectors;
        v.vnorm2 = bytes ? (const void*)f.d_bnorm2 : (const void*)f.d_vnorm2;
        v.ord_to_doc = f.d_ord_to_doc;
        v.n_vec = f.n_vec;
      }
    }
    v.doc_base = doc_bases ? doc_bases[si] : 0;
    v.max_doc = segs[si]->max_doc;
    memcpy((char*)leaves + (size_t)si * sizeof v, &v, sizeof v);
  }
  if (bytes) return byte_queries_stage((const int8_t*)queries, n, dim, sim, (int8_t*)staged, (int32_t*)qnorm2);
  if (staged) memcpy(staged, queries, (size_t)n * (size_t)dim * 4);
  for (int32_t q = 0; qnorm2 && q < n; ++q) ((float*)qnorm2)[q] = float_qnorm2((const float*)queries + (size_t)q * dim, dim);
  return NRTGPU_OK;
}

// ------------------------------------------------------------------------------------------------
// The element type of a vector entry.  The request and the coalesced entries over float fields and their twins over byte (int8)
// fields are ONE code further down -- the checks, the passes, the panels -- handed the kind, as the rescorers are handed a
// RescoreKind (runtime_internal.h); what a kind brings is its search (knn_search here, knn_bytes_search in vectors_bytes.cpp), its
// refusals of the other element type, and the panels that fit its kernel's LDS.
// ------------------------------------------------------------------------------------------------
struct KnnKind {
  bool bytes;         // int8 rows and queries; else fp32
  size_t elem_size;   // bytes of a query element
  const char* other_type_hint;   // where the other element type's fields are searched (knn_check_field)
  // queries per pass over the rows: 160 KB of LDS hold the float search's two 16-query panels up to 1280 dimensions, beyond that
  // one panel (16 queries per pass) up to 2048; the byte search's four panels of 16 fit at every dimension
  int32_t pass_q(int32_t dim) const { return !bytes && dim > 1280 ? 16 : kKnnMaxQ; }
  int search(nrtgpu_ctx* ctx, const KnnCall& call) const { return bytes ? knn_bytes_search(ctx, call) : knn_search(ctx, call); }
};
static const KnnKind kKnnFloat{false, 4, kHintSearchBytes}, kKnnBytes{true, 1, kHintSearchFloat};

// ------------------------------------------------------------------------------------------------
// The exact search over float rows
// ------------------------------------------------------------------------------------------------
// The workspace of a float search (the slot's d_work): offsets, built here and nowhere else.  The panel's inputs are staged in
// pinned memory laid out like the head [o_q, o_th): two copies per panel, no sync.  The answer, its counts, the certificates and
// the overflow flag come back into h_out at 0, oh_cnt, oh_cert, oh_ov.
struct KnnLayout {
  uint32_t k_stride, k_int, ki_stride;
  size_t o_q, o_qn, o_eb, o_eb16, o_qs, o_segs, o_leaves, o_ms, o_acc, o_th, o_tk, o_tc, o_cc, o_xk, o_xc, o_cert, o_ov, o_p16, o_cd, size;
  size_t oh_cnt, oh_cert, oh_ov;
  KnnLayout(int32_t dim, int32_t n_segs, int32_t k, bool table) {
    k_stride = round_up((uint32_t)k, 16);
    // The matrix-core pass NOMINATES: it keeps the k_int best rows by its estimate of the score (an fp32 fma chain in the
    // MFMA's order, |q|^2 + |v|^2 - 2 q.v for EUCLIDEAN).  The answer is the top k of the nominations rescored in the
    // oracle's order (knn_score_seq), certified against the rows left outside (knn.hip: knn_select_kernel<true>).
    k_int = std::min<uint32_t>((uint32_t)NRTGPU_MAX_K, (uint32_t)k + std::max<uint32_t>(32u, (uint32_t)k / 2u));
    ki_stride = round_up(k_int, 16);
    const size_t leaves = (size_t)std::max(n_segs, 1);
    Carver wc;
    o_q = wc.take((size_t)kKnnMaxQ * dim * 4), o_qn = wc.take(kKnnMaxQ * 4), o_eb = wc.take(kKnnMaxQ * 4);
    o_eb16 = wc.take(kKnnMaxQ * 4), o_qs = wc.take(kKnnMaxQ * 4);
    o_segs = wc.take(leaves * sizeof(DVecSeg));     // the leaves' vector matrices, for docid -> row on the device (the rescoring reads rows by docid)
    o_leaves = wc.take(leaves * sizeof(DKnnLeaf));   // the sketch kernel's leaf table (plan.h)
    o_ms = wc.take(kKnnMaxQ * 4);   // the queries' thresholds on the unboosted score (0: none)
    o_acc = wc.take(table ? leaves * kKnnAcceptCols * sizeof(uint64_t*) : 8);   // the accept table (plan.h)
    o_th = wc.take(kKnnMaxQ * 8);
    o_tk = wc.take((size_t)kKnnMaxQ * ki_stride * 8), o_tc = wc.take(kKnnMaxQ * 4);
    o_cc = wc.take(kKnnMaxQ * 4), o_xk = wc.take((size_t)kKnnMaxQ * k_stride * 8);
    o_xc = wc.take(kKnnMaxQ * 4), o_cert = wc.take(kKnnMaxQ * 4), o_ov = wc.take(64);   // (fetched in one copy)
    o_p16 = wc.take(160 * 1024);   // the panel in fp16, the sketch kernel's operand order (knn_panel_fp16_kernel)
    o_cd = wc.take((size_t)kKnnMaxQ * kKnnCap * 8);
    size = wc.off;
    oh_cnt = (size_t)kKnnMaxQ * k_stride * 8, oh_cert = oh_cnt + (o_cert - o_xc), oh_ov = oh_cnt + (o_ov - o_xc);
  }
};

// One float search on its slot: what the call fixes (the leaves' tables and statistics), then pass after pass of up to pass_q
// queries -- staged, nominated from the fp16 sketch or the fp32 rows, rescored, certified, and the uncertified answered by a
// second pass.
struct KnnFloatSearch {
  nrtgpu_ctx* ctx;
  const KnnCall& call;   // (the queries padded to the RESIDENT dimension, call.dim)
  Slot* slot;
  const int32_t k;       // the largest of the call
  const KnnLayout L;
  KnnRun run{ctx, slot};   // (the turns on the device and what they order: runtime_internal.h)
  hipStream_t st = slot->stream;
  const bool table = !call.one_filter();
  const int32_t dim = call.dim, sim = call.sim, n_segs = call.n_segs;
  const float score_boost = call.score_boost(), erel = hostmath::knn_e_rel();
  char *wb = nullptr, *ho = nullptr, *hs = nullptr;
  // the leaves
  int32_t n_kleaves = 0;
  int64_t total_tiles = 0, total_rows = 0, live_vectors = 0;
  double nv_max = 0.0, nv_min = INFINITY, rows_unit = 0.0;   // rows_unit: the largest 1 / scale of the leaves' sketches
  bool sketch_ok = false;
  // the pass under way
  int q0 = 0, nq = 0;
  bool panel_sketch = false;
  int64_t total_vec = 0, rows_scored = 0, sketch_launches = 0;
  float q_max_of[kKnnMaxQ];
  double q_l1_of[kKnnMaxQ];

  float* staged(size_t off) const { return (float*)(hs + off); }
  const uint32_t* certified() const { return (const uint32_t*)(ho + L.oh_cert); }
  const uint32_t* overflow() const { return (const uint32_t*)(ho + L.oh_ov); }
  const uint64_t* const* d_acc() const { return table ? (const uint64_t* const*)(wb + L.o_acc) : nullptr; }

  int reserve();
  int stage_leaves(int pass_q);
  void stage_bounds();
  int stage_pass();
  void select();
  void refine(size_t o_list, size_t o_cnt, uint32_t cap, size_t o_bound, int32_t certify);
  int rows_pass(bool nominate, int safe);
  int sketch_pass(int safe, bool nominate);
  int fetch();
  int first_stage(int safe);
  void second_theta(const float* bound, std::vector<uint64_t>& th2);
  int second_pass(bool from_sketch, int safe, const std::vector<uint64_t>& th2);
  int second_stage();
  int deliver();
  int pass(int q0_, int nq_);
};

int KnnFloatSearch::reserve() {
  if (int rc = slot->d_work.reserve(L.size)) return rc;
  if (int rc = slot->h_out.reserve(L.oh_ov + 64)) return rc;
  if (int rc = slot->h_aux.reserve(L.o_th)) return rc;
  wb = (char*)slot->d_work.p;
  ho = (char*)slot->h_out.p;
  hs = (char*)slot->h_aux.p;
  return NRTGPU_OK;
}

// The leaf tables (the rescoring kernel's and the sketch kernel's view of the same leaves: ONE launch walks them all, tiles of 16
// rows numbered through the leaves) and what the bounds want of the rows.
int KnnFloatSearch::stage_leaves(int pass_q) {
  (void)stage_rescore_inputs(call.segs, call.doc_bases, n_segs, call.field_id, false, sim, nullptr, 0, dim, hs + L.o_segs, nullptr, nullptr);
  DKnnLeaf* hleaves = (DKnnLeaf*)(hs + L.o_leaves);
  bool all_sketched = true;
  if (int rc = knn_walk_leaves(call, call.shared_mask(), [&](const KnnLeaf& at) -> int {
        const FieldData& f = *at.f;
        nv_max = std::max(nv_max, (double)f.vnorm2_max);
        if (!f.d_sketch) all_sketched = false;
        if (f.vnorm2_min > 0.f) nv_min = std::min(nv_min, (double)f.vnorm2_min);
        rows_unit = std::max(rows_unit, 1.0 / (double)f.sketch_scale);
        DKnnLeaf l{};
        l.sketch = f.d_sketch;
        l.vnorm2 = f.d_vnorm2;
        l.ord_to_doc = f.d_ord_to_doc;
        l.accept = at.accept;
        l.accept_of = table ? d_acc() + (size_t)at.index * kKnnAcceptCols : nullptr;
        l.tile_begin = at.tile_begin;
        l.n_rows = f.n_vec;
        l.doc_base = at.doc_base;
        l.inv_rows_scale = 1.0f / f.sketch_scale;
        hleaves[n_kleaves++] = l;
        live_vectors += at.live;
        total_tiles = at.tile_begin + (((int64_t)f.n_vec + 15) >> 4);
        total_rows = at.row_begin + f.n_vec;
        return NRTGPU_OK;
      }))
    return rc;
  // (the query panel in fp16 and at least a small nomination queue behind it must fit the CU's 160 KB of LDS)
  sketch_ok = all_sketched && n_kleaves > 0 && std::isfinite(nv_max) && knn_sketch_fits(dim, std::min(call.n_queries, pass_q));
  return NRTGPU_OK;
}

// |estimate - result| <= E, the e_abs of plan.h's knn_result_upper / knn_estimate_lower, and the scale of the fp16 panel, per query
// of the pass: host_math.h states the bounds (knn_bound32 for an fp32 estimate in the MFMA's order, knn_bound16 for the fp16
// sketch's) and DESIGN §4.5 derives the constants.
void KnnFloatSearch::stage_bounds() {
  const float* qn = staged(L.o_qn);
  float *eb = staged(L.o_eb), *eb16 = staged(L.o_eb16), *qsc = staged(L.o_qs);
  for (int q = 0; q < nq; ++q) {
    eb[q] = hostmath::knn_bound32(sim, dim, (double)qn[q], nv_max, (double)score_boost);
    // the scaled query's largest |element| is below 2^14; a query too small for such a scale (or not finite) sends the panel
    // to the fp32 rows
    const bool q_scaled = hostmath::knn_sketch_scale(q_max_of[q], &qsc[q]);
    eb16[q] = hostmath::knn_bound16(sim, dim, (double)qn[q], q_l1_of[q], 1.0 / (double)qsc[q], nv_max, nv_min, rows_unit, (double)score_boost);
    if (!q_scaled || !std::isfinite(eb16[q])) panel_sketch = false;
  }
}

// The pass's inputs into the pinned head and from there to the device.
int KnnFloatSearch::stage_pass() {
  // nominate from the sketch unless it failed to certify lately for this similarity (then: a few panels straight from fp32)
  panel_sketch = sketch_ok;
  if (panel_sketch && ctx->knn_sketch_skip[sim].load(std::memory_order_relaxed) > 0) {
    ctx->knn_sketch_skip[sim].fetch_sub(1, std::memory_order_relaxed);
    panel_sketch = false;
  }
  const float* queries = (const float*)call.queries + (size_t)q0 * dim;
  knn_query_stats(queries, nq, dim, staged(L.o_qn), q_max_of, q_l1_of);
  stage_bounds();
  float* ms = staged(L.o_ms);
  for (int q = 0; q < kKnnMaxQ; ++q) ms[q] = q < nq ? call.ask.min_score(q0 + q) : 0.0f;
  if (table)   // liveDocs & the member's filter per (leaf, member)
    if (int rc = knn_stage_accept_table(call, q0, nq, (const uint64_t**)(hs + L.o_acc))) return rc;
  memcpy(hs + L.o_q, queries, (size_t)nq * dim * 4);
  HIP_TRY(hipMemcpyAsync(wb + L.o_q, hs + L.o_q, (size_t)nq * dim * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(wb + L.o_qn, hs + L.o_qn, L.o_th - L.o_qn, hipMemcpyHostToDevice, st));   // |q|^2, bounds, scales, leaf table
  return NRTGPU_OK;
}

void KnnFloatSearch::select() {   // the candidates into the running top-k_int, theta tightened
  launch_knn_select(st, (uint32_t)nq, (uint64_t*)(wb + L.o_tk), (uint32_t*)(wb + L.o_tc), L.ki_stride, L.k_int, (const uint64_t*)(wb + L.o_cd),
                    (uint32_t*)(wb + L.o_cc), kKnnCap, (unsigned long long*)(wb + L.o_th), (uint32_t*)(wb + L.o_ov));
}
void KnnFloatSearch::refine(size_t o_list, size_t o_cnt, uint32_t cap, size_t o_bound, int32_t certify) {   // a list rescored into the answer
  launch_knn_refine_select(st, (uint32_t)nq, (uint64_t*)(wb + L.o_xk), (uint32_t*)(wb + L.o_xc), L.k_stride, (uint32_t)k,
                           (const uint64_t*)(wb + o_list), (uint32_t*)(wb + o_cnt), cap, (unsigned long long*)(wb + L.o_th),
                           (uint32_t*)(wb + L.o_ov), (const DVecSeg*)(wb + L.o_segs), n_segs, dim, sim, (const float*)(wb + L.o_q),
                           (const float*)(wb + L.o_qn), score_boost, (const float*)(wb + o_bound), erel, (const float*)(wb + L.o_ms),
                           L.k_int, certify, (uint32_t*)(wb + L.o_cert));
}

// Rows are scored in rounds with a selection in between (theta tightens from round to round).  The first round of
// a panel gives every row a slot of the candidate list; later rounds only append rows that beat theta, so they can
// be long: with rows in no particular order a round that multiplies the rows seen by 16 appends about
// k * ln 16 candidates.  Rows ordered by rising similarity could overflow the list (every row beats theta): the
// select kernel flags that and the panel is redone with rounds no longer than the list (`safe`).
// (rows of the first round: every row takes a slot of the list and the first selection scans them all)
static const int64_t kKnnFirstRound = []() { const long v = dev_env_int("NRTGPU_KNN_FIRST_ROUND", 0); return (int64_t)(v >= 1024 && v <= (1 << 18) ? (v & ~15L) : (1 << 16)); }();

// One pass over the fp32 rows of every leaf, a launch per leaf and round.  nominate: the estimates' running top-k_int, theta
// tightening (knn_select_kernel<false>); else theta stays what the certification left and every nomination is rescored into the
// answer (<true>).
int KnnFloatSearch::rows_pass(bool nominate, int safe) {
  int64_t seen = 0, round = kKnnFirstRound;
  // Nominating, theta tightens fast: after two selections (>= 1M rows seen) a later launch appends about k ln(rows / rows
  // seen) keys per query, so the remaining launches run back to back (append_only) and ONE selection closes the pass.  A
  // theta still unknown then (hardly any live row) makes those launches append every live row: the list overflows, the
  // flag is raised and the panel is redone in bounded rounds with a selection after each.
  int selections = 0;
  bool pending = false;
  total_vec = 0;
  if (int rc = knn_walk_leaves(call, call.shared_mask(), [&](const KnnLeaf& at) -> int {
        const FieldData& f = *at.f;
        total_vec += at.live;
        const uint64_t* const* leaf_acc = table ? d_acc() + (size_t)at.index * kKnnAcceptCols : nullptr;
        // rounds never exceed the candidate capacity, so a list cannot overflow; theta tightens between rounds
        int64_t r = 0;
        if (seen == 0) round = kKnnFirstRound;
        while (r < f.n_vec) {
          const int64_t rb = r;
          int64_t len = (safe || (nominate && seen == 0)) ? std::min<int64_t>(round, kKnnCap) : round;
          if (!nominate && !safe) len = f.n_vec;   // theta is fixed and tight: the whole leaf at once
          const int64_t re = std::min<int64_t>(f.n_vec, (r + len + 15) & ~(int64_t)15);   // rounds begin on tile boundaries (16 rows)
          uint32_t blocks = (uint32_t)std::min<int64_t>((re - r + 255) / 256, (int64_t)std::max(ctx->n_cus, 1));  // 256 rows per workgroup step
          if (nq > 32) blocks = std::max(16u, std::min((uint32_t)std::max(ctx->n_cus, 16), 2u * blocks) / 16u * 16u);   // paired workgroups
          const bool defer = nominate && !safe && selections >= 2;
          if (int rc = run.timed_launch("knn_score", [&]() {
                return launch_knn_score(st, blocks, f.d_vectors, f.d_vnorm2, f.d_ord_to_doc, at.accept, dim, r, re, at.doc_base,
                                        (const float*)(wb + L.o_q), (const float*)(wb + L.o_qn), nq, sim, score_boost,
                                        (const unsigned long long*)(wb + L.o_th), (uint64_t*)(wb + L.o_cd), (uint32_t*)(wb + L.o_cc), kKnnCap,
                                        defer ? 1 : 0, leaf_acc);
              }))
            return rc;
          if (defer) {
            pending = true;
          } else if (nominate) {
            select();
            ++selections;
          } else
            refine(L.o_cd, L.o_cc, kKnnCap, L.o_eb, 0);
          r = re;
          seen += re - rb;
          round = safe ? std::min<int64_t>(round * 4, kKnnCap) : std::min<int64_t>(seen * 15, (int64_t)1 << 40);
        }
        return NRTGPU_OK;
      }))
    return rc;
  if (pending) select();
  rows_scored += seen;
  return NRTGPU_OK;
}

// The same from the fp16 sketch: a round is a range of the leaves' tiles, ONE launch whatever the number of leaves it crosses.
// nominate = false: theta is fixed, every nomination is rescored into the answer.
int KnnFloatSearch::sketch_pass(int safe, bool nominate) {
  total_vec = live_vectors;
  auto launch = [&](int64_t t, int64_t te, uint32_t blocks, int32_t append_only) -> int {
    if (int rc = run.timed_launch("knn_sketch", [&]() {
          return launch_knn_sketch(st, blocks, (const DKnnLeaf*)(wb + L.o_leaves), n_kleaves, dim, t, te, (const void*)(wb + L.o_p16),
                                   (const float*)(wb + L.o_qn), (const float*)(wb + L.o_qs), nq, sim, score_boost,
                                   (const unsigned long long*)(wb + L.o_th), (uint64_t*)(wb + L.o_cd), (uint32_t*)(wb + L.o_cc), kKnnCap, append_only);
        }))
      return rc;
    ++sketch_launches;
    return NRTGPU_OK;
  };
  if (int rc = run.tile_rounds(total_tiles, kKnnFirstRound >> 4, kKnnCap, nominate, safe, launch, [&]() {
        if (nominate) select();
        else refine(L.o_cd, L.o_cc, kKnnCap, L.o_eb16, 0);
      }))
    return rc;
  rows_scored += total_rows;
  return NRTGPU_OK;
}

int KnnFloatSearch::fetch() {   // the answer so far + the flags
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(ho, wb + L.o_xk, (size_t)nq * L.k_stride * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(ho + L.oh_cnt, wb + L.o_xc, L.o_ov + 4 - L.o_xc, hipMemcpyDeviceToHost, st));   // counts, flags, overflow: one copy
  HIP_TRY(hipStreamSynchronize(st));
  return NRTGPU_OK;
}

// 1. nominate, rescore the nominations, certify
int KnnFloatSearch::first_stage(int safe) {
  const float *ms = staged(L.o_ms), *bound = staged(panel_sketch ? L.o_eb16 : L.o_eb);
  if (int rc = run.take_turn()) return rc;
  HIP_TRY(hipMemsetAsync(wb + L.o_th, 0, L.o_cd - L.o_th, st));  // theta, lists, counters
  if (std::any_of(ms, ms + nq, [](float v) { return v > 0.0f; })) {  // start theta below the lowest key whose RESULT can still reach the query's min_score
    std::vector<uint64_t> th0((size_t)nq, 0ull);
    for (int q = 0; q < nq; ++q) {
      if (!(ms[q] > 0.0f)) continue;
      const float lo = (float)knn_estimate_lower(sim, (double)ms[q], (double)bound[q], (double)erel, 1.0);
      th0[(size_t)q] = lo > 0.0f ? pack_key(lo, 0xFFFFFFFFu) - 1ull : 0ull;
    }
    HIP_TRY(hipMemcpyAsync(wb + L.o_th, th0.data(), (size_t)nq * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));  // th0 is a stack vector
  }
  if (panel_sketch) launch_knn_panel_fp16(st, (const float*)(wb + L.o_q), (const float*)(wb + L.o_qs), dim, nq, wb + L.o_p16);
  if (int rc = panel_sketch ? sketch_pass(safe, true) : rows_pass(true, safe)) return rc;
  refine(L.o_tk, L.o_tc, L.ki_stride, panel_sketch ? L.o_eb16 : L.o_eb, 1);
  if (int rc = run.end_turn()) return rc;
  return fetch();
}

// a row of the answer scores >= the k-th rescored score known so far (or >= min_score while fewer than k are known): the
// lowest key its estimate can carry; certified queries nominate nothing (theta = ~0)
void KnnFloatSearch::second_theta(const float* bound, std::vector<uint64_t>& th2) {
  th2.assign((size_t)nq, ~0ull);
  const uint64_t* xk = (const uint64_t*)ho;
  const uint32_t* xc = (const uint32_t*)(ho + L.oh_cnt);
  const float* ms = staged(L.o_ms);
  for (int q = 0; q < nq; ++q) {
    if (certified()[q] != 0u) continue;
    const double base = xc[q] >= (uint32_t)k ? (double)key_score(xk[(size_t)q * L.k_stride + (size_t)k - 1]) : (double)ms[q];
    const float lo = (float)knn_estimate_lower(sim, base, (double)bound[q], (double)erel, (double)score_boost);
    th2[(size_t)q] = lo > 0.0f ? pack_key(lo, 0xFFFFFFFFu) - 1ull : 0ull;
  }
}
int KnnFloatSearch::second_pass(bool from_sketch, int safe, const std::vector<uint64_t>& th2) {
  if (int rc = run.take_turn()) return rc;
  HIP_TRY(hipMemcpyAsync(wb + L.o_th, th2.data(), (size_t)nq * 8, hipMemcpyHostToDevice, st));
  for (int q = 0; q < nq; ++q)   // their answers start over (a nomination found again must not be counted twice)
    if (certified()[q] == 0u) HIP_TRY(hipMemsetAsync(wb + L.o_xc + (size_t)q * 4, 0, 4, st));
  HIP_TRY(hipMemsetAsync(wb + L.o_cc, 0, kKnnMaxQ * 4, st));
  HIP_TRY(hipMemsetAsync(wb + L.o_ov, 0, 4, st));
  if (int rc = from_sketch ? sketch_pass(safe, false) : rows_pass(false, safe)) return rc;
  if (int rc = run.end_turn()) return rc;
  return fetch();   // (the second pass leaves the flags as they are)
}
// 2. queries whose answer the nominations do not certify (rows outside the list within the rounding bound of the k-th
//    result: near-duplicates, or k at the list's capacity): a second pass nominates every row whose estimate is within
//    the bound of the k-th rescored score, and rescores all of them.
// Where: first the sketch again (half the bytes; its bound is wider, so more rows are nominated -- all of them are rescored,
// which costs nothing much while they are thousands); if that overflows a list -- the bound reaches down to rows by the
// hundred thousand: large norms against small distances -- the fp32 rows with their tight bound, and the next panels of this
// similarity go there directly.
int KnnFloatSearch::second_stage() {
  std::vector<uint64_t> th2;
  bool done = false;
  if (panel_sketch) {
    const std::vector<uint32_t> cert0(certified(), certified() + nq);
    const std::vector<uint64_t> xk0((const uint64_t*)ho, (const uint64_t*)ho + (size_t)nq * L.k_stride);
    const std::vector<uint32_t> xc0((const uint32_t*)(ho + L.oh_cnt), (const uint32_t*)(ho + L.oh_cnt) + nq);
    second_theta(staged(L.o_eb16), th2);
    if (int rc = second_pass(true, 0, th2)) return rc;
    done = *overflow() == 0u;
    if (!done) {   // back to what the first stage left (the flags are untouched on the device; the host's copies are restored)
      memcpy(ho, xk0.data(), xk0.size() * 8);
      memcpy(ho + L.oh_cnt, xc0.data(), xc0.size() * 4);
      memcpy(ho + L.oh_cert, cert0.data(), cert0.size() * 4);
      ctx->knn_sketch_skip[sim].store(16, std::memory_order_relaxed);
    }
  }
  if (done) return NRTGPU_OK;
  second_theta(staged(L.o_eb), th2);
  return run.redo_on_overflow(overflow(), "knn: candidate list overflow in a bounded round", [&](int safe) { return second_pass(false, safe, th2); });
}

int KnnFloatSearch::deliver() {
  if (!call.ext_keys) {
    knn_unpack_topdocs((const uint64_t*)ho, (const uint32_t*)(ho + L.oh_cnt), L.k_stride, nq, false, total_vec, call.knn_request, call.ask.from(q0),
                       &call.out[q0]);
    return NRTGPU_OK;
  }
  // stays in HBM: what nrtgpu_dist_knn_exact exchanges
  std::vector<uint64_t> tv((size_t)nq, (uint64_t)total_vec);
  HIP_TRY(hipMemcpyAsync(call.ext_keys + (size_t)q0 * L.k_stride * 8, wb + L.o_xk, (size_t)nq * L.k_stride * 8, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(call.ext_cnts + (size_t)q0 * 4, wb + L.o_xc, (size_t)nq * 4, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(call.ext_hits + (size_t)q0 * 8, tv.data(), (size_t)nq * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));   // (tv is a stack vector; the workspace is reused by the next panel)
  return NRTGPU_OK;
}

int KnnFloatSearch::pass(int q0_, int nq_) {
  q0 = q0_, nq = nq_;
  total_vec = rows_scored = sketch_launches = 0;
  if (int rc = stage_pass()) return rc;
  if (int rc = run.take_turn()) return rc;   // (the staging above and its copies are not part of the turn)
  if (int rc = run.redo_on_overflow(overflow(), "knn: candidate list overflow in a bounded round", [&](int safe) { return first_stage(safe); })) return rc;
  int uncertified = 0;
  for (int q = 0; q < nq; ++q) uncertified += certified()[q] == 0u;
  if (uncertified)
    if (int rc = second_stage()) return rc;
  run.add_stats(rows_scored, sketch_launches, uncertified != 0);
  return deliver();
}

int nrtgpu::rt::knn_search(nrtgpu_ctx* ctx, const KnnCall& user) {
  forget_foreign_hip_error();
  const nrtgpu_seg* const* segs = user.segs;
  const int32_t n_segs = user.n_segs, n_queries = user.n_queries;
  if (!ctx || !user.queries || (!user.out && !user.ext_keys) || (n_segs > 0 && !segs)) return fail(NRTGPU_ERR_INVALID_ARG, "NULL argument");
  const int32_t k = user.k_max();
  if (int rc = knn_check_scalars(n_queries <= 0, k, user.dim, user.sim)) return rc;
  NRT_CHECK_DEADLINE("before the vector search started");
  HIP_TRY(hipSetDevice(ctx->device));
  for (int si = 0; si < n_segs; ++si)
    if (!segs[si]) return fail(NRTGPU_ERR_STATE, "segment %d missing or not sealed", si);
  SegReadLocks content(segs, n_segs);  // liveDocs / masks stay as they are until the kernels have finished
  for (int si = 0; si < n_segs; ++si)
    if (!segs[si] || !segs[si]->sealed) return fail(NRTGPU_ERR_STATE, "segment %d missing or not sealed", si);
  // from here on the call's `dim` is the RESIDENT dimension (a multiple of 16) and the queries are padded like the rows
  PaddedQueries padded;
  if (int rc = pad_query_vectors(segs, n_segs, user.field_id, (const float*)user.queries, n_queries, user.dim, &padded)) return rc;
  KnnCall call = user;
  call.queries = padded.p;
  call.dim = padded.dim;
  if (call.shared_mask() != 0) {   // a selective filter: score only the rows it accepts (vectors_gather.cpp) -- no sketch is built or read
    bool gather = false;
    int64_t estimate = 0;
    if (int rc = knn_gather_route(ctx, call, &gather, &estimate)) return rc;
    if (gather) return knn_gather_run(ctx, call, nullptr, estimate);
  }
  for (int si = 0; si < n_segs; ++si)   // the fp16 sketches this search nominates from: built on a field's first exact search
    if (int rc = ensure_vector_sketch(segs[si], call.field_id)) return rc;
  Slot* slot = nullptr;
  acquire_slot(ctx, &slot);
  SlotGuard guard{ctx, slot};
  KnnFloatSearch s{ctx, call, slot, k, KnnLayout(call.dim, n_segs, k, !call.one_filter())};
  const int pass_q = kKnnFloat.pass_q(call.dim);
  if (int rc = s.reserve()) return rc;
  if (int rc = s.stage_leaves(pass_q)) return rc;
  for (int q0 = 0; q0 < n_queries; q0 += pass_q) {
    if (deadline_passed(g_deadline_ns)) {   // between two passes over the rows: nothing of the next one has been launched
      (void)hipStreamSynchronize(s.st);
      return fail(NRTGPU_ERR_TIMEOUT, "deadline passed between two passes over the rows (%d of %d queries answered)", q0, n_queries);
    }
    if (int rc = s.pass(q0, std::min(pass_q, n_queries - q0))) return rc;
  }
  return NRTGPU_OK;
}

int nrtgpu::rt::knn_exact_device(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs, int32_t field_id,
                                 int32_t sim, const float* queries, int32_t n_queries, int32_t dim, int32_t k, float boost, int32_t k_stride,
                                 void* d_keys, void* d_counts, void* d_hits) {
  if (!d_keys || !d_counts || !d_hits) return fail(NRTGPU_ERR_INVALID_ARG, "NULL argument");
  if (k_stride != (int32_t)round_up((uint32_t)k, 16)) return fail(NRTGPU_ERR_INVALID_ARG, "k_stride must be numHits rounded up to 16");
  const KnnUniform one{k, 0, boost, 0.0f};
  KnnCall call{segs, doc_bases, n_segs, field_id, /*bytes*/ false, queries, n_queries, dim, sim, /*knn_request*/ false, one.ask(), /*out*/ nullptr};
  call.ext_keys = (char*)d_keys, call.ext_cnts = (char*)d_counts, call.ext_hits = (char*)d_hits;
  return knn_search(ctx, call);
}

// An ExactVectorQuery per query: one k and one boost for all of them -- a stride-0 view (runtime_internal.h: KnnAsk).
extern "C" int nrtgpu_knn_exact(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                int32_t field_id, int32_t sim, const float* queries, int32_t n_queries, int32_t dim,
                                int32_t k, float boost, nrtgpu_topdocs* out) {
  const KnnUniform one{k, 0, boost, 0.0f};
  return knn_search(ctx, KnnCall{segs, doc_bases, n_segs, field_id, /*bytes*/ false, queries, n_queries, dim, sim, /*knn_request*/ false, one.ask(), out});
}

// ------------------------------------------------------------------------------------------------
// Request coalescing for exact vector searches (coalescer.h): what a kNN request is and which requests share a panel
// ------------------------------------------------------------------------------------------------
struct KnnCoRequest : CoQueued {
  const nrtgpu_seg* const* segs;
  const int32_t* doc_bases;
  int32_t n_segs, field_id, sim, dim, k;
  float boost;
  const void* query;   // dim elements of elem_size bytes: fp32, or int8 (the byte entries, on coalescers of their own)
  size_t elem_size;
  nrtgpu_topdocs* out;
  int32_t filter_mask = 0;   // (the knn request entries only: nrtgpu_knn_search_coalesced, nrtgpu_knn_search_bytes_coalesced)
  float min_score = 0.0f;
};

// same_boost: an ExactVectorQuery's boost is inside the scores its panel computes; a knn request's is applied when it is unpacked
static bool knn_co_compatible(const KnnCoRequest* a, const KnnCoRequest* b, bool same_boost) {
  if (a->n_segs != b->n_segs || a->field_id != b->field_id || a->sim != b->sim || a->dim != b->dim) return false;
  if (same_boost && a->boost != b->boost) return false;
  if (a->n_segs && memcmp(a->segs, b->segs, (size_t)a->n_segs * sizeof(void*)) != 0) return false;
  if ((a->doc_bases == nullptr) != (b->doc_bases == nullptr)) return false;
  return !a->doc_bases || memcmp(a->doc_bases, b->doc_bases, (size_t)a->n_segs * 4) == 0;
}

// TotalHits.relation of an exact vector query by the reference's rule (include/nrtgpu.h): one collector per searcher slice
// (MyIndexSearcher.java:163-208), each flips to GREATER_THAN_OR_EQUAL_TO once it has collected more than
// max(totalHitsThreshold, numHits) hits with its queue full (LazyQueueTopScoreDocCollector.java:176-199).  A slice collects the
// live docs of its leaves that carry a vector.  Host only.
extern "C" int nrtgpu_knn_exact_relation(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                         int32_t field_id, int32_t k, int32_t total_hits_threshold) {
  if (!ctx || (n_segs > 0 && !segs) || n_segs < 0 || k <= 0 || total_hits_threshold < 0) return fail(NRTGPU_ERR_INVALID_ARG, "bad knn_exact_relation arguments");
  if (total_hits_threshold == INT32_MAX) return 0;   // ScoreMode.COMPLETE: the collector never publishes a min competitive score
  for (int32_t i = 0; i < n_segs; ++i)
    if (!segs[i]) return fail(NRTGPU_ERR_STATE, "segment %d missing or not sealed", i);
  SegReadLocks content(segs, n_segs);   // liveDocs of the handles are read: not under a set_live_docs on one of them
  std::vector<int64_t> live((size_t)std::max(n_segs, 1), 0);
  std::vector<hostmath::LeafInfo> all((size_t)n_segs);
  int32_t base = 0;
  for (int32_t i = 0; i < n_segs; ++i) {
    if (!segs[i] || !segs[i]->sealed) return fail(NRTGPU_ERR_STATE, "segment %d missing or not sealed", i);
    all[(size_t)i] = {i, segs[i]->max_doc, segs[i]->max_doc - segs[i]->n_deleted, doc_bases ? doc_bases[i] : base};
    base += segs[i]->max_doc;
  }
  for (const bool bytes : {false, true})   // (a field holds float rows or byte rows)
    (void)knn_walk_leaves(segs, doc_bases, n_segs, field_id, bytes, -1, [&](const KnnLeaf& at) -> int {
      live[(size_t)at.si] = at.live;
      return NRTGPU_OK;
    });
  const int64_t floor_ = (int64_t)std::max(total_hits_threshold, k);
  if (ctx->slice_max_docs.load() <= 0 || n_segs == 0) {   // the whole search counts as one slice
    int64_t sum = 0;
    for (int64_t v : live) sum += v;
    return sum > floor_ ? 1 : 0;
  }
  const int32_t vs = ctx->virtual_shards.load();
  const std::vector<std::vector<int32_t>> sl = vs > 1
      ? hostmath::slices_for_shards(all, vs, ctx->slice_max_docs.load(), ctx->slice_max_segments.load(), nullptr)
      : hostmath::slices(all, ctx->slice_max_docs.load(), ctx->slice_max_segments.load(), all);
  for (const std::vector<int32_t>& s_ : sl) {
    int64_t sum = 0;
    for (int32_t li : s_) sum += live[(size_t)li];
    if (sum > floor_) return 1;
  }
  return 0;
}

// The wait of the single-query vector entries (nrtgpu_knn_exact_coalesced on ctx->kco, nrtgpu_knn_search_coalesced on ctx->rco,
// their byte twins on ctx->bkco and ctx->brco): one leave rule, one cap.  false: the request travelled in a leader's panel (or expired in the queue), me.rc / me.err
// and its results are in place.  true: this caller leads *batch -- itself first -- and runs it.
static bool knn_co_wait(Coalescer& co, KnnCoRequest& me, bool same_boost, std::vector<CoQueued*>* batch) {
  me.deadline_ns = g_deadline_ns;
  {
    std::unique_lock<std::mutex> lk;
    // (a follower wakes the leader when a whole panel waits, or -- device free -- when the last panel's cohort is back)
    const bool leads = co.join(lk, &me, [&](int32_t waiting) {
      return waiting >= kKnnMaxQ || (co.inflight == 0 && co.last_batch > 1 && waiting >= co.last_batch);
    });
    if (!leads) {   // travelled in a leader's panel
      if (me.rc != 0) g_last_error = me.err;
      return false;
    }
    // leader: leave at once when the device is free; else when the running panel finishes, or -- as a second panel in flight,
    // whose launches fill the tails of the first one's -- as soon as a whole panel is waiting
    // (NO linger for company: a caller that finds the device free runs alone -- company comes from the callers that arrive while a
    //  panel is running.  The clock handed to leader_wait bounds the cohort wait below and nothing else: while a panel is in flight,
    //  or under hold, the leader sleeps until it is woken.  hold: the test hook of nrtgpu_debug_hold_coalescers.)
    // The cohort of a closed loop: the members of a panel come back within tens of microseconds of each other, and the first one
    // back used to find the device free and leave alone -- the others then waited a whole pass (2.7 ms at C4) for theirs: 8
    // callers ran at 1.8 k queries/s with p50 5.5 ms where one panel of 8 per pass gives 2.9 k at 2.8 ms.  So a leader that finds
    // the device free after a panel of N > 1 waits until N callers are pending again, for at most kKnnCohortLingerUs; a lone
    // stream of callers (last panel 1) never waits.  NRTGPU_KCO_COHORT=0 (development build): leave at once, A/B.
    static const bool cohort_rule = dev_env_int("NRTGPU_KCO_COHORT", 1) != 0;
    constexpr int kKnnCohortLingerUs = 150;
    co.leader_wait(lk, &me, kKnnCohortLingerUs, [&](int32_t waiting, bool late) {
      if ((co.inflight == 1 || co.hold) && waiting >= kKnnMaxQ) return CoWait::leave;
      if (co.inflight != 0 || co.hold) return CoWait::until_woken;   // (for the running panel's end, a whole panel, the release)
      const bool cohort_due = cohort_rule && co.last_batch > 1 && waiting < std::min(co.last_batch, kKnnMaxQ) && !late;
      return cohort_due ? CoWait::until_linger_end : CoWait::leave;
    });
    *batch = co.form(&me, kKnnMaxQ, [&](const CoQueued* r) { return knn_co_compatible(&me, static_cast<const KnnCoRequest*>(r), same_boost); },
                     deadline_passed, NRTGPU_ERR_TIMEOUT, "deadline passed while the request waited for a panel");
  }
  return true;
}

// The leader's panel, outside the lock: the members' queries side by side, the largest k; every member's buffers take its own k.
// run(queries, kmax, outs) searches them (queries: the members' element type); then every member gets its results (or the panel's
// error) and its caller is woken.
template <class Run>
static int knn_co_run_panel(Coalescer& co, const std::vector<CoQueued*>& batch, KnnCoRequest& me, Run&& run) {
  auto member = [&](size_t i) { return static_cast<KnnCoRequest*>(batch[i]); };
  int32_t kmax = 0;
  const size_t q_bytes = (size_t)me.dim * me.elem_size;
  std::vector<char> qs(batch.size() * q_bytes);
  std::vector<nrtgpu_topdocs> outs(batch.size());
  for (size_t i = 0; i < batch.size(); ++i) {
    const KnnCoRequest* r = member(i);
    kmax = std::max(kmax, r->k);
    memcpy(qs.data() + i * q_bytes, r->query, q_bytes);
    outs[i] = *r->out;
    const int32_t cap = outs[i].capacity > 0 ? outs[i].capacity : r->k;
    outs[i].capacity = std::min(cap, r->k);
  }
  int rc;
  {
    // (a panel of several requests does not run under its leader's deadline: its mates have not expired)
    DeadlineScope deadline_scope(batch.size() > 1);
    rc = run((const void*)qs.data(), kmax, outs.data());
  }
  const std::string err = rc ? g_last_error : std::string();
  for (size_t i = 0; i < batch.size(); ++i) {
    KnnCoRequest* r = member(i);
    auto copy_back = [&] {   // (the caller's own capacity stays)
      if (rc != 0) return;
      const int32_t cap = r->out->capacity;
      *r->out = outs[i];
      r->out->capacity = cap;
    };
    if (r == &me) copy_back();
    else Coalescer::finish(r, rc, err, copy_back);
  }
  co.retire(batch.size());
  if (rc != 0) g_last_error = err;
  return rc;
}

// What only a byte entry asks of its queries and its boost, in knn_bytes_search's words: cosine refuses a zero query as the reference
// does (validateVectorForSearch, VectorFieldDef.java:853-861), named like every other bad request.
static int knn_check_queries(const KnnKind& kind, int32_t sim, const void* queries, int32_t n_queries, int32_t dim) {
  if (!kind.bytes || sim != 0) return NRTGPU_OK;
  for (int32_t q = 0; q < n_queries; ++q) {
    const int8_t* v = (const int8_t*)queries + (size_t)q * dim;
    if (std::all_of(v, v + dim, [](int8_t x) { return x == 0; }))
      return fail(NRTGPU_ERR_INVALID_ARG, "query %d: a zero vector: cosine similarity is not defined for it", q);
  }
  return NRTGPU_OK;
}

// nrtgpu_knn_exact_coalesced and nrtgpu_knn_exact_bytes_coalesced, on the kind's own coalescer.
static int knn_exact_coalesced(const KnnKind& kind, Coalescer& co, nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases,
                               int32_t n_segs, int32_t field_id, int32_t sim, const void* query, int32_t dim, int32_t k, float boost,
                               nrtgpu_topdocs* out) {
  if (!ctx || !query || !out || (n_segs > 0 && !segs)) return fail(NRTGPU_ERR_INVALID_ARG, "NULL argument");
  // (what would fail the panel must fail this request alone)
  if (int rc = knn_check_scalars(n_segs < 0, k, dim, sim)) return rc;
  if (kind.bytes)
    if (int rc = knn_check_byte_boost(boost)) return rc;
  if (int rc = knn_check_queries(kind, sim, query, 1, dim)) return rc;
  for (int si = 0; si < n_segs; ++si) {
    if (!segs[si] || !segs[si]->sealed) return fail(NRTGPU_ERR_STATE, "segment %d missing or not sealed", si);
    auto fit = segs[si]->fields.find(field_id);
    if (fit != segs[si]->fields.end())
      if (int rc = knn_check_field(kind.bytes, si, field_id, fit->second, dim, kind.other_type_hint)) return rc;
  }
  NRT_CHECK_DEADLINE("before the request was queued");
  KnnCoRequest me{{}, segs, doc_bases, n_segs, field_id, sim, dim, k, boost, query, kind.elem_size, out};
  std::vector<CoQueued*> batch;
  if (!knn_co_wait(co, me, true, &batch)) return me.rc;
  return knn_co_run_panel(co, batch, me, [&](const void* qs, int32_t kmax, nrtgpu_topdocs* outs) {
    const KnnUniform one{kmax, 0, boost, 0.0f};   // (the members' buffers take their own k of the panel's largest: knn_co_run_panel)
    return kind.search(ctx, KnnCall{segs, doc_bases, n_segs, field_id, kind.bytes, qs, (int32_t)batch.size(), dim, sim, /*knn_request*/ false, one.ask(), outs});
  });
}

extern "C" int nrtgpu_knn_exact_coalesced(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                          int32_t field_id, int32_t sim, const float* query, int32_t dim, int32_t k, float boost,
                                          nrtgpu_topdocs* out) {
  if (!ctx) return fail(NRTGPU_ERR_INVALID_ARG, "NULL argument");
  return knn_exact_coalesced(kKnnFloat, ctx->kco, ctx, segs, doc_bases, n_segs, field_id, sim, query, dim, k, boost, out);
}
extern "C" int nrtgpu_knn_exact_bytes_coalesced(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                                int32_t field_id, int32_t sim, const int8_t* query, int32_t dim, int32_t k, float boost,
                                                nrtgpu_topdocs* out) {
  if (!ctx) return fail(NRTGPU_ERR_INVALID_ARG, "NULL argument");
  return knn_exact_coalesced(kKnnBytes, ctx->bkco, ctx, segs, doc_bases, n_segs, field_id, sim, query, dim, k, boost, out);
}

extern "C" int nrtgpu_knn_search(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                 int32_t field_id, int32_t sim, const float* queries, int32_t n_queries, int32_t dim,
                                 int32_t k, float boost, int32_t filter_mask, float min_score, nrtgpu_topdocs* out) {
  if (filter_mask < 0 || !(min_score >= 0.0f) || !(boost > 0.0f))
    return fail(NRTGPU_ERR_INVALID_ARG, "knn search: filter_mask >= 0, min_score >= 0 and boost > 0 expected");
  const KnnUniform one{k, filter_mask, boost, min_score};   // one request for every query: a stride-0 view (runtime_internal.h: KnnAsk)
  return knn_search(ctx, KnnCall{segs, doc_bases, n_segs, field_id, /*bytes*/ false, queries, n_queries, dim, sim, /*knn_request*/ true, one.ask(), out});
}

// ------------------------------------------------------------------------------------------------
// knn requests with a k, boost, pre-filter and threshold EACH, in passes that share one read of the rows (include/nrtgpu.h)
// ------------------------------------------------------------------------------------------------
// What one request may ask (nrtgpu_knn_search's refusals); qi names it in the error text.
static int knn_request_check(int32_t qi, int32_t k, float boost, int32_t filter_mask, float min_score) {
  if (k <= 0) return fail(NRTGPU_ERR_INVALID_ARG, "query %d: k %d (> 0 expected)", qi, k);
  if (filter_mask < 0) return fail(NRTGPU_ERR_INVALID_ARG, "query %d: filter_mask %d (>= 0 expected)", qi, filter_mask);
  if (!(min_score >= 0.0f)) return fail(NRTGPU_ERR_INVALID_ARG, "query %d: min_score >= 0 expected", qi);
  if (!(boost > 0.0f) || !std::isfinite(boost)) return fail(NRTGPU_ERR_INVALID_ARG, "query %d: a finite boost > 0 expected", qi);
  if (k > NRTGPU_MAX_K) return fail(NRTGPU_ERR_UNSUPPORTED, "query %d: k %d > %d", qi, k, NRTGPU_MAX_K);
  return NRTGPU_OK;
}
// What the call asks of the field in every leaf (a field of the kind's element type and of the queries' dimension, or absent) and
// of the requests' masks (resident on every leaf that holds the field's rows -- the leaves a search would read them on).  Host only.
static int knn_requests_check_leaves(const KnnKind& kind, const nrtgpu_seg* const* segs, int32_t n_segs, int32_t field_id, int32_t dim,
                                     const int32_t* masks, int32_t n_queries) {
  for (int si = 0; si < n_segs; ++si)
    if (!segs[si]) return fail(NRTGPU_ERR_STATE, "segment %d missing or not sealed", si);
  SegReadLocks content(segs, n_segs);   // (the handles' masks are read)
  for (int si = 0; si < n_segs; ++si) {
    if (!segs[si]->sealed) return fail(NRTGPU_ERR_STATE, "segment %d missing or not sealed", si);
    auto fit = segs[si]->fields.find(field_id);
    if (fit == segs[si]->fields.end()) continue;
    bool has_rows = false;
    if (int rc = knn_check_field(kind.bytes, si, field_id, fit->second, dim, kind.other_type_hint, &has_rows)) return rc;
    if (!has_rows) continue;
    for (int32_t q = 0; masks && q < n_queries; ++q)
      if (masks[q] != 0 && segs[si]->masks.find(masks[q]) == segs[si]->masks.end())
        return fail(NRTGPU_ERR_UNSUPPORTED, "query %d: filter mask %d is not resident on segment %d", q, masks[q], si);
  }
  return NRTGPU_OK;
}

// The requests are valid (knn_request_check, knn_requests_check_leaves); call.ask: one value per query (stride 1).
static int knn_requests_run(const KnnKind& kind, nrtgpu_ctx* ctx, KnnCall call) {
  const KnnAsk all = call.ask;
  const int32_t n_queries = call.n_queries;
  bool all_equal = true;
  for (int32_t q = 1; q < n_queries && all_equal; ++q)
    all_equal = all.k(q) == all.k(0) && all.boost(q) == all.boost(0) && all.mask(q) == all.mask(0) && all.min_score(q) == all.min_score(0);
  if (all_equal) {   // one filter, one threshold: nrtgpu_knn_search's (nrtgpu_knn_search_bytes') own path, the gather route included
    call.ask.stride = 0;
    return kind.search(ctx, call);
  }
  const int32_t pass_q = kind.pass_q(call.dim);
  for (int32_t q0 = 0; q0 < n_queries; q0 += pass_q) {
    if (q0 > 0 && deadline_passed(g_deadline_ns))
      return fail(NRTGPU_ERR_TIMEOUT, "deadline passed between two passes over the rows (%d of %d queries answered)", q0, n_queries);
    KnnCall pass = call;   // (a search of its own: its slot, its locks, the largest k of ITS members)
    pass.queries = (const char*)call.queries + (size_t)q0 * call.dim * kind.elem_size;
    pass.n_queries = std::min(pass_q, n_queries - q0);
    pass.ask = all.from(q0);
    pass.out = call.out + q0;
    if (int rc = kind.search(ctx, pass)) return rc;
  }
  return NRTGPU_OK;
}

// nrtgpu_knn_search_requests and nrtgpu_knn_search_bytes_requests.
static int knn_search_requests(const KnnKind& kind, nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                               int32_t field_id, int32_t sim, const void* queries, int32_t n_queries, int32_t dim, const int32_t* ks,
                               const float* boosts, const int32_t* filter_masks, const float* min_scores, nrtgpu_topdocs* out) {
  if (!ctx || !queries || !out || !ks || (n_segs > 0 && !segs)) return fail(NRTGPU_ERR_INVALID_ARG, "NULL argument");
  if (int rc = knn_check_scalars(n_queries <= 0 || n_segs < 0, 1, dim, sim)) return rc;
  // a bad request refuses the whole call before anything is launched
  for (int32_t q = 0; q < n_queries; ++q)
    if (int rc = knn_request_check(q, ks[q], boosts ? boosts[q] : 1.0f, filter_masks ? filter_masks[q] : 0, min_scores ? min_scores[q] : 0.0f)) return rc;
  if (int rc = knn_check_queries(kind, sim, queries, n_queries, dim)) return rc;
  if (int rc = knn_requests_check_leaves(kind, segs, n_segs, field_id, dim, filter_masks, n_queries)) return rc;
  NRT_CHECK_DEADLINE("before the vector search started");
  std::vector<float> one, none_f;
  std::vector<int32_t> none_i;
  if (!boosts) one.assign((size_t)n_queries, 1.0f);
  if (!min_scores) none_f.assign((size_t)n_queries, 0.0f);
  if (!filter_masks) none_i.assign((size_t)n_queries, 0);
  const KnnAsk ask{ks, boosts ? boosts : one.data(), filter_masks ? filter_masks : none_i.data(), min_scores ? min_scores : none_f.data(), 1};
  return knn_requests_run(kind, ctx, KnnCall{segs, doc_bases, n_segs, field_id, kind.bytes, queries, n_queries, dim, sim, /*knn_request*/ true, ask, out});
}

// nrtgpu_knn_search_coalesced and nrtgpu_knn_search_bytes_coalesced, on the kind's own coalescer.
static int knn_search_coalesced(const KnnKind& kind, Coalescer& co, nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases,
                                int32_t n_segs, int32_t field_id, int32_t sim, const void* query, int32_t dim, int32_t k, float boost,
                                int32_t filter_mask, float min_score, nrtgpu_topdocs* out) {
  if (!ctx || !query || !out || (n_segs > 0 && !segs)) return fail(NRTGPU_ERR_INVALID_ARG, "NULL argument");
  // (what would fail the panel must fail this request alone: its scalars, its query, the field, its mask on every leaf)
  if (int rc = knn_check_scalars(n_segs < 0, 1, dim, sim)) return rc;
  if (int rc = knn_request_check(0, k, boost, filter_mask, min_score)) return rc;
  if (int rc = knn_check_queries(kind, sim, query, 1, dim)) return rc;
  if (int rc = knn_requests_check_leaves(kind, segs, n_segs, field_id, dim, &filter_mask, 1)) return rc;
  NRT_CHECK_DEADLINE("before the request was queued");
  KnnCoRequest me{{}, segs, doc_bases, n_segs, field_id, sim, dim, k, boost, query, kind.elem_size, out, filter_mask, min_score};
  std::vector<CoQueued*> batch;
  if (!knn_co_wait(co, me, false, &batch)) return me.rc;
  return knn_co_run_panel(co, batch, me, [&](const void* qs, int32_t, nrtgpu_topdocs* outs) {
    std::vector<int32_t> ks(batch.size()), masks(batch.size());
    std::vector<float> boosts(batch.size()), mins(batch.size());
    for (size_t i = 0; i < batch.size(); ++i) {
      const KnnCoRequest* r = static_cast<const KnnCoRequest*>(batch[i]);
      ks[i] = r->k;
      boosts[i] = r->boost;
      masks[i] = r->filter_mask;
      mins[i] = r->min_score;
    }
    const KnnAsk ask{ks.data(), boosts.data(), masks.data(), mins.data(), 1};
    return knn_requests_run(kind, ctx, KnnCall{segs, doc_bases, n_segs, field_id, kind.bytes, qs, (int32_t)batch.size(), dim, sim, /*knn_request*/ true, ask, outs});
  });
}

extern "C" int nrtgpu_knn_search_requests(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                          int32_t field_id, int32_t sim, const float* queries, int32_t n_queries, int32_t dim,
                                          const int32_t* ks, const float* boosts, const int32_t* filter_masks, const float* min_scores,
                                          nrtgpu_topdocs* out) {
  return knn_search_requests(kKnnFloat, ctx, segs, doc_bases, n_segs, field_id, sim, queries, n_queries, dim, ks, boosts, filter_masks, min_scores, out);
}
extern "C" int nrtgpu_knn_search_bytes_requests(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                                int32_t field_id, int32_t sim, const int8_t* queries, int32_t n_queries, int32_t dim,
                                                const int32_t* ks, const float* boosts, const int32_t* filter_masks, const float* min_scores,
                                                nrtgpu_topdocs* out) {
  return knn_search_requests(kKnnBytes, ctx, segs, doc_bases, n_segs, field_id, sim, queries, n_queries, dim, ks, boosts, filter_masks, min_scores, out);
}
extern "C" int nrtgpu_knn_search_coalesced(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                           int32_t field_id, int32_t sim, const float* query, int32_t dim, int32_t k, float boost,
                                           int32_t filter_mask, float min_score, nrtgpu_topdocs* out) {
  if (!ctx) return fail(NRTGPU_ERR_INVALID_ARG, "NULL argument");
  return knn_search_coalesced(kKnnFloat, ctx->rco, ctx, segs, doc_bases, n_segs, field_id, sim, query, dim, k, boost, filter_mask, min_score, out);
}
extern "C" int nrtgpu_knn_search_bytes_coalesced(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                                 int32_t field_id, int32_t sim, const int8_t* query, int32_t dim, int32_t k, float boost,
                                                 int32_t filter_mask, float min_score, nrtgpu_topdocs* out) {
  if (!ctx) return fail(NRTGPU_ERR_INVALID_ARG, "NULL argument");
  return knn_search_coalesced(kKnnBytes, ctx->brco, ctx, segs, doc_bases, n_segs, field_id, sim, query, dim, k, boost, filter_mask, min_score, out);
}

// The two-call rescorer: QueryRescorer over a first pass's hits, for either element type (runtime_internal.h: RescoreKind).
int nrtgpu::rt::rescore_hits_impl(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs, int32_t field_id,
                                  const RescoreKind& kind, const int32_t* docs, const float* first_scores, int32_t n, double query_weight,
                                  int32_t window, nrtgpu_topdocs* out) {
  auto rows_of = [&](int si) -> const FieldData* {
    auto fit = segs[si]->fields.find(field_id);
    return fit != segs[si]->fields.end() && kind.rows(fit->second) ? &fit->second : nullptr;
  };
  // hits -> (segment, vector row); per segment one gather kernel
  std::vector<int> seg_of((size_t)n, -1);
  std::vector<int64_t> row_of((size_t)n, -1);
  for (int i = 0; i < n; ++i) {
    for (int si = 0; si < n_segs; ++si) {
      const int64_t local = (int64_t)docs[i] - (int64_t)doc_bases[si];
      if (local < 0 || local >= (int64_t)segs[si]->max_doc) continue;
      seg_of[(size_t)i] = si;
      const FieldData* f = rows_of(si);
      if (!f) break;
      if (f->h_ord_to_doc.empty()) {
        if (local < (int64_t)f->n_vec) row_of[(size_t)i] = local;
      } else {
        auto it = std::lower_bound(f->h_ord_to_doc.begin(), f->h_ord_to_doc.end(), (int32_t)local);
        if (it != f->h_ord_to_doc.end() && *it == (int32_t)local) row_of[(size_t)i] = it - f->h_ord_to_doc.begin();
      }
      break;
    }
    if (seg_of[(size_t)i] < 0) return fail(NRTGPU_ERR_INVALID_ARG, "hit %d (doc %d) is outside every segment", i, docs[i]);
  }
  Slot* slot = nullptr;
  acquire_slot(ctx, &slot);
  SlotGuard guard{ctx, slot};
  std::lock_guard<std::mutex> gpu(ctx->gpu_mu);
  hipStream_t st = slot->stream;
  std::vector<float> combined((size_t)n);
  auto on_device = [&]() -> int {
    if (ctx->last_turn) HIP_TRY(hipStreamWaitEvent(st, ctx->last_turn, 0));
    Carver wc;
    const size_t o_q = wc.take(kind.query_bytes), o_rows = wc.take((size_t)n * 8 + 8), o_first = wc.take((size_t)n * 4 + 4),
                 o_out = wc.take((size_t)n * 4 + 4);
    if (int rc = slot->d_work.reserve(wc.off)) return rc;
    char* wb = (char*)slot->d_work.p;
    HIP_TRY(hipMemcpyAsync(wb + o_q, kind.query, kind.query_bytes, hipMemcpyHostToDevice, st));
    for (int si = 0; si < n_segs; ++si) {
      std::vector<int> idx;
      for (int i = 0; i < n; ++i)
        if (seg_of[(size_t)i] == si) idx.push_back(i);
      if (idx.empty()) continue;
      const FieldData* f = rows_of(si);
      if (!f) {  // no vectors in this leaf: the second pass matches nothing
        for (int i : idx) combined[(size_t)i] = (float)(query_weight * (double)first_scores[i]);
        continue;
      }
      std::vector<int64_t> rows(idx.size());
      std::vector<float> first(idx.size()), res(idx.size());
      for (size_t j = 0; j < idx.size(); ++j) {
        rows[j] = row_of[(size_t)idx[j]];
        first[j] = first_scores[idx[j]];
      }
      HIP_TRY(hipMemcpyAsync(wb + o_rows, rows.data(), rows.size() * 8, hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(wb + o_first, first.data(), first.size() * 4, hipMemcpyHostToDevice, st));
      kind.launch(st, *f, wb + o_q, (const int64_t*)(wb + o_rows), (const float*)(wb + o_first), (int32_t)idx.size(), (float*)(wb + o_out));
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(res.data(), wb + o_out, res.size() * 4, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));   // (the staging vectors of this leaf go out of scope)
      for (size_t j = 0; j < idx.size(); ++j) combined[(size_t)idx[j]] = res[j];
    }
    return NRTGPU_OK;
  };
  if (int rc = on_device()) {
    (void)hipStreamSynchronize(st);   // nothing of a failed call is in flight when the slot is released (its copies read this frame's vectors)
    return rc;
  }
  // QueryRescorer: sort by (combined score desc, doc asc), keep the window
  std::vector<int> order((size_t)n);
  for (int i = 0; i < n; ++i) order[(size_t)i] = i;
  std::sort(order.begin(), order.end(), [&](int a, int b) {
    if (combined[(size_t)a] != combined[(size_t)b]) return combined[(size_t)a] > combined[(size_t)b];
    return docs[a] < docs[b];
  });
  const int32_t cap = out->capacity > 0 ? out->capacity : window;
  const int32_t m = std::min<int32_t>(std::min<int32_t>(n, window), cap);
  for (int32_t i = 0; i < m; ++i) {
    if (out->docs) out->docs[i] = docs[order[(size_t)i]];
    if (out->scores) out->scores[i] = combined[(size_t)order[(size_t)i]];
  }
  out->n_hits = m;
  out->total_hits = n;
  out->total_hits_is_lower_bound = 0;
  return NRTGPU_OK;
}

extern "C" int nrtgpu_rescore_vectors(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                      int32_t field_id, int32_t sim, const float* query, int32_t dim, float boost,
                                      const int32_t* docs, const float* first_scores, int32_t n, double query_weight,
                                      double rescore_weight, int32_t window, nrtgpu_topdocs* out) {
  forget_foreign_hip_error();
  if (!ctx || !query || !out || (n > 0 && (!docs || !first_scores)) || (n_segs > 0 && (!segs || !doc_bases)))
    return fail(NRTGPU_ERR_INVALID_ARG, "NULL argument");
  if (n < 0 || dim <= 0 || sim < 0 || sim > 3 || window <= 0) return fail(NRTGPU_ERR_INVALID_ARG, "bad rescore arguments");
  HIP_TRY(hipSetDevice(ctx->device));
  for (int si = 0; si < n_segs; ++si)
    if (!segs[si]) return fail(NRTGPU_ERR_INVALID_ARG, "segment %d is NULL", si);
  PaddedQueries padded;   // (rows are resident padded to a multiple of 16 elements: the query likewise)
  if (int rc = pad_query_vectors(segs, n_segs, field_id, query, 1, dim, &padded)) return rc;
  const int32_t rdim = padded.dim;   // the RESIDENT dimension: every leaf's rows have it once pad_query_vectors has accepted the field
  float qn = 0.f;
  (void)stage_rescore_inputs(segs, doc_bases, n_segs, field_id, false, sim, padded.p, 1, rdim, nullptr, nullptr, &qn);
  const RescoreKind kind{[](const FieldData& f) -> const void* { return f.d_vectors; }, padded.p, (size_t)rdim * 4,
                         [&](hipStream_t st, const FieldData& f, const void* d_query, const int64_t* d_rows, const float* d_first, int32_t m, float* d_out) {
                           launch_rescore_vectors(st, f.d_vectors, f.d_vnorm2, rdim, (const float*)d_query, qn, sim, boost, d_rows, d_first, m,
                                                  query_weight, rescore_weight, d_out);
                         }};
  return rescore_hits_impl(ctx, segs, doc_bases, n_segs, field_id, kind, docs, first_scores, n, query_weight, window, out);
}
