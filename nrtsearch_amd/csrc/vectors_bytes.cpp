// vectors_bytes.cpp -- exact search over byte (int8) vector fields: ExactByteVectorQuery and the `knn` request path over a byte field.
//
// The host side of knn_bytes.hip, beside knn_impl (vectors.cpp) and a fraction of it: the pass over the rows returns RESULTS
// (integers from the i8 matrix cores, mapped to score bits by plan.h: knn_byte_score), so there are no error bounds, no
// rescoring, no certificate and no second pass here -- only the rounds that tighten theta and the selection they share with the
// float search (knn.hip: knn_select_kernel<false>).  Workspace, stream, turn-taking, content locks, deadlines and statistics are
// knn_impl's.
#include "runtime_internal.h"

static const uint32_t kKnnBytesCap = 1u << 18;   // candidate keys per query and round (2 MiB)
static const int kKnnBytesMaxQ = 64;             // queries per pass over the rows: four panels of 16

static int knn_bytes_impl(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs, int32_t field_id,
                          int32_t sim, const int8_t* queries, int32_t n_queries, int32_t dim, int32_t k, float boost, bool knn_request,
                          int32_t filter_mask, float min_score, nrtgpu_topdocs* out) {
  forget_foreign_hip_error();
  if (!ctx || !queries || !out || (n_segs > 0 && !segs)) return fail(NRTGPU_ERR_INVALID_ARG, "NULL argument");
  if (n_queries <= 0 || k <= 0 || dim <= 0 || sim < 0 || sim > 3 || n_segs < 0) return fail(NRTGPU_ERR_INVALID_ARG, "bad knn arguments");
  // (hits are kept as keys whose order is the order of NON-NEGATIVE float bits: a negative boost would rank them backwards)
  if (!(boost >= 0.0f) || !(boost < INFINITY)) return fail(NRTGPU_ERR_INVALID_ARG, "byte vector search: a finite boost >= 0 expected");
  if (k > NRTGPU_MAX_K) return fail(NRTGPU_ERR_UNSUPPORTED, "k %d > %d", k, NRTGPU_MAX_K);
  if (dim > 2048) return fail(NRTGPU_ERR_UNSUPPORTED, "vector dimension %d (device path takes <= 2048)", dim);
  // |q|^2 of every query; cosine refuses a zero query as the reference does (validateVectorForSearch, VectorFieldDef.java:853-861)
  std::vector<int32_t> qn2((size_t)n_queries);
  for (int32_t q = 0; q < n_queries; ++q) {
    int32_t s = 0;
    for (int32_t d = 0; d < dim; ++d) {
      const int32_t x = queries[(size_t)q * dim + d];
      s += x * x;
    }
    if (sim == 0 && s == 0) return fail(NRTGPU_ERR_INVALID_ARG, "query %d is a zero vector: cosine similarity is not defined for it", q);
    qn2[(size_t)q] = s;
  }
  NRT_CHECK_DEADLINE("before the vector search started");
  HIP_TRY(hipSetDevice(ctx->device));
  for (int si = 0; si < n_segs; ++si)
    if (!segs[si]) return fail(NRTGPU_ERR_STATE, "segment %d missing or not sealed", si);
  SegReadLocks content(segs, n_segs);  // liveDocs / masks stay as they are until the kernels have finished
  for (int si = 0; si < n_segs; ++si) {
    if (!segs[si]->sealed) return fail(NRTGPU_ERR_STATE, "segment %d missing or not sealed", si);
    auto fit = segs[si]->fields.find(field_id);
    if (fit == segs[si]->fields.end()) continue;
    const FieldData& f = fit->second;
    if (!f.byte_rows && (f.d_vectors || f.dim > 0))
      return fail(NRTGPU_ERR_INVALID_ARG, "segment %d: field %d holds float (fp32) vectors: search it with nrtgpu_knn_exact / nrtgpu_knn_search", si, field_id);
    if (f.byte_rows && f.dim_user != dim)
      return fail(NRTGPU_ERR_INVALID_ARG, "segment %d: field %d has dimension %d, query has %d", si, field_id, f.dim_user, dim);
  }
  const uint32_t k_stride = round_up((uint32_t)k, 16);
  const float score_boost = knn_request ? 1.0f : boost;   // the knn request: min_score tests the unboosted score, the boost comes afterwards
  Slot* slot = nullptr;
  acquire_slot(ctx, &slot);
  struct Guard { nrtgpu_ctx* c; Slot* s; ~Guard() { release_slot(c, s); } } guard{ctx, slot};
  hipStream_t st = slot->stream;
  auto take_turn = [&]() -> int {   // (vectors.cpp: knn_impl explains the ordering against the BM25 scorers)
    std::lock_guard<std::mutex> gpu(ctx->gpu_mu);
    if (ctx->last_turn) HIP_TRY(hipStreamWaitEvent(st, ctx->last_turn, 0));
    return NRTGPU_OK;
  };
  auto end_turn = [&]() -> int {
    std::lock_guard<std::mutex> gpu(ctx->gpu_mu);
    HIP_TRY(hipEventRecord(slot->ev_turn, st));
    ctx->last_knn_turn = slot->ev_turn;
    return NRTGPU_OK;
  };
  const bool timing = ctx->cfg.collect_timing != 0;
  const size_t panel_max = knn_bytes_panel_bytes(dim, kKnnBytesMaxQ);
  Carver wc;
  // the head [o_p, o_th) is staged in pinned memory laid out alike: one copy per panel
  const size_t o_p = wc.take(panel_max), o_qn = wc.take(kKnnBytesMaxQ * 4);
  const size_t o_leaves = wc.take((size_t)std::max(n_segs, 1) * sizeof(DKnnBytesLeaf));
  const size_t o_th = wc.take(kKnnBytesMaxQ * 8);
  const size_t o_tk = wc.take((size_t)kKnnBytesMaxQ * k_stride * 8), o_tc = wc.take(kKnnBytesMaxQ * 4);
  const size_t o_cc = wc.take(kKnnBytesMaxQ * 4), o_ov = wc.take(64);
  const size_t o_cd = wc.take((size_t)kKnnBytesMaxQ * kKnnBytesCap * 8);
  if (int rc = slot->d_work.reserve(wc.off)) return rc;
  const size_t oh_cnt = o_tc - o_tk, oh_ov = o_ov - o_tk;   // keys, counts and the overflow flag come back in one copy
  if (int rc = slot->h_out.reserve(o_cd - o_tk)) return rc;
  if (int rc = slot->h_aux.reserve(o_th)) return rc;
  char* wb = (char*)slot->d_work.p;
  char* ho = (char*)slot->h_out.p;
  char* hs = (char*)slot->h_aux.p;
  // the leaves' tiles of 16 rows, numbered through: ONE launch walks every leaf
  DKnnBytesLeaf* hleaves = (DKnnBytesLeaf*)(hs + o_leaves);
  int32_t n_kleaves = 0;
  int64_t total_tiles = 0, total_rows = 0, live_vectors = 0;
  for (int si = 0; si < n_segs; ++si) {
    auto fit = segs[si]->fields.find(field_id);
    if (fit == segs[si]->fields.end() || !fit->second.d_btiles || fit->second.n_vec == 0) continue;
    const FieldData& f = fit->second;
    live_vectors += live_vector_count(segs[si], f);   // (deleted docs are masked inside the kernel and are no hits)
    const uint64_t* accept = segs[si]->d_live;
    if (knn_request && filter_mask != 0)
      if (int rc = accept_set_of(segs[si], filter_mask, 0, &accept)) return rc;
    DKnnBytesLeaf l{};
    l.tiles = f.d_btiles;
    l.vnorm2 = f.d_bnorm2;
    l.ord_to_doc = f.d_ord_to_doc;
    l.accept = accept;
    l.tile_begin = total_tiles;
    l.n_rows = f.n_vec;
    l.doc_base = doc_bases ? doc_bases[si] : 0;
    hleaves[n_kleaves++] = l;
    total_tiles += ((int64_t)f.n_vec + 15) >> 4;
    total_rows += f.n_vec;
  }
  const int32_t steps = knn_bytes_steps(dim);
  static const int64_t kFirstRound = (int64_t)(1 << 16) >> 4;   // tiles of the first round: every row takes a slot of the list
  for (int q0 = 0; q0 < n_queries; q0 += kKnnBytesMaxQ) {
    const int nq = std::min(kKnnBytesMaxQ, n_queries - q0);
    if (deadline_passed(g_deadline_ns)) {   // between two passes over the rows: nothing of the next one has been launched
      (void)hipStreamSynchronize(st);
      return fail(NRTGPU_ERR_TIMEOUT, "deadline passed between two passes over the rows (%d of %d queries answered)", q0, n_queries);
    }
    // the panel in the matrix instruction's operand order (knn_bytes.hip): [step][panel][lane] x 16 bytes, zeros behind the
    // field's dimension and behind the last query
    const int panels = nq > 16 ? 4 : 1;
    const size_t panel_bytes = (size_t)steps * panels * 1024;
    memset(hs + o_p, 0, panel_bytes);
    for (int q = 0; q < nq; ++q) {
      const int8_t* src = queries + (size_t)(q0 + q) * dim;
      const int p = q >> 4, j = q & 15;
      for (int32_t d0 = 0; d0 < dim; d0 += 16) {
        const int32_t s = d0 >> 6, kk = (d0 >> 4) & 3;
        memcpy(hs + o_p + (((size_t)s * panels + p) * 64 + (size_t)(kk * 16 + j)) * 16, src + d0, (size_t)std::min(16, dim - d0));
      }
    }
    memset(hs + o_qn, 0, kKnnBytesMaxQ * 4);
    memcpy(hs + o_qn, qn2.data() + q0, (size_t)nq * 4);
    HIP_TRY(hipMemcpyAsync(wb + o_p, hs + o_p, panel_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(wb + o_qn, hs + o_qn, o_th - o_qn, hipMemcpyHostToDevice, st));   // |q|^2, leaf table
    size_t n_ev = 0;
    // One pass over the rows of every leaf, in rounds with a selection in between (theta tightens from round to round): the first
    // round gives every row a slot of the list; later rounds only append rows that beat theta, so they grow -- and after two
    // selections the remaining launches run back to back with ONE selection behind them.  Rows in rising order of similarity could
    // overflow a list: the selection flags that and the panel is redone in rounds no longer than the list (`safe`).
    for (int safe = 0;; ++safe) {
      if (int rc = take_turn()) return rc;
      HIP_TRY(hipMemsetAsync(wb + o_th, 0, o_cd - o_th, st));  // theta, the running top-k, counters, flag
      int64_t seen = 0, round = kFirstRound;
      int selections = 0;
      bool pending = false;
      for (int64_t t = 0; t < total_tiles;) {
        int64_t len = (safe || seen == 0) ? std::min<int64_t>(round, kKnnBytesCap >> 4) : round;
        len = std::min<int64_t>(len, (int64_t)1 << 22);   // (a queue entry carries the padded row inside the launch in 26 bits)
        const int64_t te = std::min<int64_t>(total_tiles, t + len);
        const uint32_t blocks = (uint32_t)std::min<int64_t>(((te - t) * 16 + 255) / 256, (int64_t)std::max(ctx->n_cus, 1));
        if (timing) {
          while (slot->round_ev.size() < n_ev + 2) {
            hipEvent_t ev = nullptr;
            HIP_TRY(hipEventCreate(&ev));
            slot->round_ev.push_back(ev);
          }
          HIP_TRY(hipEventRecord(slot->round_ev[n_ev], st));
        }
        const bool defer = !safe && selections >= 2;
        const int e = launch_knn_bytes(st, blocks, (const DKnnBytesLeaf*)(wb + o_leaves), n_kleaves, dim, t, te, wb + o_p,
                                       (const int32_t*)(wb + o_qn), nq, sim, score_boost, knn_request ? min_score : 0.0f,
                                       (const unsigned long long*)(wb + o_th), (uint64_t*)(wb + o_cd), (uint32_t*)(wb + o_cc), kKnnBytesCap,
                                       defer ? 1 : 0);
        if (e) return fail(NRTGPU_ERR_HIP, "knn_bytes launch: %s", hipGetErrorString((hipError_t)e));
        if (timing) {
          HIP_TRY(hipEventRecord(slot->round_ev[n_ev + 1], st));
          n_ev += 2;
        }
        if (defer) {
          pending = true;
        } else {
          launch_knn_select(st, (uint32_t)nq, (uint64_t*)(wb + o_tk), (uint32_t*)(wb + o_tc), k_stride, (uint32_t)k,
                            (const uint64_t*)(wb + o_cd), (uint32_t*)(wb + o_cc), kKnnBytesCap, (unsigned long long*)(wb + o_th),
                            (uint32_t*)(wb + o_ov));
          ++selections;
        }
        seen += te - t;
        t = te;
        round = safe ? std::min<int64_t>(round * 4, kKnnBytesCap >> 4) : std::min<int64_t>(seen * 15, (int64_t)1 << 36);
      }
      if (pending)
        launch_knn_select(st, (uint32_t)nq, (uint64_t*)(wb + o_tk), (uint32_t*)(wb + o_tc), k_stride, (uint32_t)k,
                          (const uint64_t*)(wb + o_cd), (uint32_t*)(wb + o_cc), kKnnBytesCap, (unsigned long long*)(wb + o_th),
                          (uint32_t*)(wb + o_ov));
      if (int rc = end_turn()) return rc;
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(ho, wb + o_tk, o_ov + 4 - o_tk, hipMemcpyDeviceToHost, st));   // the answer, its counts, the flag
      HIP_TRY(hipStreamSynchronize(st));
      if (*(const uint32_t*)(ho + oh_ov) == 0u) break;
      if (safe) return fail(NRTGPU_ERR_HIP, "knn_bytes: candidate list overflow in a bounded round");
    }
    {
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
      ctx->stats.knn_rows += total_rows;
    }
    const uint64_t* keys = (const uint64_t*)ho;
    const uint32_t* cnts = (const uint32_t*)(ho + oh_cnt);
    for (int q = 0; q < nq; ++q) {
      nrtgpu_topdocs* o = &out[q0 + q];
      const int32_t cap = o->capacity > 0 ? o->capacity : k;
      const int32_t m = std::min<int32_t>((int32_t)std::min<uint32_t>(cnts[q], (uint32_t)k), cap);
      for (int32_t i = 0; i < m; ++i) {
        if (o->docs) o->docs[i] = (int32_t)key_doc(keys[(size_t)q * k_stride + i]);
        if (o->scores) o->scores[i] = key_score(keys[(size_t)q * k_stride + i]);
      }
      o->n_hits = m;
      o->total_hits = live_vectors;   // every live doc with a vector matches an exact vector query
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
  return NRTGPU_OK;
}

extern "C" int nrtgpu_knn_exact_bytes(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                      int32_t field_id, int32_t sim, const int8_t* queries, int32_t n_queries, int32_t dim, int32_t k,
                                      float boost, nrtgpu_topdocs* out) {
  return knn_bytes_impl(ctx, segs, doc_bases, n_segs, field_id, sim, queries, n_queries, dim, k, boost, false, 0, 0.0f, out);
}

extern "C" int nrtgpu_knn_search_bytes(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                       int32_t field_id, int32_t sim, const int8_t* queries, int32_t n_queries, int32_t dim, int32_t k,
                                       float boost, int32_t filter_mask, float min_score, nrtgpu_topdocs* out) {
  if (filter_mask < 0 || !(min_score >= 0.0f) || !(boost > 0.0f))
    return fail(NRTGPU_ERR_INVALID_ARG, "knn search: filter_mask >= 0, min_score >= 0 and boost > 0 expected");
  return knn_bytes_impl(ctx, segs, doc_bases, n_segs, field_id, sim, queries, n_queries, dim, k, boost, true, filter_mask, min_score, out);
}

// ---- the rescorers over a byte field: QueryRescore (rescore/QueryRescore.java:40-57) with the field's ExactByteVectorQuery
// (VectorFieldDef.java:842) in the rescore slot -- nrtgpu_rescore_byte_vectors here, the tail of nrtgpu_search_hybrid_bytes_batch in
// search.cpp: search_hybrid_impl, which stages its inputs through the three functions below ------------------------------------
// What the byte entries ask of their scalars, in knn_bytes_impl's order.
int nrtgpu::rt::byte_rescore_check_args(int32_t sim, int32_t dim, float boost, int32_t window) {
  if (dim <= 0 || sim < 0 || sim > 3 || window <= 0) return fail(NRTGPU_ERR_INVALID_ARG, "bad rescore arguments");
  // (the fused tail keeps hits as keys that order like NON-NEGATIVE float bits; the two-call path refuses the same boosts)
  if (!(boost >= 0.0f) || !(boost < INFINITY)) return fail(NRTGPU_ERR_INVALID_ARG, "byte vector rescore: a finite boost >= 0 expected");
  if (dim > 2048) return fail(NRTGPU_ERR_UNSUPPORTED, "vector dimension %d (device path takes <= 2048)", dim);
  return NRTGPU_OK;
}
// n queries of `dim` int8 -> piece order (knn_bytes.hip: the query itself, zero-padded to 64 x steps bytes per query) and |q|^2 as
// int32; cosine refuses a zero query as the reference does (validateVectorForSearch, VectorFieldDef.java:853-861).
size_t nrtgpu::rt::byte_query_stride(int32_t dim) { return (size_t)knn_bytes_steps(dim) * 64; }
int nrtgpu::rt::byte_queries_stage(const int8_t* queries, int32_t n, int32_t dim, int32_t sim, int8_t* padded, int32_t* qnorm2) {
  const size_t stride = byte_query_stride(dim);
  for (int32_t q = 0; q < n; ++q) {
    const int8_t* src = queries + (size_t)q * dim;
    int32_t s = 0;
    for (int32_t d = 0; d < dim; ++d) s += (int32_t)src[d] * (int32_t)src[d];
    if (sim == 0 && s == 0) return fail(NRTGPU_ERR_INVALID_ARG, "query %d is a zero vector: cosine similarity is not defined for it", q);
    if (qnorm2) qnorm2[q] = s;
    if (padded) {
      memcpy(padded + (size_t)q * stride, src, (size_t)dim);
      memset(padded + (size_t)q * stride + dim, 0, stride - (size_t)dim);
    }
  }
  return NRTGPU_OK;
}
// The field in every leaf: byte rows of the query's dimension, or absent.  `out` (may be NULL): the leaf table the kernel reads.
int nrtgpu::rt::byte_rescore_leaves(const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs, int32_t field_id, int32_t dim,
                                    DByteVecSeg* out) {
  for (int si = 0; si < n_segs; ++si) {
    DByteVecSeg v{};
    auto fit = segs[si]->fields.find(field_id);
    if (fit != segs[si]->fields.end()) {
      const FieldData& f = fit->second;
      if (!f.byte_rows && (f.d_vectors || f.dim > 0))
        return fail(NRTGPU_ERR_INVALID_ARG, "segment %d: field %d holds float (fp32) vectors: rescore it with nrtgpu_rescore_vectors / nrtgpu_search_hybrid_batch",
                    si, field_id);
      if (f.byte_rows && f.dim_user != dim)
        return fail(NRTGPU_ERR_INVALID_ARG, "segment %d: field %d has dimension %d, query has %d", si, field_id, f.dim_user, dim);
      if (f.byte_rows && f.d_btiles && f.n_vec > 0) {
        v.tiles = f.d_btiles;
        v.vnorm2 = f.d_bnorm2;
        v.ord_to_doc = f.d_ord_to_doc;
        v.n_vec = f.n_vec;
      }
    }
    v.doc_base = doc_bases[si];
    v.max_doc = segs[si]->max_doc;
    if (out) out[si] = v;
  }
  return NRTGPU_OK;
}

extern "C" int nrtgpu_rescore_byte_vectors(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                           int32_t field_id, int32_t sim, const int8_t* query, int32_t dim, float boost,
                                           const int32_t* docs, const float* first_scores, int32_t n, double query_weight,
                                           double rescore_weight, int32_t window, nrtgpu_topdocs* out) {
  forget_foreign_hip_error();
  if (!ctx || !query || !out || (n > 0 && (!docs || !first_scores)) || (n_segs > 0 && (!segs || !doc_bases)))
    return fail(NRTGPU_ERR_INVALID_ARG, "NULL argument");
  if (n < 0 || n_segs < 0) return fail(NRTGPU_ERR_INVALID_ARG, "bad rescore arguments");
  if (int rc = byte_rescore_check_args(sim, dim, boost, window)) return rc;
  // (the hits are sorted on the host: any finite weights)
  if (!(std::fabs(query_weight) < INFINITY) || !(std::fabs(rescore_weight) < INFINITY))
    return fail(NRTGPU_ERR_INVALID_ARG, "byte vector rescore: finite weights expected");
  std::vector<int8_t> qpad(byte_query_stride(dim));
  int32_t qn = 0;
  if (int rc = byte_queries_stage(query, 1, dim, sim, qpad.data(), &qn)) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  for (int si = 0; si < n_segs; ++si)
    if (!segs[si]) return fail(NRTGPU_ERR_INVALID_ARG, "segment %d is NULL", si);
  if (int rc = byte_rescore_leaves(segs, doc_bases, n_segs, field_id, dim, nullptr)) return rc;
  // hits -> (segment, vector row), on the host as nrtgpu_rescore_vectors does; per segment one kernel
  std::vector<int> seg_of((size_t)n, -1);
  std::vector<int64_t> row_of((size_t)n, -1);
  for (int i = 0; i < n; ++i) {
    for (int si = 0; si < n_segs; ++si) {
      const int64_t local = (int64_t)docs[i] - (int64_t)doc_bases[si];
      if (local < 0 || local >= (int64_t)segs[si]->max_doc) continue;
      seg_of[(size_t)i] = si;
      auto fit = segs[si]->fields.find(field_id);
      if (fit == segs[si]->fields.end() || !fit->second.d_btiles) break;
      const FieldData& f = fit->second;
      if (f.h_ord_to_doc.empty()) {
        if (local < (int64_t)f.n_vec) row_of[(size_t)i] = local;
      } else {
        auto it = std::lower_bound(f.h_ord_to_doc.begin(), f.h_ord_to_doc.end(), (int32_t)local);
        if (it != f.h_ord_to_doc.end() && *it == (int32_t)local) row_of[(size_t)i] = it - f.h_ord_to_doc.begin();
      }
      break;
    }
    if (seg_of[(size_t)i] < 0) return fail(NRTGPU_ERR_INVALID_ARG, "hit %d (doc %d) is outside every segment", i, docs[i]);
  }
  Slot* slot = nullptr;
  acquire_slot(ctx, &slot);
  struct Guard { nrtgpu_ctx* c; Slot* s; ~Guard() { release_slot(c, s); } } guard{ctx, slot};
  std::lock_guard<std::mutex> gpu(ctx->gpu_mu);
  hipStream_t st = slot->stream;
  std::vector<float> combined((size_t)n);
  auto on_device = [&]() -> int {
    if (ctx->last_turn) HIP_TRY(hipStreamWaitEvent(st, ctx->last_turn, 0));
    Carver wc;
    const size_t o_q = wc.take(qpad.size()), o_rows = wc.take((size_t)n * 8 + 8), o_first = wc.take((size_t)n * 4 + 4),
                 o_out = wc.take((size_t)n * 4 + 4);
    if (int rc = slot->d_work.reserve(wc.off)) return rc;
    char* wb = (char*)slot->d_work.p;
    HIP_TRY(hipMemcpyAsync(wb + o_q, qpad.data(), qpad.size(), hipMemcpyHostToDevice, st));
    for (int si = 0; si < n_segs; ++si) {
      std::vector<int> idx;
      for (int i = 0; i < n; ++i)
        if (seg_of[(size_t)i] == si) idx.push_back(i);
      if (idx.empty()) continue;
      auto fit = segs[si]->fields.find(field_id);
      const FieldData* f = (fit != segs[si]->fields.end() && fit->second.d_btiles) ? &fit->second : nullptr;
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
      launch_rescore_byte_vectors(st, f->d_btiles, f->d_bnorm2, dim, wb + o_q, qn, sim, boost, (const int64_t*)(wb + o_rows),
                                  (const float*)(wb + o_first), (int32_t)idx.size(), query_weight, rescore_weight, (float*)(wb + o_out));
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

// Needs no device: the one statement of the byte scores (plan.h), as the kernel compiles it.
extern "C" int nrtgpu_byte_vector_score(int32_t sim, int32_t dim, int32_t dot, int32_t q_norm2, int32_t v_norm2, float* out) {
  if (!out) return fail(NRTGPU_ERR_INVALID_ARG, "NULL argument");
  if (sim < 0 || sim > 3 || dim <= 0 || dim > 2048) return fail(NRTGPU_ERR_INVALID_ARG, "byte vector score: sim in 0..3 and dim in 1..2048 expected");
  const int32_t lim = dim * 128 * 128;   // what `dim` int8 pairs can reach
  if (q_norm2 < 0 || v_norm2 < 0 || q_norm2 > lim || v_norm2 > lim || dot > lim || dot < -lim)
    return fail(NRTGPU_ERR_INVALID_ARG, "byte vector score: |dot|, |q|^2 and |v|^2 of %d int8 pairs are at most %d", dim, lim);
  *out = knn_byte_score(sim, dim, dot, q_norm2, v_norm2);
  return NRTGPU_OK;
}
