// vectors_bytes.cpp -- exact search over byte (int8) vector fields: ExactByteVectorQuery and the `knn` request path over a byte field.
//
// The host side of knn_bytes.hip, beside knn_search (vectors.cpp) and a fraction of it: the pass over the rows returns RESULTS
// (integers from the i8 matrix cores, mapped to score bits by plan.h: knn_byte_score), so there are no error bounds, no
// rescoring, no certificate and no second pass here -- only the rounds that tighten theta and the selection they share with the
// float search (knn.hip: knn_select_kernel<false>).  The call's description, the leaf walk, the accept table, the field check,
// turn-taking, the timed launches, the rounds, the redo of an overflowed pass, the statistics and the unpacking are the float
// search's own code (runtime_internal.h: KnnCall, knn_walk_leaves, KnnRun, ...), as is the rescorers' host path further down.
#include "runtime_internal.h"

// nq queries in the matrix instruction's operand order (knn_bytes.hip): [step][panel][lane] x 16 bytes, zeros behind the field's
// dimension and behind the last query
static void stage_byte_panel(char* dst, const int8_t* queries, int nq, int32_t dim, int32_t steps, int panels) {
  memset(dst, 0, (size_t)steps * panels * 1024);
  for (int q = 0; q < nq; ++q) {
    const int8_t* src = queries + (size_t)q * dim;
    const int p = q >> 4, j = q & 15;
    for (int32_t d0 = 0; d0 < dim; d0 += 16) {
      const int32_t s = d0 >> 6, kk = (d0 >> 4) & 3;
      memcpy(dst + (((size_t)s * panels + p) * 64 + (size_t)(kk * 16 + j)) * 16, src + d0, (size_t)std::min(16, dim - d0));
    }
  }
}

int nrtgpu::rt::knn_bytes_search(nrtgpu_ctx* ctx, const KnnCall& call) {
  forget_foreign_hip_error();
  // Members with a filter and a threshold EACH (!call.one_filter()) change two inputs of the device: a table of accept sets per
  // (leaf, query) in place of the leaf's one, and the queries' own thresholds in place of the launch's one (knn_bytes.hip:
  // knn_bytes_requests_kernel).  Scores stay unboosted.
  const nrtgpu_seg* const* segs = call.segs;
  const int8_t* queries = (const int8_t*)call.queries;
  const int32_t n_segs = call.n_segs, n_queries = call.n_queries, dim = call.dim, sim = call.sim;
  if (!ctx || !queries || !call.out || (n_segs > 0 && !segs)) return fail(NRTGPU_ERR_INVALID_ARG, "NULL argument");
  const int32_t k = call.k_max();
  // (a request's boost was checked with the request; here: the boost of an ExactByteVectorQuery or of a uniform request)
  if (int rc = knn_check_scalars(n_queries <= 0 || n_segs < 0, k, dim, sim, &call.ask.boosts[0])) return rc;
  // |q|^2 of every query; cosine refuses a zero query as the reference does (validateVectorForSearch, VectorFieldDef.java:853-861)
  std::vector<int32_t> qn2((size_t)n_queries);
  if (int rc = byte_queries_stage(queries, n_queries, dim, sim, nullptr, qn2.data())) return rc;
  NRT_CHECK_DEADLINE("before the vector search started");
  HIP_TRY(hipSetDevice(ctx->device));
  for (int si = 0; si < n_segs; ++si)
    if (!segs[si]) return fail(NRTGPU_ERR_STATE, "segment %d missing or not sealed", si);
  SegReadLocks content(segs, n_segs);  // liveDocs / masks stay as they are until the kernels have finished
  for (int si = 0; si < n_segs; ++si) {
    if (!segs[si]->sealed) return fail(NRTGPU_ERR_STATE, "segment %d missing or not sealed", si);
    auto fit = segs[si]->fields.find(call.field_id);
    if (fit != segs[si]->fields.end())
      if (int rc = knn_check_field(true, si, call.field_id, fit->second, dim, kHintSearchFloat)) return rc;
  }
  if (call.shared_mask() != 0) {   // a selective filter: score only the rows it accepts (vectors_gather.cpp)
    bool gather = false;
    int64_t estimate = 0;
    if (int rc = knn_gather_route(ctx, call, &gather, &estimate)) return rc;
    if (gather) return knn_gather_run(ctx, call, qn2.data(), estimate);
  }
  const bool table = !call.one_filter();
  const uint32_t k_stride = round_up((uint32_t)k, 16);
  const float score_boost = call.score_boost();   // the knn request: min_score tests the unboosted score, the boost comes afterwards
  Slot* slot = nullptr;
  acquire_slot(ctx, &slot);
  SlotGuard guard{ctx, slot};
  KnnRun run{ctx, slot};
  hipStream_t st = slot->stream;
  Carver wc;
  // the head [o_p, o_th) is staged in pinned memory laid out alike: one copy per panel
  const size_t o_p = wc.take(knn_bytes_panel_bytes(dim, kKnnMaxQ)), o_qn = wc.take(kKnnMaxQ * 4);
  const size_t o_leaves = wc.take((size_t)std::max(n_segs, 1) * sizeof(DKnnBytesLeaf));
  const size_t o_ms = wc.take(table ? kKnnMaxQ * 4 : 8);   // table: the members' thresholds on the unboosted score (0: none)
  const size_t o_acc = wc.take(table ? (size_t)std::max(n_segs, 1) * kKnnAcceptCols * sizeof(uint64_t*) : 8);   // the accept table (plan.h)
  const size_t o_th = wc.take(kKnnMaxQ * 8);
  const size_t o_tk = wc.take((size_t)kKnnMaxQ * k_stride * 8), o_tc = wc.take(kKnnMaxQ * 4);
  const size_t o_cc = wc.take(kKnnMaxQ * 4), o_ov = wc.take(64);
  const size_t o_cd = wc.take((size_t)kKnnMaxQ * kKnnCap * 8);
  if (int rc = slot->d_work.reserve(wc.off)) return rc;
  const size_t oh_cnt = o_tc - o_tk, oh_ov = o_ov - o_tk;   // keys, counts and the overflow flag come back in one copy
  if (int rc = slot->h_out.reserve(o_cd - o_tk)) return rc;
  if (int rc = slot->h_aux.reserve(o_th)) return rc;
  char* wb = (char*)slot->d_work.p;
  char* ho = (char*)slot->h_out.p;
  char* hs = (char*)slot->h_aux.p;
  // the leaves' tiles of 16 rows, numbered through: ONE launch walks every leaf
  DKnnBytesLeaf* hleaves = (DKnnBytesLeaf*)(hs + o_leaves);
  float* ms = (float*)(hs + o_ms);
  const uint64_t* const* d_acc = table ? (const uint64_t* const*)(wb + o_acc) : nullptr;
  int32_t n_kleaves = 0;
  int64_t total_tiles = 0, total_rows = 0, live_vectors = 0;
  if (int rc = knn_walk_leaves(call, call.shared_mask(), [&](const KnnLeaf& at) -> int {
        DKnnBytesLeaf l{};
        l.tiles = at.f->d_btiles;
        l.vnorm2 = at.f->d_bnorm2;
        l.ord_to_doc = at.f->d_ord_to_doc;
        l.accept = at.accept;
        l.accept_of = d_acc ? d_acc + (size_t)at.index * kKnnAcceptCols : nullptr;
        l.tile_begin = at.tile_begin;
        l.n_rows = at.f->n_vec;
        l.doc_base = at.doc_base;
        hleaves[n_kleaves++] = l;
        live_vectors += at.live;
        total_tiles = at.tile_begin + (((int64_t)at.f->n_vec + 15) >> 4);
        total_rows = at.row_begin + at.f->n_vec;
        return NRTGPU_OK;
      }))
    return rc;
  const int32_t steps = knn_bytes_steps(dim);
  static const int64_t kFirstRound = (int64_t)(1 << 16) >> 4;   // tiles of the first round: every row takes a slot of the list
  for (int q0 = 0; q0 < n_queries; q0 += kKnnMaxQ) {
    const int nq = std::min(kKnnMaxQ, n_queries - q0);
    if (deadline_passed(g_deadline_ns)) {   // between two passes over the rows: nothing of the next one has been launched
      (void)hipStreamSynchronize(st);
      return fail(NRTGPU_ERR_TIMEOUT, "deadline passed between two passes over the rows (%d of %d queries answered)", q0, n_queries);
    }
    const int panels = nq > 16 ? 4 : 1;
    stage_byte_panel(hs + o_p, queries + (size_t)q0 * dim, nq, dim, steps, panels);
    memset(hs + o_qn, 0, kKnnMaxQ * 4);
    memcpy(hs + o_qn, qn2.data() + q0, (size_t)nq * 4);
    if (table) {   // the members' thresholds, and liveDocs & the member's filter per (leaf, member)
      for (int q = 0; q < kKnnMaxQ; ++q) ms[q] = q < nq ? call.ask.min_score(q0 + q) : 0.0f;
      if (int rc = knn_stage_accept_table(call, q0, nq, (const uint64_t**)(hs + o_acc))) return rc;
    }
    HIP_TRY(hipMemcpyAsync(wb + o_p, hs + o_p, (size_t)steps * panels * 1024, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(wb + o_qn, hs + o_qn, o_th - o_qn, hipMemcpyHostToDevice, st));   // |q|^2, leaf table (thresholds, accept table)
    // One pass over the rows of every leaf in KnnRun::tile_rounds' rounds, always nominating.  Rows in rising order of similarity
    // could overflow a list: the selection flags that and the panel is redone in rounds no longer than the list (`safe`).
    auto pass = [&](int safe) -> int {
      if (int rc = run.take_turn()) return rc;
      HIP_TRY(hipMemsetAsync(wb + o_th, 0, o_cd - o_th, st));  // theta, the running top-k, counters, flag
      auto launch = [&](int64_t t, int64_t te, uint32_t blocks, int32_t append_only) -> int {
        return run.timed_launch("knn_bytes", [&]() {
          return launch_knn_bytes(st, blocks, (const DKnnBytesLeaf*)(wb + o_leaves), n_kleaves, dim, t, te, wb + o_p, (const int32_t*)(wb + o_qn),
                                  nq, sim, score_boost, table ? 0.0f : call.ask.min_scores[0], (const unsigned long long*)(wb + o_th),
                                  (uint64_t*)(wb + o_cd), (uint32_t*)(wb + o_cc), kKnnCap, append_only,
                                  table ? (const float*)(wb + o_ms) : nullptr);
        });
      };
      if (int rc = run.tile_rounds(total_tiles, kFirstRound, kKnnCap, true, safe, launch, [&]() {
            launch_knn_select(st, (uint32_t)nq, (uint64_t*)(wb + o_tk), (uint32_t*)(wb + o_tc), k_stride, (uint32_t)k, (const uint64_t*)(wb + o_cd),
                              (uint32_t*)(wb + o_cc), kKnnCap, (unsigned long long*)(wb + o_th), (uint32_t*)(wb + o_ov));
          }))
        return rc;
      if (int rc = run.end_turn()) return rc;
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(ho, wb + o_tk, o_ov + 4 - o_tk, hipMemcpyDeviceToHost, st));   // the answer, its counts, the flag
      HIP_TRY(hipStreamSynchronize(st));
      return NRTGPU_OK;
    };
    if (int rc = run.redo_on_overflow((const uint32_t*)(ho + oh_ov), "knn_bytes: candidate list overflow in a bounded round", pass)) return rc;
    run.add_stats(total_rows, 0, false);
    knn_unpack_topdocs((const uint64_t*)ho, (const uint32_t*)(ho + oh_cnt), k_stride, nq, true, live_vectors, call.knn_request, call.ask.from(q0),
                       &call.out[q0]);
  }
  return NRTGPU_OK;
}

// An ExactByteVectorQuery per query / one knn request for all of them: a stride-0 view of one value (runtime_internal.h: KnnAsk).
extern "C" int nrtgpu_knn_exact_bytes(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                      int32_t field_id, int32_t sim, const int8_t* queries, int32_t n_queries, int32_t dim, int32_t k,
                                      float boost, nrtgpu_topdocs* out) {
  const KnnUniform one{k, 0, boost, 0.0f};
  return knn_bytes_search(ctx, KnnCall{segs, doc_bases, n_segs, field_id, /*bytes*/ true, queries, n_queries, dim, sim, /*knn_request*/ false, one.ask(), out});
}

extern "C" int nrtgpu_knn_search_bytes(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                       int32_t field_id, int32_t sim, const int8_t* queries, int32_t n_queries, int32_t dim, int32_t k,
                                       float boost, int32_t filter_mask, float min_score, nrtgpu_topdocs* out) {
  if (filter_mask < 0 || !(min_score >= 0.0f) || !(boost > 0.0f))
    return fail(NRTGPU_ERR_INVALID_ARG, "knn search: filter_mask >= 0, min_score >= 0 and boost > 0 expected");
  const KnnUniform one{k, filter_mask, boost, min_score};
  return knn_bytes_search(ctx, KnnCall{segs, doc_bases, n_segs, field_id, /*bytes*/ true, queries, n_queries, dim, sim, /*knn_request*/ true, one.ask(), out});
}

// ---- the rescorers over a byte field: QueryRescore (rescore/QueryRescore.java:40-57) with the field's ExactByteVectorQuery
// (VectorFieldDef.java:842) in the rescore slot -- nrtgpu_rescore_byte_vectors here, the tail of nrtgpu_search_hybrid_bytes_batch in
// search.cpp: search_hybrid_impl.  Both run the float rescorers' host code (vectors.cpp: rescore_hits_impl, stage_rescore_inputs);
// here is what only a byte field asks: the refusals and the queries in piece order ------------------------------------------------
// What the byte entries ask of their scalars, in knn_bytes_search's order.
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
  if (int rc = stage_rescore_inputs(segs, doc_bases, n_segs, field_id, true, sim, query, 1, dim, nullptr, qpad.data(), &qn)) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  for (int si = 0; si < n_segs; ++si)
    if (!segs[si]) return fail(NRTGPU_ERR_INVALID_ARG, "segment %d is NULL", si);
  if (int rc = knn_check_leaves(segs, n_segs, field_id, true, dim, kHintRescoreFloat)) return rc;
  const RescoreKind kind{[](const FieldData& f) -> const void* { return f.d_btiles; }, qpad.data(), qpad.size(),
                         [&](hipStream_t st, const FieldData& f, const void* d_query, const int64_t* d_rows, const float* d_first, int32_t m, float* d_out) {
                           launch_rescore_byte_vectors(st, f.d_btiles, f.d_bnorm2, dim, d_query, qn, sim, boost, d_rows, d_first, m, query_weight,
                                                       rescore_weight, d_out);
                         }};
  return rescore_hits_impl(ctx, segs, doc_bases, n_segs, field_id, kind, docs, first_scores, n, query_weight, window, out);
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
