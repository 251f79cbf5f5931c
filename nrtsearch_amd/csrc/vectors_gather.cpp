// vectors_gather.cpp -- the GATHER route of the filtered knn entries (nrtgpu_knn_search, nrtgpu_knn_search_bytes).
//
// The full pass of either entry tests the filter INSIDE a pass over every row of the field: its cost does not depend on how few
// rows the filter accepts.  Here the accepted rows are listed on the device once per call (knn.hip: knn_accept_rows_kernel), and
// every panel of 64 queries scores exactly those with final score bits (knn_gather_score_kernel: knn_score_seq, the oracle's
// order; knn_gather_bytes_kernel: the rescorers' integer walk + plan.h: knn_byte_score) into one slot per row of the candidate
// lists the full passes use, which their selection (knn_select_kernel<false>) reduces to the top k.  Turn-taking, timed launches,
// statistics and unpacking are the full passes' own (runtime_internal.h: KnnRun, knn_unpack_topdocs); argument checks, refusals,
// locks and the deadline check on entry happen in knn_impl / knn_bytes_impl before the route is decided.
#include "runtime_internal.h"

static const int kKnnGatherMaxQ = 64;   // queries per pass over the accepted rows (the full passes' panel)

extern "C" int nrtgpu_set_knn_gather(nrtgpu_ctx* ctx, int32_t max_accept_permille) {
  if (!ctx || max_accept_permille < 0 || max_accept_permille > 1000)
    return fail(NRTGPU_ERR_INVALID_ARG, "knn gather: a context and a share of the rows in 0..1000 permille expected");
  ctx->knn_gather_permille.store(max_accept_permille, std::memory_order_relaxed);
  return NRTGPU_OK;
}

// the leaves of the call that hold rows of the field's element type
static const FieldData* gather_rows_of(const nrtgpu_seg* seg, const KnnGatherCall& call) {
  auto fit = seg->fields.find(call.field_id);
  if (fit == seg->fields.end() || fit->second.n_vec == 0) return nullptr;
  const FieldData& f = fit->second;
  return (call.bytes ? f.d_btiles != nullptr : f.d_vectors != nullptr) ? &f : nullptr;
}

int nrtgpu::rt::knn_gather_route(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs, const KnnGatherCall& call, bool* gather,
                                 int64_t* estimate) {
  *gather = false;
  *estimate = 0;
  const int64_t permille = ctx->knn_gather_permille.load(std::memory_order_relaxed);
  if (permille <= 0 || call.filter_mask == 0) return NRTGPU_OK;
  int64_t est = 0, rows = 0;
  for (int si = 0; si < n_segs; ++si) {
    const FieldData* f = gather_rows_of(segs[si], call);
    if (!f) continue;
    const uint64_t* accept = nullptr;
    int64_t docs = 0;
    if (int rc = accept_set_of(segs[si], call.filter_mask, 0, &accept, &docs)) return rc;
    est += std::min<int64_t>(docs, f->n_vec);
    rows += f->n_vec;
  }
  *estimate = est;
  // every accepted row gets a slot of one candidate list: no rounds, no theta between them
  *gather = est * 1000 <= permille * rows && est <= (int64_t)call.cap;
  return NRTGPU_OK;
}

// |q|^2 of the panel's float queries as knn_score_seq's cosine wants it (vectors.cpp: float_qnorm2's chain, every query its own
// element order); eight queries side by side: eight independent chains of dependent additions
static void gather_float_qnorm2(const float* queries, int nq, int dim, float* out) {
  for (int qb = 0; qb < nq; qb += 8) {
    const int nb = std::min(8, nq - qb);
    float s2[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const float* qv0 = queries + (size_t)qb * dim;
    {
#pragma clang fp contract(off)   // (x * x rounded, then added: never one fused operation, whatever the build's flags)
      for (int d = 0; d < dim; ++d)
        for (int j = 0; j < nb; ++j) {
          const float x = qv0[(size_t)j * dim + d];
          const float p2 = x * x;
          s2[j] = s2[j] + p2;
        }
    }
    for (int j = 0; j < nb; ++j) out[qb + j] = s2[j];
  }
}

int nrtgpu::rt::knn_gather_run(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                               const KnnGatherCall& call, int64_t estimate, nrtgpu_topdocs* out) {
  const int32_t k = call.k, dim = call.dim;
  const uint32_t k_stride = round_up((uint32_t)k, 16);
  if (estimate <= 0) {   // the filter accepts no row of the field: nothing to launch
    const std::vector<uint32_t> none((size_t)kKnnGatherMaxQ, 0u);
    for (int q0 = 0; q0 < call.n_queries; q0 += kKnnGatherMaxQ)
      knn_unpack_topdocs(nullptr, none.data(), k_stride, std::min(kKnnGatherMaxQ, call.n_queries - q0), k, true, 0, true, call.boost, &out[q0]);
    return NRTGPU_OK;
  }
  if (estimate > (int64_t)call.cap) return fail(NRTGPU_ERR_STATE, "knn gather: %lld rows for a list of %u", (long long)estimate, call.cap);
  const uint32_t max_rows = (uint32_t)estimate;
  const uint32_t list_cap = round_up(max_rows, 256);   // slots per candidate list: the rows the filter can accept, not the full pass's capacity
  Slot* slot = nullptr;
  acquire_slot(ctx, &slot);
  SlotGuard guard{ctx, slot};
  KnnRun run{ctx, slot};
  hipStream_t st = slot->stream;
  const size_t q_stride = call.bytes ? byte_query_stride(dim) : (size_t)dim * 4;
  Carver wc;
  // the head [o_q, o_th) is staged in pinned memory laid out alike: two copies per panel, no sync
  const size_t o_q = wc.take((size_t)kKnnGatherMaxQ * q_stride), o_qn = wc.take(kKnnGatherMaxQ * 4);
  const size_t o_leaves = wc.take((size_t)std::max(n_segs, 1) * sizeof(DKnnGatherLeaf));
  const size_t o_th = wc.take(kKnnGatherMaxQ * 8);
  const size_t o_tk = wc.take((size_t)kKnnGatherMaxQ * k_stride * 8), o_tc = wc.take(kKnnGatherMaxQ * 4);
  const size_t o_cc = wc.take(kKnnGatherMaxQ * 4), o_ov = wc.take(64);
  const size_t o_n = wc.take(64);   // the accepted rows, counted by the listing kernel (kept over the call's panels, like the list)
  const size_t o_list = wc.take((size_t)list_cap * 8);
  const size_t o_cd = wc.take((size_t)kKnnGatherMaxQ * list_cap * 8);
  if (int rc = slot->d_work.reserve(wc.off)) return rc;
  const size_t oh_cnt = o_tc - o_tk, oh_ov = o_ov - o_tk, oh_n = o_n - o_tk;   // keys, counts, the flag and the row count come back in one copy
  if (int rc = slot->h_out.reserve(o_list - o_tk)) return rc;
  if (int rc = slot->h_aux.reserve(o_th)) return rc;
  char* wb = (char*)slot->d_work.p;
  char* ho = (char*)slot->h_out.p;
  char* hs = (char*)slot->h_aux.p;
  DKnnGatherLeaf* hleaves = (DKnnGatherLeaf*)(hs + o_leaves);
  int32_t n_leaves = 0;
  int64_t total_rows = 0;
  for (int si = 0; si < n_segs; ++si) {
    const FieldData* f = gather_rows_of(segs[si], call);
    if (!f) continue;
    const uint64_t* accept = nullptr;
    if (int rc = accept_set_of(segs[si], call.filter_mask, 0, &accept)) return rc;
    DKnnGatherLeaf l{};
    l.rows = call.bytes ? (const void*)f->d_btiles : (const void*)f->d_vectors;
    l.vnorm2 = call.bytes ? f->d_bnorm2 : nullptr;
    l.ord_to_doc = f->d_ord_to_doc;
    l.accept = accept;
    l.row_begin = total_rows;
    l.n_rows = f->n_vec;
    l.doc_base = doc_bases ? doc_bases[si] : 0;
    l.max_doc = segs[si]->max_doc;
    hleaves[n_leaves++] = l;
    total_rows += f->n_vec;
  }
  int64_t n_accepted = -1;   // known once the first panel has come back
  for (int q0 = 0; q0 < call.n_queries; q0 += kKnnGatherMaxQ) {
    const int nq = std::min(kKnnGatherMaxQ, call.n_queries - q0);
    if (deadline_passed(g_deadline_ns)) {   // between two passes over the rows: nothing of the next one has been launched
      (void)hipStreamSynchronize(st);
      return fail(NRTGPU_ERR_TIMEOUT, "deadline passed between two passes over the rows (%d of %d queries answered)", q0, call.n_queries);
    }
    memset(hs + o_qn, 0, kKnnGatherMaxQ * 4);
    if (call.bytes) {   // piece order (knn_bytes.hip): the query itself, zero-padded to whole 64-dimension steps
      if (int rc = byte_queries_stage((const int8_t*)call.queries + (size_t)q0 * dim, nq, dim, call.sim, (int8_t*)(hs + o_q), nullptr)) return rc;
      memcpy(hs + o_qn, call.byte_qnorm2 + q0, (size_t)nq * 4);
    } else {
      memcpy(hs + o_q, (const float*)call.queries + (size_t)q0 * dim, (size_t)nq * q_stride);
      if (call.sim == 0) gather_float_qnorm2((const float*)(hs + o_q), nq, dim, (float*)(hs + o_qn));   // (only the cosine reads |q|^2)
    }
    HIP_TRY(hipMemcpyAsync(wb + o_q, hs + o_q, (size_t)nq * q_stride, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(wb + o_qn, hs + o_qn, o_th - o_qn, hipMemcpyHostToDevice, st));   // |q|^2, leaf table
    if (int rc = run.take_turn()) return rc;
    HIP_TRY(hipMemsetAsync(wb + o_th, 0, o_n - o_th, st));   // theta, the top k, counters, flag
    if (q0 == 0) {   // the call's row list: once, every panel scores it
      HIP_TRY(hipMemsetAsync(wb + o_n, 0, 64, st));
      if (const int e = launch_knn_accept_rows(st, (const DKnnGatherLeaf*)(wb + o_leaves), n_leaves, total_rows, (uint64_t*)(wb + o_list),
                                               (uint32_t*)(wb + o_n), list_cap))
        return fail(NRTGPU_ERR_HIP, "knn_accept_rows launch: %s", hipGetErrorString((hipError_t)e));
    }
    if (int rc = run.timed_launch(call.bytes ? "knn_gather_bytes" : "knn_gather_score", [&]() {
          if (call.bytes)
            return launch_knn_gather_bytes(st, (const DKnnGatherLeaf*)(wb + o_leaves), (const uint64_t*)(wb + o_list), (const uint32_t*)(wb + o_n),
                                           max_rows, dim, wb + o_q, (const int32_t*)(wb + o_qn), nq, call.sim, 1.0f, call.min_score,
                                           (uint64_t*)(wb + o_cd), (uint32_t*)(wb + o_cc), list_cap);
          return launch_knn_gather_score(st, (const DKnnGatherLeaf*)(wb + o_leaves), (const uint64_t*)(wb + o_list), (const uint32_t*)(wb + o_n),
                                         max_rows, dim, (const float*)(wb + o_q), (const float*)(wb + o_qn), nq, call.sim, 1.0f, call.min_score,
                                         (uint64_t*)(wb + o_cd), (uint32_t*)(wb + o_cc), list_cap);
        }))
      return rc;
    launch_knn_select(st, (uint32_t)nq, (uint64_t*)(wb + o_tk), (uint32_t*)(wb + o_tc), k_stride, (uint32_t)k, (const uint64_t*)(wb + o_cd),
                      (uint32_t*)(wb + o_cc), list_cap, (unsigned long long*)(wb + o_th), (uint32_t*)(wb + o_ov));
    if (int rc = run.end_turn()) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(ho, wb + o_tk, o_n + 4 - o_tk, hipMemcpyDeviceToHost, st));   // the answer, its counts, the flag, the rows listed
    HIP_TRY(hipStreamSynchronize(st));
    const uint32_t listed = *(const uint32_t*)(ho + oh_n);
    if (listed > max_rows || *(const uint32_t*)(ho + oh_ov) != 0u)   // (the estimate is an upper bound: a list cannot overflow)
      return fail(NRTGPU_ERR_HIP, "knn gather: %u rows listed where at most %u were expected", listed, max_rows);
    n_accepted = (int64_t)listed;
    run.add_stats(n_accepted, 0, false);
    knn_unpack_topdocs((const uint64_t*)ho, (const uint32_t*)(ho + oh_cnt), k_stride, nq, k, true, 0, true, call.boost, &out[q0]);
  }
  return NRTGPU_OK;
}
