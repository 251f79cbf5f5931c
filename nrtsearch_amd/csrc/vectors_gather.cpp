// vectors_gather.cpp -- the GATHER route of the filtered knn entries (nrtgpu_knn_search, nrtgpu_knn_search_bytes).
//
// The full pass of either entry tests the filter INSIDE a pass over every row of the field: its cost does not depend on how few
// rows the filter accepts.  Here the accepted rows are listed on the device once per call (knn.hip: knn_accept_rows_kernel), and
// every panel of 64 queries scores exactly those with final score bits (knn_gather_score_kernel: knn_score_seq, the oracle's
// order; knn_gather_bytes_kernel: the rescorers' integer walk + plan.h: knn_byte_score) into one slot per row of the candidate
// lists the full passes use, which their selection (knn_select_kernel<false>) reduces to the top k.  The call's description, the
// leaf walk, turn-taking, timed launches, statistics and unpacking are the full passes' own (runtime_internal.h: KnnCall,
// knn_walk_leaves, KnnRun, knn_unpack_topdocs); argument checks, refusals, locks and the deadline check on entry happen in
// knn_search / knn_bytes_search before the route is decided.
#include "runtime_internal.h"

extern "C" int nrtgpu_set_knn_gather(nrtgpu_ctx* ctx, int32_t max_accept_permille) {
  if (!ctx || max_accept_permille < 0 || max_accept_permille > 1000)
    return fail(NRTGPU_ERR_INVALID_ARG, "knn gather: a context and a share of the rows in 0..1000 permille expected");
  ctx->knn_gather_permille.store(max_accept_permille, std::memory_order_relaxed);
  return NRTGPU_OK;
}

int nrtgpu::rt::knn_gather_route(nrtgpu_ctx* ctx, const KnnCall& call, bool* gather, int64_t* estimate) {
  *gather = false;
  *estimate = 0;
  const int64_t permille = ctx->knn_gather_permille.load(std::memory_order_relaxed);
  if (permille <= 0 || call.shared_mask() == 0) return NRTGPU_OK;
  int64_t est = 0, rows = 0;
  if (int rc = knn_walk_leaves(call, call.shared_mask(), [&](const KnnLeaf& at) -> int {
        est += std::min<int64_t>(at.accept_docs, at.f->n_vec);
        rows += at.f->n_vec;
        return NRTGPU_OK;
      }))
    return rc;
  *estimate = est;
  // every accepted row gets a slot of one candidate list: no rounds, no theta between them
  *gather = est * 1000 <= permille * rows && est <= (int64_t)kKnnCap;
  return NRTGPU_OK;
}

int nrtgpu::rt::knn_gather_run(nrtgpu_ctx* ctx, const KnnCall& call, const int32_t* byte_qnorm2, int64_t estimate) {
  const int32_t k = call.k_max(), dim = call.dim, n_segs = call.n_segs;
  const float min_score = call.ask.min_scores[0];
  const uint32_t k_stride = round_up((uint32_t)k, 16);
  if (estimate <= 0) {   // the filter accepts no row of the field: nothing to launch
    const std::vector<uint32_t> none((size_t)kKnnMaxQ, 0u);
    for (int q0 = 0; q0 < call.n_queries; q0 += kKnnMaxQ)
      knn_unpack_topdocs(nullptr, none.data(), k_stride, std::min(kKnnMaxQ, call.n_queries - q0), true, 0, true, call.ask, &call.out[q0]);
    return NRTGPU_OK;
  }
  if (estimate > (int64_t)kKnnCap) return fail(NRTGPU_ERR_STATE, "knn gather: %lld rows for a list of %u", (long long)estimate, kKnnCap);
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
  const size_t o_q = wc.take((size_t)kKnnMaxQ * q_stride), o_qn = wc.take(kKnnMaxQ * 4);
  const size_t o_leaves = wc.take((size_t)std::max(n_segs, 1) * sizeof(DKnnGatherLeaf));
  const size_t o_th = wc.take(kKnnMaxQ * 8);
  const size_t o_tk = wc.take((size_t)kKnnMaxQ * k_stride * 8), o_tc = wc.take(kKnnMaxQ * 4);
  const size_t o_cc = wc.take(kKnnMaxQ * 4), o_ov = wc.take(64);
  const size_t o_n = wc.take(64);   // the accepted rows, counted by the listing kernel (kept over the call's panels, like the list)
  const size_t o_list = wc.take((size_t)list_cap * 8);
  const size_t o_cd = wc.take((size_t)kKnnMaxQ * list_cap * 8);
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
  if (int rc = knn_walk_leaves(call, call.shared_mask(), [&](const KnnLeaf& at) -> int {
        DKnnGatherLeaf l{};
        l.rows = call.bytes ? (const void*)at.f->d_btiles : (const void*)at.f->d_vectors;
        l.vnorm2 = call.bytes ? at.f->d_bnorm2 : nullptr;
        l.ord_to_doc = at.f->d_ord_to_doc;
        l.accept = at.accept;
        l.row_begin = at.row_begin;
        l.n_rows = at.f->n_vec;
        l.doc_base = at.doc_base;
        l.max_doc = at.seg->max_doc;
        hleaves[n_leaves++] = l;
        total_rows = at.row_begin + at.f->n_vec;
        return NRTGPU_OK;
      }))
    return rc;
  int64_t n_accepted = -1;   // known once the first panel has come back
  for (int q0 = 0; q0 < call.n_queries; q0 += kKnnMaxQ) {
    const int nq = std::min(kKnnMaxQ, call.n_queries - q0);
    if (deadline_passed(g_deadline_ns)) {   // between two passes over the rows: nothing of the next one has been launched
      (void)hipStreamSynchronize(st);
      return fail(NRTGPU_ERR_TIMEOUT, "deadline passed between two passes over the rows (%d of %d queries answered)", q0, call.n_queries);
    }
    memset(hs + o_qn, 0, kKnnMaxQ * 4);
    if (call.bytes) {   // piece order (knn_bytes.hip): the query itself, zero-padded to whole 64-dimension steps
      if (int rc = byte_queries_stage((const int8_t*)call.queries + (size_t)q0 * dim, nq, dim, call.sim, (int8_t*)(hs + o_q), nullptr)) return rc;
      memcpy(hs + o_qn, byte_qnorm2 + q0, (size_t)nq * 4);
    } else {
      memcpy(hs + o_q, (const float*)call.queries + (size_t)q0 * dim, (size_t)nq * q_stride);
      if (call.sim == 0) knn_query_stats((const float*)(hs + o_q), nq, dim, (float*)(hs + o_qn), nullptr, nullptr);   // (only the cosine reads |q|^2)
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
                                           max_rows, dim, wb + o_q, (const int32_t*)(wb + o_qn), nq, call.sim, 1.0f, min_score,
                                           (uint64_t*)(wb + o_cd), (uint32_t*)(wb + o_cc), list_cap);
          return launch_knn_gather_score(st, (const DKnnGatherLeaf*)(wb + o_leaves), (const uint64_t*)(wb + o_list), (const uint32_t*)(wb + o_n),
                                         max_rows, dim, (const float*)(wb + o_q), (const float*)(wb + o_qn), nq, call.sim, 1.0f, min_score,
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
    knn_unpack_topdocs((const uint64_t*)ho, (const uint32_t*)(ho + oh_cnt), k_stride, nq, true, 0, true, call.ask.from(q0), &call.out[q0]);
  }
  return NRTGPU_OK;
}
