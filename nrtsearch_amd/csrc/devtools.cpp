// devtools.cpp -- measurement helpers that are NOT part of the product ABI: compiled into the library only with
// -DNRTGPU_DEV (python -m nrtsearch_amd.build --dev writes libnrtgpu_dev.so); declared in include/nrtgpu_dev.h.
#include "runtime_internal.h"
#include "../../include/nrtgpu_dev.h"

// Closed-loop load generator (diagnostics; SURVEY 8d's "C concurrent clients"): `clients` native threads each
// issue one query at a time through nrtgpu_search_bm25_coalesced for duration_ms, cycling through `queries`.
// out[0] = completed queries, out[1] = seconds, out[2] = p50 latency ms, out[3] = p99 latency ms.
extern "C" int nrtgpu_bench_closed_loop(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases,
                                        int32_t n_segs, const nrtgpu_bm25_query* queries, int32_t n_queries,
                                        int32_t clients, int32_t duration_ms, double* out4) {
  if (!ctx || !queries || !out4 || n_queries <= 0 || clients <= 0 || duration_ms <= 0)
    return fail(NRTGPU_ERR_INVALID_ARG, "bad closed-loop arguments");
  std::vector<std::vector<float>> lat((size_t)clients);
  std::vector<int> rcs((size_t)clients, 0);
  std::vector<std::string> errs((size_t)clients);
  const auto t_begin = std::chrono::steady_clock::now();
  const auto t_stop = t_begin + std::chrono::milliseconds(duration_ms);
  auto client = [&](int c) {
    int32_t kmax = 1;
    for (int i = 0; i < n_queries; ++i) kmax = std::max(kmax, queries[i].k);
    std::vector<int32_t> docs((size_t)kmax);
    std::vector<float> scores((size_t)kmax);
    size_t i = (size_t)c * 7919u;
    for (;;) {
      const auto t0 = std::chrono::steady_clock::now();
      if (t0 >= t_stop) break;
      nrtgpu_topdocs o{};
      o.capacity = kmax;
      o.docs = docs.data();
      o.scores = scores.data();
      const int rc = nrtgpu_search_bm25_coalesced(ctx, segs, doc_bases, n_segs, &queries[i % (size_t)n_queries], &o);
      if (rc != 0) {
        rcs[(size_t)c] = rc;
        errs[(size_t)c] = g_last_error;
        break;
      }
      lat[(size_t)c].push_back(std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count());
      ++i;
    }
  };
  std::vector<std::thread> pool;
  for (int c = 0; c < clients; ++c) pool.emplace_back(client, c);
  for (auto& t : pool) t.join();
  const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
  for (int c = 0; c < clients; ++c)
    if (rcs[(size_t)c] != 0) return fail(rcs[(size_t)c], "client %d: %s", c, errs[(size_t)c].c_str());
  std::vector<float> all;
  for (auto& v : lat) all.insert(all.end(), v.begin(), v.end());
  std::sort(all.begin(), all.end());
  out4[0] = (double)all.size();
  out4[1] = secs;
  out4[2] = all.empty() ? 0.0 : all[all.size() / 2];
  out4[3] = all.empty() ? 0.0 : all[(size_t)((double)all.size() * 0.99)];
  return NRTGPU_OK;
}


// Test hook (include/nrtgpu_dev.h): the exact vector search's certification bounds as the search computes them (host_math.h:
// knn_bound32 / knn_bound16 / knn_sketch_scale; plan.h: knn_result_upper / knn_estimate_lower).  No context, no device work.
extern "C" int nrtgpu_debug_knn_bounds(int32_t sim, int32_t dim, double q_norm2, double q_l1, float q_absmax, double nv_max, double nv_min,
                                       float rows_absmax, float score_boost, double m, double s, double* out10) {
  if (!out10 || sim < 0 || sim > 3 || dim <= 0 || (dim & 15)) return fail(NRTGPU_ERR_INVALID_ARG, "bad knn_bounds arguments");
  float q_scale = 1.0f, rows_scale = 1.0f;
  const bool q_ok = hostmath::knn_sketch_scale(q_absmax, &q_scale), rows_ok = hostmath::knn_sketch_scale(rows_absmax, &rows_scale);
  const double e_rel = (double)hostmath::knn_e_rel(), b = (double)score_boost;
  const float e32 = hostmath::knn_bound32(sim, dim, q_norm2, nv_max, b);
  const float e16 = hostmath::knn_bound16(sim, dim, q_norm2, q_l1, 1.0 / (double)q_scale, nv_max, nv_min, 1.0 / (double)rows_scale, b);
  out10[0] = (double)e32;
  out10[1] = (double)e16;
  out10[2] = knn_result_upper(sim, m, (double)e32, e_rel, b);
  out10[3] = knn_result_upper(sim, m, (double)e16, e_rel, b);
  out10[4] = knn_estimate_lower(sim, s, (double)e32, e_rel, b);
  out10[5] = knn_estimate_lower(sim, s, (double)e16, e_rel, b);
  out10[6] = (double)q_scale;
  out10[7] = (double)rows_scale;
  out10[8] = q_ok ? 1.0 : 0.0;
  out10[9] = rows_ok ? 1.0 : 0.0;
  return NRTGPU_OK;
}

// Test hook (include/nrtgpu_dev.h): a panel's sorted keys -> its members' nrtgpu_topdocs as the knn request entries unpack them
// (vectors.cpp: knn_unpack_topdocs with a k and a boost per member).  No context, no device work.
extern "C" int nrtgpu_debug_knn_unpack(const float* scores, const int32_t* docs, const uint32_t* counts, int32_t k_stride, int32_t n_queries,
                                       int32_t k_pass, const int32_t* ks, const float* boosts, nrtgpu_topdocs* out) {
  if (!scores || !docs || !counts || !out || n_queries <= 0 || k_pass <= 0 || k_stride < k_pass) return fail(NRTGPU_ERR_INVALID_ARG, "bad knn_unpack arguments");
  std::vector<uint64_t> keys((size_t)n_queries * (size_t)k_stride, 0ull);
  for (size_t i = 0; i < keys.size(); ++i)
    if ((uint32_t)(i % (size_t)k_stride) < counts[i / (size_t)k_stride]) keys[i] = pack_key(scores[i], (uint32_t)docs[i]);
  const KnnUniform one{k_pass, 0, 1.0f, 0.0f};
  std::vector<int32_t> k_of((size_t)n_queries, k_pass);
  std::vector<float> boost_of((size_t)n_queries, 1.0f);
  const KnnAsk each{ks ? ks : k_of.data(), boosts ? boosts : boost_of.data(), nullptr, nullptr, 1};
  knn_unpack_topdocs(keys.data(), counts, (uint32_t)k_stride, n_queries, false, 0, true, ks || boosts ? each : one.ask(), out);
  return NRTGPU_OK;
}

// Test hook (tests/test_knn_query_stats_host.py binds it itself: the Python bindings list the header's symbols and stay as they
// are): the query statistics of a float pass (vectors.cpp: knn_query_stats) of n_queries x dim floats -- |q|^2, the largest
// |element| and the 1-norm per query as the search computes them, eight queries side by side -- next to |q|^2 by the rescorers'
// chain (float_qnorm2), one query after the other: the two must agree bit for bit.  No context, no device work.
extern "C" int nrtgpu_debug_knn_query_stats(const float* queries, int32_t n_queries, int32_t dim, float* norm2, float* max_abs, double* l1,
                                            float* ref_norm2) {
  if (!queries || !norm2 || !max_abs || !l1 || !ref_norm2 || n_queries <= 0 || dim <= 0) return fail(NRTGPU_ERR_INVALID_ARG, "bad knn_query_stats arguments");
  knn_query_stats(queries, n_queries, dim, norm2, max_abs, l1);
  for (int32_t q = 0; q < n_queries; ++q) ref_norm2[q] = float_qnorm2(queries + (size_t)q * dim, dim);
  return NRTGPU_OK;
}

// The MaxScore route's meetings (include/nrtgpu_dev.h), from the instrumented kernels' per-item counters (search.cpp takes them
// out of the profile rows).
extern "C" int nrtgpu_debug_maxscore_meetings(nrtgpu_ctx* ctx, int64_t* out4) {
  if (!ctx || !out4) return fail(NRTGPU_ERR_INVALID_ARG, "NULL argument");
  std::lock_guard<std::mutex> lk(ctx->stats_mu);
  for (int i = 0; i < 4; ++i) out4[i] = ctx->ms_meetings[i];
  return NRTGPU_OK;
}

extern "C" int nrtgpu_debug_maxscore_meeting_guesses(nrtgpu_ctx* ctx, int64_t* out1) {
  if (!ctx || !out1) return fail(NRTGPU_ERR_INVALID_ARG, "NULL argument");
  std::lock_guard<std::mutex> lk(ctx->stats_mu);
  *out1 = ctx->ms_meetings[4];
  return NRTGPU_OK;
}

// Test hook (include/nrtgpu_dev.h): the one-wave selection of the MaxScore walk's estimator on keys of the caller's.
extern "C" int nrtgpu_debug_wave_kth(const uint64_t* keys, int32_t n, int32_t r, uint64_t* out) {
  if (!keys || !out || n < 1 || n > kMsCandCap || r < 1 || r > n) return fail(NRTGPU_ERR_INVALID_ARG, "bad wave_kth arguments (1 <= r <= n <= %d)", kMsCandCap);
  uint64_t* d = nullptr;
  if (hipMalloc((void**)&d, ((size_t)n + 1) * sizeof(uint64_t)) != hipSuccess) return fail(NRTGPU_ERR_OOM, "hipMalloc");
  hipError_t e = hipMemcpy(d, keys, (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    launch_debug_wave_kth(nullptr, d, (uint32_t)n, (uint32_t)r, d + n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out, d + n, sizeof(uint64_t), hipMemcpyDeviceToHost);   // (the null stream: behind the kernel)
  (void)hipFree(d);
  if (e != hipSuccess) return fail(NRTGPU_ERR_HIP, "wave_kth: %s", hipGetErrorString(e));
  return NRTGPU_OK;
}

// Test hook (include/nrtgpu_dev.h): the walk rows of a batch.  The plan is the searches' own (build_plan), the expansion the
// searches' own kernel; the buffers are this call's.
extern "C" int64_t nrtgpu_debug_walk_rows(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                          const nrtgpu_bm25_query* queries, int32_t n_queries, int32_t* out_begin, int32_t* out_n,
                                          uint64_t* out_rows, int64_t cap_rows) {
  if (!ctx || !segs || !queries || !out_begin || !out_n || (!out_rows && cap_rows > 0)) return -(int64_t)fail(NRTGPU_ERR_INVALID_ARG, "NULL argument");
  if (n_queries <= 0 || n_segs <= 0 || cap_rows < 0) return -(int64_t)fail(NRTGPU_ERR_INVALID_ARG, "n_queries and n_segs must be > 0");
  if (hipSetDevice(ctx->device) != hipSuccess) return -(int64_t)fail(NRTGPU_ERR_HIP, "hipSetDevice");
  for (int si = 0; si < n_segs; ++si)
    if (!segs[si]) return -(int64_t)fail(NRTGPU_ERR_INVALID_ARG, "segment %d is NULL", si);
  SegReadLocks content(segs, n_segs);
  HostPlan hp;
  if (int rc = build_plan(ctx, segs, doc_bases, n_segs, queries, n_queries, hp, 1)) return -(int64_t)rc;
  const size_t n_pairs = (size_t)n_queries * (size_t)n_segs;
  for (size_t i = 0; i < n_pairs; ++i) out_begin[i] = -1, out_n[i] = 0;
  if (hp.n_dterms == 0) return 0;
  Carver c;
  const size_t o_qx = c.take(sizeof(DExpandHead) + hp.qexpand.size() * sizeof(DQExpand)) + sizeof(DExpandHead), o_qt = c.take(hp.qterms.size() * sizeof(DQTerm));
  const size_t o_qsb = c.take(hp.qs_begin.size() * 4), o_caches = c.take(hp.caches.size() * sizeof(float));
  const size_t o_queries = c.take(hp.queries.size() * sizeof(DQuery)), o_up = c.off;
  const size_t o_terms = c.take((size_t)hp.n_dterms * sizeof(DTerm)), o_rows = c.take((size_t)hp.n_dterms * sizeof(DWalkRow));
  std::vector<char> hb(c.off, 0);
  memcpy(hb.data() + o_qx, hp.qexpand.data(), hp.qexpand.size() * sizeof(DQExpand));
  if (!hp.qterms.empty()) memcpy(hb.data() + o_qt, hp.qterms.data(), hp.qterms.size() * sizeof(DQTerm));
  memcpy(hb.data() + o_qsb, hp.qs_begin.data(), hp.qs_begin.size() * 4);
  if (!hp.caches.empty()) memcpy(hb.data() + o_caches, hp.caches.data(), hp.caches.size() * sizeof(float));
  memcpy(hb.data() + o_queries, hp.queries.data(), hp.queries.size() * sizeof(DQuery));
  char* db = nullptr;
  if (hipMalloc((void**)&db, c.off) != hipSuccess) return -(int64_t)fail(NRTGPU_ERR_OOM, "hipMalloc");
  DExpandHead xh{};
  xh.caches = (const float*)(db + o_caches);
  xh.queries = (const DQuery*)(db + o_queries);
  xh.rows = (DWalkRow*)(db + o_rows);
  memcpy(hb.data() + o_qx - sizeof(DExpandHead), &xh, sizeof(xh));
  hipError_t e = hipMemcpy(db, hb.data(), o_up, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(db + o_up, 0, c.off - o_up);
  if (e == hipSuccess) {
    launch_expand_terms(nullptr, (const DQExpand*)(db + o_qx), (const DQTerm*)(db + o_qt), (const uint32_t*)(db + o_qsb), (uint32_t)n_queries,
                        hp.n_leaves, (DTerm*)(db + o_terms));
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(hb.data() + o_rows, db + o_rows, (size_t)hp.n_dterms * sizeof(DWalkRow), hipMemcpyDeviceToHost);   // (the null stream: behind the kernel)
  (void)hipFree(db);
  if (e != hipSuccess) return -(int64_t)fail(NRTGPU_ERR_HIP, "walk_rows: %s", hipGetErrorString(e));
  static_assert(sizeof(DWalkRow) == 80, "ten words per row");
  if (out_rows) memcpy(out_rows, hb.data() + o_rows, (size_t)std::min<int64_t>(cap_rows, (int64_t)hp.n_dterms) * sizeof(DWalkRow));
  // the rows of (query, leaf): where the plan put them; how many: up to the next pair's (pairs are numbered in plan order)
  std::vector<uint32_t> begins;
  for (size_t i = 0; i < n_pairs; ++i)
    if (hp.qs_begin[i] != 0xFFFFFFFFu) begins.push_back(hp.qs_begin[i]);
  std::sort(begins.begin(), begins.end());
  for (size_t i = 0; i < n_pairs; ++i) {
    const uint32_t b = hp.qs_begin[i];
    if (b == 0xFFFFFFFFu || hp.qexpand[i / (size_t)n_segs].by_weight == 0u) continue;
    auto nx = std::upper_bound(begins.begin(), begins.end(), b);
    out_begin[i] = (int32_t)b;
    out_n[i] = (int32_t)((nx == begins.end() ? hp.n_dterms : *nx) - b);
  }
  return (int64_t)hp.n_dterms;
}

// Test hook (include/nrtgpu_dev.h): one posting's fixed-point value, by the device's own statement of it.
extern "C" int nrtgpu_debug_walk_value(float weight, const uint32_t* freq, const uint32_t* norm, int32_t n, const float* table256, int32_t fx_scale,
                                       uint32_t fx_shift, uint64_t* out) {
  if (!freq || !norm || !table256 || !out || n < 1 || fx_shift > 31u) return fail(NRTGPU_ERR_INVALID_ARG, "bad walk_value arguments");
  char* d = nullptr;
  const size_t o_f = 0, o_n = (size_t)n * 4, o_t = 2 * (size_t)n * 4, o_o = o_t + 1024, bytes = o_o + (size_t)n * 8;
  if (hipMalloc((void**)&d, bytes) != hipSuccess) return fail(NRTGPU_ERR_OOM, "hipMalloc");
  hipError_t e = hipMemcpy(d + o_f, freq, (size_t)n * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d + o_n, norm, (size_t)n * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d + o_t, table256, 1024, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    launch_debug_walk_value(nullptr, weight, (const uint32_t*)(d + o_f), (const uint32_t*)(d + o_n), (const float*)(d + o_t), fx_scale, fx_shift, (uint32_t)n,
                            (uint64_t*)(d + o_o));
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out, d + o_o, (size_t)n * 8, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) return fail(NRTGPU_ERR_HIP, "walk_value: %s", hipGetErrorString(e));
  return NRTGPU_OK;
}
