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

// The MaxScore route's meetings (include/nrtgpu_dev.h), from the instrumented kernels' per-item counters (search.cpp takes them
// out of the profile rows).
extern "C" int nrtgpu_debug_maxscore_meetings(nrtgpu_ctx* ctx, int64_t* out4) {
  if (!ctx || !out4) return fail(NRTGPU_ERR_INVALID_ARG, "NULL argument");
  std::lock_guard<std::mutex> lk(ctx->stats_mu);
  for (int i = 0; i < 4; ++i) out4[i] = ctx->ms_meetings[i];
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
