// knn_bytes.hip -- exact (brute-force) search over byte (int8) vector fields on the i8 matrix cores of gfx950.
//
// Replaces ExactVectorQuery.ExactByteVectorQuery (query/vector/ExactVectorQuery.java:230-247) and the exact reading of
// NrtKnnByteVectorQuery (field/VectorFieldDef.java:789-829): score = similarityToScore(compare(query, doc vector)) * boost
// (VectorFieldDef.java:870-881) for every doc that has a vector, and the top-k collector behind it.
//
// Every quantity the byte scorers compute is an INTEGER -- dot product, squared norms, squared distance; below 2^28 at 2048
// dimensions -- and v_mfma_i32_16x16x64_i8 returns integers exactly, in whatever order it sums.  So ONE pass over the rows gives
// final score bits (plan.h: knn_byte_score, the function nrtgpu_byte_vector_score exposes): nothing is nominated, rescored or
// certified here, unlike the fp32 search (knn.hip).  What is kept of that search is its skeleton -- one workgroup per CU, the query
// panel in LDS in operand order, a wave streaming a contiguous run of 16-row tiles over ALL leaves of the call with a ring of
// 16-byte requests in flight, a workgroup-local queue of the rows that beat theta -- and its selection contract (candidate lists
// of `cap` keys, theta, overflow; knn_select_kernel<false>), with keys that are results.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "plan.h"
#include "topk.hiph"

namespace nrtgpu {

typedef int i32x4 __attribute__((ext_vector_type(4)));   // 16 int8 of an operand, or 4 int32 of a result

constexpr int kKnnBytesThreads = 1024;   // 16 waves, one workgroup per CU (the panel takes up to 128 KiB of LDS)
constexpr size_t kKnnBytesStaticLds = 1280;   // knn_bytes_kernel's per-query tables
constexpr size_t kKnnBytesReqStaticLds = 1536;   // knn_bytes_requests_kernel's: the same + a threshold per query

// Resident format, written at upload from a staged chunk of the caller's rows (row-major, `dim` bytes each, rows
// [row0, row0 + n_chunk) of the field; row0 is a multiple of 16): one thread per 16-byte piece of the chunk's tiles.  Elements
// beyond `dim` and rows beyond n_chunk are zero: they add nothing to a dot product or a squared norm.  The piece's share of its
// row's |v|^2 is added to norm2[row] (integer atomics: exact in any order; zeroed by the caller).
__global__ __launch_bounds__(256) void knn_bytes_pack_kernel(const int8_t* __restrict__ rows, int32_t dim, int64_t row0, int64_t n_chunk,
                                                            int32_t steps, i32x4* __restrict__ tiles, int32_t* __restrict__ norm2) {
  const int64_t piece = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t chunk_tiles = (n_chunk + 15) >> 4;
  if (piece >= chunk_tiles * steps * 64) return;
  const int32_t l = (int32_t)(piece & 63);
  const int64_t ts = piece >> 6;
  const int32_t s = (int32_t)(ts % steps);
  const int64_t row = (ts / steps) * 16 + (l & 15);   // in the chunk
  const int32_t k0 = 64 * s + 16 * (l >> 4);
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  int32_t n2 = 0;
  if (row < n_chunk) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int32_t k = k0 + e;
      const int32_t x = k < dim ? (int32_t)rows[row * dim + k] : 0;
      n2 += x * x;
      w[e >> 2] |= ((uint32_t)x & 0xFFu) << (8 * (e & 3));
    }
  }
  tiles[(row0 >> 4) * steps * 64 + piece] = i32x4{(int)w[0], (int)w[1], (int)w[2], (int)w[3]};
  if (n2) atomicAdd(&norm2[row0 + row], n2);
}

// The ring of row pieces is driven by hand, as knn_sketch_kernel's (knn.hip): the requests are inline asm loads, and before slot
// i is consumed the wave waits until at most D - 1 requests are outstanding -- exactly the ones issued after slot i's.
template <int OFF>
__device__ __forceinline__ void kb_request(i32x4& dst, const i32x4* p) {
  asm volatile("global_load_dwordx4 %0, %1, off offset:%2" : "=v"(dst) : "v"(p), "n"(OFF) : "memory");
}
template <int N>
__device__ __forceinline__ void kb_wait(i32x4& slot) {
  asm volatile("s_waitcnt vmcnt(%1)" : "+v"(slot) : "n"(N) : "memory");
}
template <int D, int I>
__device__ __forceinline__ void kb_fill(i32x4 (&abuf)[D], const i32x4* cur) {
  if constexpr (I < D) {
    kb_request<(I & 3) * 1024>(abuf[I], I < 4 ? cur : cur + 256);
    kb_fill<D, I + 1>(abuf, cur);
  }
}
// steps I .. D - 1 of a group of D: the step's P query operands are asked of the LDS together and before the wait for the row
// piece; the piece D ahead is requested into the registers the matrix instructions have just read
template <int P, int D, int I>
__device__ __forceinline__ void kb_steps(i32x4 (&abuf)[D], i32x4 (&acc)[P], const i32x4* qs_group, const i32x4* nxt) {
  if constexpr (I < D) {
    i32x4 b[P];
#pragma unroll
    for (int p = 0; p < P; ++p) b[p] = qs_group[(I * P + p) * 64];
    __builtin_amdgcn_sched_barrier(0);
    kb_wait<D - 1>(abuf[I]);
#pragma unroll
    for (int p = 0; p < P; ++p) acc[p] = __builtin_amdgcn_mfma_i32_16x16x64_i8(abuf[I], b[p], acc[p], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    kb_request<(I & 3) * 1024>(abuf[I], I < 4 ? nxt : nxt + 256);
    __builtin_amdgcn_sched_barrier(0);
    kb_steps<P, D, I + 1>(abuf, acc, qs_group, nxt);
  }
}

__device__ __forceinline__ uint64_t kb_uniform_u64(uint64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
  return ((uint64_t)hi << 32) | (uint64_t)lo;
}
__device__ __forceinline__ int32_t kb_leaf_of_tile(const DKnnBytesLeaf* __restrict__ leaves, int32_t n_leaves, int64_t tile) {
  int32_t lo = 0, hi = n_leaves;   // the last leaf whose tile_begin <= tile
  while (hi - lo > 1) {
    const int32_t mid = (lo + hi) >> 1;
    if (leaves[mid].tile_begin <= tile) lo = mid; else hi = mid;
  }
  return lo;
}

// Which rows can beat theta, decided on the INTEGERS (one compare per element; the score proper is computed for the few that pass).
// The score is a monotone function of the dot product (dot_product, max_inner_product: non-decreasing) or of the squared distance
// (l2_norm: non-increasing) -- every step of knn_byte_score is one correctly rounded, hence monotone, operation, and so is the
// multiplication by a boost > 0 -- so "score * boost >= theta's score" is "dot >= D" / "d2 <= D" for an integer D found by
// bisection over the very function the epilogue calls: the test is exact, not a bound.  Cosine divides by the row's own norm:
// there the test is a necessary condition on (float)dot * rsq(|v|^2), lowered by 2^-16 of the scale the estimate's few fp32
// roundings (2^-21) live on.  One 32-bit word per query:
//   sim 1, 3: a row may pass iff dot >= thr          (everything: INT32_MIN, nothing: INT32_MAX)
//   sim 2   : iff |v|^2 - 2 dot <= thr               (thr = D - |q|^2; everything: INT32_MAX, nothing: INT32_MIN)
//   sim 0   : iff !((float)dot * rsq|v|^2 <= thr as float)   (everything: -inf, nothing: +inf; a NaN product -- a zero row -- passes)
constexpr int32_t kKnnBytesMaxDot = 1 << 26;   // > 2048 * 128 * 128
__device__ inline int32_t knn_bytes_threshold(int sim, int32_t dim, int32_t nq, unsigned long long th, float boost, bool has_query) {
  const bool upward = sim != 2;
  const int32_t all = sim == 0 ? (int32_t)__float_as_uint(-INFINITY) : (upward ? INT32_MIN : INT32_MAX);
  const int32_t none = sim == 0 ? (int32_t)__float_as_uint(INFINITY) : (upward ? INT32_MAX : INT32_MIN);
  if (!has_query || th == ~0ull) return none;
  const float ts = key_score(th);
  if (th == 0ull || !(boost > 0.0f) || !(boost < INFINITY) || !(ts > 0.0f)) return all;
  if (sim == 0) {
    const float x = 2.0f * (ts / boost) - 1.0f;   // the cosine must reach about this
    if (!(x > -INFINITY && x < INFINITY)) return all;
    const float t = (x - (fabsf(x) + 1.0f) * 0x1p-16f) * sqrtf((float)nq);
    return t == t ? (int32_t)__float_as_uint(t) : all;
  }
  if (upward) {   // the smallest dot whose score reaches ts
    int32_t lo = -kKnnBytesMaxDot, hi = kKnnBytesMaxDot;
    if (!(knn_byte_score(sim, dim, hi, 0, 0) * boost >= ts)) return none;
    while (lo < hi) {
      const int32_t mid = lo + ((hi - lo) >> 1);
      if (knn_byte_score(sim, dim, mid, 0, 0) * boost >= ts) hi = mid; else lo = mid + 1;
    }
    return lo;
  }
  int32_t lo = 0, hi = 1 << 28;   // the largest squared distance whose score reaches ts (knn_byte_score(2, ., 0, d2, 0): d2 = nq + 0 - 0)
  if (!(knn_byte_score(2, dim, 0, lo, 0) * boost >= ts)) return none;
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo + 1) >> 1);
    if (knn_byte_score(2, dim, 0, mid, 0) * boost >= ts) lo = mid; else hi = mid - 1;
  }
  return lo - nq;
}

// Scores the global tiles [tile_begin, tile_end) of the call's leaves against <= 16 P queries; rows whose key beats theta[q] are
// appended to query q's candidate list (knn.hip: knn_score_kernel's contract: `cap` keys per list, cand_cnt may exceed cap =>
// overflow, the host redoes; a query without a theta gives every padded row of the launch its own slot of the list unless
// append_only).  `steps` = resident dimension / 64, a multiple of D (the ring's depth; launch_knn_bytes picks it).
//   panel  : [steps][P][64] 16-byte operands: step s, panel p, lane l -> q[(l & 15) + 16p][64s + 16(l >> 4) .. +15] (the host stages it)
//   qnorm2 : |q|^2 per query; dim_user: the field's own dimension (dot_product's divisor)
//   min_score > 0: rows whose UNBOOSTED score is below it are no hits (the knn request path, which passes boost = 1)
// C/D layout of the instruction: query col = lane & 15 (+ 16p), row in tile = 4 (lane >> 4) + reg.
//
// knn_bytes_kernel and knn_bytes_requests_kernel are ONE body, knn_bytes_body.hiph, compiled twice (it says why it is a text and
// not a __device__ template).  The second is the pass of nrtgpu_knn_search_bytes_requests, whose queries are knn requests with a
// filter and a threshold EACH: min_scores[q] (n_q floats) in place of the launch's one min_score, and the leaves bring their rows
// of the pass's accept table (DKnnBytesLeaf::accept_of, plan.h) in place of their one accept set.
#define KB_KERNEL knn_bytes_kernel
#define KB_REQUESTS 0
#include "knn_bytes_body.hiph"
#undef KB_KERNEL
#undef KB_REQUESTS
#define KB_KERNEL knn_bytes_requests_kernel
#define KB_REQUESTS 1
#include "knn_bytes_body.hiph"
#undef KB_KERNEL
#undef KB_REQUESTS

// ---- the RESCORER over a byte field (QueryRescore with an ExactByteVectorQuery in the rescore slot) -------------------------
// A first-pass hit names ONE row, and the rows have one copy: the tiles above.  Row r is not contiguous there -- it is the 16-byte
// PIECES (s, kk), s < steps, kk < 4 (dimensions 64s + 16kk .. +15), at
//   tiles[((r >> 4) * steps + s) * 64 + kk * 16 + (r & 15)]
// that is piece p = 4s + kk (dimensions 16p .. 16p + 15) at 16 p operands = 256 p bytes behind the row's BASE
// tiles + (r >> 4) * steps * 64 + (r & 15): a walk at a fixed stride.  The query is kept in the same piece order, which is the
// query itself, zero-padded to whole pieces.
constexpr int kByteRescoreRows = 8;   // hits a wave scores side by side: one or two 16-byte loads per row and lane, all in flight together
// The dot products of R rows (bases as above, wave-uniform; nullptr: no row) with the query in LDS.  Lane l takes pieces l and
// l + 64 of every row (dimension 768: 48 lanes, one load per row; 2048: two); only pieces that hold dimensions of the field are
// read (n_pieces = ceil(dim / 16) <= 128).  Products through the packed int8 dot instruction, then an integer butterfly: the
// integers are exact in any order, so every caller gets the same numbers -- the ONE routine of both rescore kernels.
template <int R>
__device__ __forceinline__ void kb_rows_dot(const i32x4* const (&rows)[R], const i32x4* q_lds, int32_t n_pieces, uint32_t lane,
                                            int32_t (&dot)[R]) {
  // (the bases come out of LDS or are computed from a kernel argument: say that they are global memory)
  typedef const __attribute__((address_space(1))) i32x4* gpiece_ptr;
  const bool p0 = (int32_t)lane < n_pieces, p1 = (int32_t)lane + 64 < n_pieces;
  const i32x4 zero = i32x4{0, 0, 0, 0};
  i32x4 x0[R], x1[R];
#pragma unroll
  for (int r = 0; r < R; ++r) x0[r] = (rows[r] && p0) ? ((gpiece_ptr)rows[r])[16u * lane] : zero;   // (rows[r]: wave-uniform)
#pragma unroll
  for (int r = 0; r < R; ++r) x1[r] = zero;
  if (n_pieces > 64) {
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (rows[r] && p1) x1[r] = ((gpiece_ptr)rows[r])[16u * (lane + 64u)];
  }
  const i32x4 q0 = p0 ? q_lds[lane] : zero, q1 = p1 ? q_lds[lane + 64u] : zero;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    int32_t a = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) a = __builtin_amdgcn_sdot4(x0[r][w], q0[w], a, false);
#pragma unroll
    for (int w = 0; w < 4; ++w) a = __builtin_amdgcn_sdot4(x1[r][w], q1[w], a, false);
    dot[r] = a;
  }
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) dot[r] += __shfl_xor(dot[r], d, 64);
}
__device__ __forceinline__ const i32x4* kb_uniform_row(const i32x4* p) {   // a pointer every lane holds, as scalars
  return (const i32x4*)(uintptr_t)kb_uniform_u64((uint64_t)(uintptr_t)p);
}
// QueryRescore.combine over the byte scorer: second = knn_byte_score(...) * boost -- what knn_bytes_kernel returns for the
// (query, row, boost) -- and (float)(qw * first + rw * second) in double; a hit without a row keeps (float)(qw * first).
__device__ __forceinline__ float kb_combined(bool has_row, int sim, int32_t dim, int32_t dot, int32_t nq, int32_t nv, float boost,
                                             float first, double qw, double rw) {
  if (!has_row) return (float)(qw * (double)first);
  const float second = knn_byte_score(sim, dim, dot, nq, nv) * boost;
  return (float)(qw * (double)first + rw * (double)second);
}

// One wave per kByteRescoreRows hits of one leaf; vec_row[i] = the hit's row in the leaf's field (< 0: no vector), given by the
// host as for rescore_vectors_kernel (knn.hip).  query: the query in piece order, 64 `steps` bytes.
__global__ __launch_bounds__(256)
void rescore_byte_vectors_kernel(const i32x4* __restrict__ tiles, const int32_t* __restrict__ vnorm2, int32_t steps, int32_t dim,
                                 const i32x4* __restrict__ query, int32_t qnorm2, int32_t sim, float boost,
                                 const int64_t* __restrict__ vec_row, const float* __restrict__ first_scores, int32_t n, double qw,
                                 double rw, float* __restrict__ out_scores) {
  __shared__ i32x4 qs[128];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const int32_t n_pieces = (dim + 15) >> 4;
  if ((int32_t)tid < n_pieces) qs[tid] = query[tid];
  __syncthreads();
  const int32_t i0 = (int32_t)(blockIdx.x * 4u + wave) * kByteRescoreRows;
  if (i0 >= n) return;
  const i32x4* rows[kByteRescoreRows];
#pragma unroll
  for (int r = 0; r < kByteRescoreRows; ++r) {
    const int64_t row = i0 + r < n ? vec_row[i0 + r] : -1;
    rows[r] = kb_uniform_row(row >= 0 ? tiles + (row >> 4) * steps * 64 + (row & 15) : nullptr);
  }
  int32_t dot[kByteRescoreRows];
  kb_rows_dot<kByteRescoreRows>(rows, qs, n_pieces, lane, dot);
  // lane r finishes hit r (every lane holds every sum)
  int32_t my_dot = 0;
#pragma unroll
  for (int r = 0; r < kByteRescoreRows; ++r)
    if (lane == (uint32_t)r) my_dot = dot[r];
  const int32_t i = i0 + (int32_t)lane;
  if (lane < (uint32_t)kByteRescoreRows && i < n) {
    const int64_t row = vec_row[i];
    out_scores[i] = kb_combined(row >= 0, sim, dim, my_dot, qnorm2, row >= 0 ? vnorm2[row] : 0, boost, first_scores[i], qw, rw);
  }
}

// The hybrid tail over a byte field: hybrid_rescore_kernel's two phases (knn.hip) -- one workgroup per query over its sorted
// first-pass hits in HBM --
//   1. a THREAD per hit: key -> (leaf, row) -> the row's base in the tiles and its norm into LDS -- every hit's chain at once;
//   2. a wave per kByteRescoreRows hits: kb_rows_dot, then a lane per hit for the score and QueryRescore.combine,
// then QueryRescorer's sort (combined score desc, doc asc) in LDS and the window.  qvecs: the queries in piece order, 64 `steps`
// bytes each.
constexpr int kHybridBytesThreads = 1024;
__global__ __launch_bounds__(kHybridBytesThreads)
void hybrid_rescore_bytes_kernel(const uint64_t* __restrict__ first_keys, const uint32_t* __restrict__ first_counts, uint32_t k_stride,
                                 const DByteVecSeg* __restrict__ segs, int32_t n_segs, int32_t steps, int32_t dim,
                                 const i32x4* __restrict__ qvecs, const int32_t* __restrict__ qnorm2, int32_t sim, float boost, double qw,
                                 double rw, uint32_t window, uint64_t* __restrict__ out_keys, uint32_t* __restrict__ out_counts,
                                 uint32_t w_stride) {
  __shared__ uint64_t cand[1024];        // phase 1: the first-pass keys; phase 2: the combined keys
  __shared__ const i32x4* h_row[1024];   // the hit's row base (nullptr: the doc has no vector)
  __shared__ int32_t h_nv[1024];
  __shared__ i32x4 qs[128];
  const uint32_t q = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t n = min(first_counts[q], 1024u);
  const int32_t n_pieces = (dim + 15) >> 4;
  const int32_t nq = qnorm2[q];
  if ((int32_t)tid < n_pieces) qs[tid] = qvecs[(size_t)q * (size_t)steps * 4 + tid];
  for (uint32_t i = tid; i < n; i += (uint32_t)kHybridBytesThreads) {
    const uint64_t key = first_keys[(size_t)q * k_stride + i];
    const uint32_t gdoc = 0xFFFFFFFFu - (uint32_t)key;
    const i32x4* base = nullptr;
    int32_t nv = 0;
    for (int32_t si = 0; si < n_segs; ++si) {
      const DByteVecSeg sg = segs[si];
      const int64_t local = (int64_t)gdoc - (int64_t)sg.doc_base;
      if (local < 0 || local >= (int64_t)sg.max_doc) continue;
      if (sg.tiles) {
        int64_t row = -1;
        if (!sg.ord_to_doc) {
          if (local < (int64_t)sg.n_vec) row = local;
        } else {  // lower_bound over the leaf's ascending ord -> doc map
          int32_t lo = 0, hi = sg.n_vec;
          while (lo < hi) {
            const int32_t mid = lo + ((hi - lo) >> 1);
            if (sg.ord_to_doc[mid] < (int32_t)local) lo = mid + 1; else hi = mid;
          }
          if (lo < sg.n_vec && sg.ord_to_doc[lo] == (int32_t)local) row = lo;
        }
        if (row >= 0) {
          base = (const i32x4*)sg.tiles + (row >> 4) * steps * 64 + (row & 15);
          nv = sg.vnorm2[row];
        }
      }
      break;
    }
    cand[i] = key;
    h_row[i] = base;
    h_nv[i] = nv;
  }
  __syncthreads();
  constexpr uint32_t kWaves = (uint32_t)(kHybridBytesThreads / 64);
  for (uint32_t i0 = wave; i0 < n; i0 += kWaves * (uint32_t)kByteRescoreRows) {
    const i32x4* rows[kByteRescoreRows];
#pragma unroll
    for (int r = 0; r < kByteRescoreRows; ++r) {
      const uint32_t idx = i0 + (uint32_t)r * kWaves;
      rows[r] = kb_uniform_row(idx < n ? h_row[idx] : nullptr);   // (uniform LDS reads)
    }
    int32_t dot[kByteRescoreRows];
    kb_rows_dot<kByteRescoreRows>(rows, qs, n_pieces, lane, dot);
    int32_t my_dot = 0;
#pragma unroll
    for (int r = 0; r < kByteRescoreRows; ++r)
      if (lane == (uint32_t)r) my_dot = dot[r];
    const uint32_t idx = i0 + lane * kWaves;   // lane r finishes hit r
    if (lane < (uint32_t)kByteRescoreRows && idx < n) {
      const uint64_t key = cand[idx];
      const float comb = kb_combined(h_row[idx] != nullptr, sim, dim, my_dot, nq, h_nv[idx], boost, key_score(key), qw, rw);
      cand[idx] = pack_key(comb, 0xFFFFFFFFu - (uint32_t)key);
    }
  }
  uint32_t n2 = 1;
  while (n2 < n) n2 <<= 1;
  for (uint32_t i = n + tid; i < n2; i += (uint32_t)kHybridBytesThreads) cand[i] = 0;
  bitonic_sort_desc<kHybridBytesThreads>(cand, n2);  // starts with a barrier
  const uint32_t m = min(n, window);
  for (uint32_t i = tid; i < w_stride; i += (uint32_t)kHybridBytesThreads) out_keys[(size_t)q * w_stride + i] = i < m ? cand[i] : 0;
  if (tid == 0) out_counts[q] = m;
}

// ---- launchers ------------------------------------------------------------------------------------
// Steps (64 dimensions each) a row is resident with, and the ring's depth: the depth must divide the steps (the ring is indexed
// statically and the epilogue stands once per tile).  Up to 8 steps the ring holds a whole tile; beyond, the steps are padded
// (with zeros) to the next count that has a divisor in 4 .. 8: 9 -> 10 (dimensions 513-576: 11 % more bytes stored and streamed, the worst case),
// 11 -> 12, 13 -> 14, 17 -> 18, 19 -> 20, 22 / 23 -> 24, 26 / 27 -> 28, 29 -> 30, 31 -> 32.
static int32_t knn_bytes_depth_of(int32_t steps) {
  if (steps <= 8) return steps;
  for (int32_t d = 8; d >= 4; --d)
    if (steps % d == 0) return d;
  return 0;
}
int32_t knn_bytes_steps(int32_t dim) {
  int32_t steps = std::max((dim + 63) >> 6, 1);
  while (knn_bytes_depth_of(steps) == 0) ++steps;
  return steps;
}
size_t knn_bytes_tile_bytes(int32_t dim, int64_t n) { return (size_t)((n + 15) >> 4) * (size_t)knn_bytes_steps(dim) * 1024; }
size_t knn_bytes_panel_bytes(int32_t dim, int32_t n_q) { return (size_t)knn_bytes_steps(dim) * (size_t)(n_q > 16 ? 4 : 1) * 1024; }

void launch_knn_bytes_pack(hipStream_t st, const int8_t* rows, int32_t dim, int64_t row0, int64_t n_chunk, void* tiles, int32_t* norm2) {
  if (n_chunk <= 0) return;
  const int32_t steps = knn_bytes_steps(dim);
  const int64_t pieces = ((n_chunk + 15) >> 4) * steps * 64;
  hipLaunchKernelGGL(knn_bytes_pack_kernel, dim3((uint32_t)((pieces + 255) / 256)), dim3(256), 0, st, rows, dim, row0, n_chunk, steps,
                     (i32x4*)tiles, norm2);
}

// min_scores == nullptr: knn_bytes_kernel with the launch's one min_score.  Else a pass of knn requests (knn_bytes_requests_kernel):
// min_scores = n_q thresholds on the device, every leaf brings its row of the accept table (accept_of), min_score is not read.
int launch_knn_bytes(hipStream_t st, uint32_t blocks, const DKnnBytesLeaf* leaves, int32_t n_leaves, int32_t dim, int64_t tile_begin,
                     int64_t tile_end, const void* panel, const int32_t* qnorm2, int32_t n_q, int32_t sim, float boost, float min_score,
                     const unsigned long long* theta, uint64_t* cand, uint32_t* cand_cnt, uint32_t cap, int32_t append_only,
                     const float* min_scores) {
  if (tile_end <= tile_begin || n_leaves <= 0) return 0;
  if (n_q < 1 || n_q > 64 || dim < 1 || dim > 2048) return (int)hipErrorInvalidValue;
  const int32_t steps = knn_bytes_steps(dim), depth = knn_bytes_depth_of(steps);
  const size_t panel_bytes = knn_bytes_panel_bytes(dim, n_q);
  // the queue behind the panel: what 160 KiB leave next to the panel and the kernel's static tables, 4096 entries at most
  const size_t static_lds = min_scores ? kKnnBytesReqStaticLds : kKnnBytesStaticLds;
  const uint32_t qcap = (uint32_t)std::min<size_t>(4096, (160 * 1024 - static_lds - panel_bytes - 16) / 8);
  const size_t lds = panel_bytes + 16 + (size_t)qcap * 8;
#define NRT_BYTES_LAUNCH(KERNEL, THRESHOLD, PANELS, DEPTH)                                                                         \
  {                                                                                                                                \
    hipError_t e = hipFuncSetAttribute((const void*)KERNEL<PANELS, DEPTH>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);  \
    if (e != hipSuccess) return (int)e;                                                                                            \
    hipLaunchKernelGGL((KERNEL<PANELS, DEPTH>), dim3(blocks), dim3(kKnnBytesThreads), lds, st, leaves, n_leaves, steps, dim,       \
                       tile_begin, tile_end, (const i32x4*)panel, qnorm2, n_q, sim, boost, THRESHOLD, theta, cand, cand_cnt, cap,  \
                       append_only, qcap);                                                                                         \
  }
#define NRT_BYTES_DEPTH(KERNEL, THRESHOLD, PANELS)                          \
  switch (depth) {                                                          \
    case 1: NRT_BYTES_LAUNCH(KERNEL, THRESHOLD, PANELS, 1) break;           \
    case 2: NRT_BYTES_LAUNCH(KERNEL, THRESHOLD, PANELS, 2) break;           \
    case 3: NRT_BYTES_LAUNCH(KERNEL, THRESHOLD, PANELS, 3) break;           \
    case 4: NRT_BYTES_LAUNCH(KERNEL, THRESHOLD, PANELS, 4) break;           \
    case 5: NRT_BYTES_LAUNCH(KERNEL, THRESHOLD, PANELS, 5) break;           \
    case 6: NRT_BYTES_LAUNCH(KERNEL, THRESHOLD, PANELS, 6) break;           \
    case 7: NRT_BYTES_LAUNCH(KERNEL, THRESHOLD, PANELS, 7) break;           \
    default: NRT_BYTES_LAUNCH(KERNEL, THRESHOLD, PANELS, 8) break;          \
  }
  if (min_scores) {
    if (n_q <= 16) { NRT_BYTES_DEPTH(knn_bytes_requests_kernel, min_scores, 1) }
    else { NRT_BYTES_DEPTH(knn_bytes_requests_kernel, min_scores, 4) }
  } else {
    if (n_q <= 16) { NRT_BYTES_DEPTH(knn_bytes_kernel, min_score, 1) }
    else { NRT_BYTES_DEPTH(knn_bytes_kernel, min_score, 4) }
  }
#undef NRT_BYTES_DEPTH
#undef NRT_BYTES_LAUNCH
  return 0;
}

void launch_rescore_byte_vectors(hipStream_t st, const void* tiles, const int32_t* vnorm2, int32_t dim, const void* query, int32_t qnorm2,
                                 int32_t sim, float boost, const int64_t* vec_row, const float* first_scores, int32_t n, double qw, double rw,
                                 float* out_scores) {
  if (n <= 0) return;
  const uint32_t per_block = 4u * (uint32_t)kByteRescoreRows;
  hipLaunchKernelGGL(rescore_byte_vectors_kernel, dim3(((uint32_t)n + per_block - 1) / per_block), dim3(256), 0, st, (const i32x4*)tiles, vnorm2,
                     knn_bytes_steps(dim), dim, (const i32x4*)query, qnorm2, sim, boost, vec_row, first_scores, n, qw, rw, out_scores);
}
void launch_hybrid_rescore_bytes(hipStream_t st, uint32_t n_queries, const uint64_t* first_keys, const uint32_t* first_counts,
                                 uint32_t k_stride, const DByteVecSeg* segs, int32_t n_segs, int32_t dim, const void* qvecs,
                                 const int32_t* qnorm2, int32_t sim, float boost, double qw, double rw, uint32_t window, uint64_t* out_keys,
                                 uint32_t* out_counts, uint32_t w_stride) {
  if (n_queries == 0) return;
  hipLaunchKernelGGL(hybrid_rescore_bytes_kernel, dim3(n_queries), dim3(kHybridBytesThreads), 0, st, first_keys, first_counts, k_stride, segs,
                     n_segs, knn_bytes_steps(dim), dim, (const i32x4*)qvecs, qnorm2, sim, boost, qw, rw, window, out_keys, out_counts, w_stride);
}

// ---- the GATHER route of nrtgpu_knn_search_bytes (knn.hip: knn_accept_rows_kernel lists the rows the filter accepts) -------------
// blockIdx.y = the panel's query (piece order, in LDS); a wave per kByteRescoreRows entries of the list: the rows' integers by the
// rescorers' routine (kb_rows_dot over the resident tiles), then a lane per row for knn_byte_score -- the bits knn_bytes_kernel
// returns for the pair -- and the key into slot i of the query's candidate list (the row's place in the list: nothing is counted,
// cand_cnt[q] = the list's length).  A row below min_score leaves key 0, which the selection drops.
__global__ __launch_bounds__(256)
void knn_gather_bytes_kernel(const DKnnGatherLeaf* __restrict__ leaves, const uint64_t* __restrict__ list, const uint32_t* __restrict__ count,
                             int32_t steps, int32_t dim, const i32x4* __restrict__ queries, const int32_t* __restrict__ qnorm2, int32_t sim,
                             float boost, float min_score, uint64_t* __restrict__ cand, uint32_t* __restrict__ cand_cnt, uint32_t cap) {
  __shared__ i32x4 qs[128];
  const uint32_t q = blockIdx.y, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  constexpr uint32_t kPerBlock = 4u * (uint32_t)kByteRescoreRows;
  const uint32_t n = min(*count, cap);
  if (blockIdx.x == 0 && tid == 0) cand_cnt[q] = n;
  if (blockIdx.x * kPerBlock >= n) return;
  const int32_t n_pieces = (dim + 15) >> 4;
  if ((int32_t)tid < n_pieces) qs[tid] = queries[(size_t)q * (size_t)steps * 4 + tid];
  __syncthreads();
  const int32_t nq = qnorm2[q];
  for (uint32_t i0 = (blockIdx.x * 4u + wave) * (uint32_t)kByteRescoreRows; i0 < n; i0 += gridDim.x * kPerBlock) {
    const i32x4* rows[kByteRescoreRows];
#pragma unroll
    for (int r = 0; r < kByteRescoreRows; ++r) {
      const i32x4* base = nullptr;
      if (i0 + (uint32_t)r < n) {
        const uint64_t e = list[i0 + (uint32_t)r];
        const int64_t row = (int64_t)(uint32_t)e;
        base = (const i32x4*)leaves[(uint32_t)(e >> 32)].rows + (row >> 4) * steps * 64 + (row & 15);
      }
      rows[r] = kb_uniform_row(base);
    }
    int32_t dot[kByteRescoreRows];
    kb_rows_dot<kByteRescoreRows>(rows, qs, n_pieces, lane, dot);
    int32_t my_dot = 0;   // lane r finishes row r (every lane holds every sum)
#pragma unroll
    for (int r = 0; r < kByteRescoreRows; ++r)
      if (lane == (uint32_t)r) my_dot = dot[r];
    const uint32_t i = i0 + lane;
    if (lane < (uint32_t)kByteRescoreRows && i < n) {
      const uint64_t e = list[i];
      const DKnnGatherLeaf* lf = leaves + (uint32_t)(e >> 32);
      const uint32_t ord = (uint32_t)e;
      const int32_t* ord_to_doc = lf->ord_to_doc;
      const int32_t doc = ord_to_doc ? ord_to_doc[ord] : (int32_t)ord;
      const float s = knn_byte_score(sim, dim, my_dot, nq, lf->vnorm2[ord]);
      uint64_t key = 0ull;
      if (!(min_score > 0.0f) || s >= min_score) key = pack_key(s * boost, (uint32_t)(lf->doc_base + doc));
      cand[(size_t)q * cap + i] = key;
    }
  }
}

// max_rows: an upper bound of *count the host knows (the grid is sized by it); queries: piece order, 64 x steps bytes each
int launch_knn_gather_bytes(hipStream_t st, const DKnnGatherLeaf* leaves, const uint64_t* list, const uint32_t* count, uint32_t max_rows,
                            int32_t dim, const void* queries, const int32_t* qnorm2, int32_t n_q, int32_t sim, float boost, float min_score,
                            uint64_t* cand, uint32_t* cand_cnt, uint32_t cap) {
  if (max_rows == 0 || n_q <= 0) return 0;
  if (n_q > 64 || dim < 1 || dim > 2048 || max_rows > cap) return (int)hipErrorInvalidValue;
  const uint32_t per_block = 4u * (uint32_t)kByteRescoreRows;
  hipLaunchKernelGGL(knn_gather_bytes_kernel, dim3((max_rows + per_block - 1) / per_block, (uint32_t)n_q), dim3(256), 0, st, leaves, list, count,
                     knn_bytes_steps(dim), dim, (const i32x4*)queries, qnorm2, sim, boost, min_score, cand, cand_cnt, cap);
  return 0;
}

}  // namespace nrtgpu
