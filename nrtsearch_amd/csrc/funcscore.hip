// funcscore.hip -- the gfx950 kernel of function-score queries (MultiFunctionScoreQuery with weight functions over a BM25
// disjunction; the reference's src/main/java/com/yelp/nrtsearch/server/query/multifunction/MultiFunctionScoreQuery.java).
//
//   bm25_function_score_kernel   postings traversal + BM25Similarity + disjunction sum, then PER DOC the function score
//                                (plan.h: function_score_value), the minScore test and the item's top-k of FINAL scores
//
// The reference creates the inner weight with ScoreMode.COMPLETE and its scorer answers getMaxScore = Float.MAX_VALUE
// (:168-174, :503-505): nothing is pruned, every live matching doc is scored and counted.  That is the exhaustive scan's
// contract (kernels.hip) with an epilogue between "sum of the clause scores" and "key into the top-k" -- which is why the scan
// itself cannot serve: it prunes in ACCUMULATOR space (acc_reaches(v, thr)) and derives candidate scores from accumulators at
// three places, and a per-doc factor breaks both.  Here theta bounds FINAL keys only and never meets an accumulator.
//
// It consumes the scan's plan records (DItem / DPart / DTerm / DQuery) and writes the scan's item outputs (item_keys unsorted,
// item_counts, item_hits, per-slice sums), so expand_terms_kernel in front and merge_topk_kernel / slice_relation_kernel behind
// are the existing ones.  Fixed-point accumulators only (ds_add_u64, marker 0): the sums are exact in any order.
//
// Work decomposition: one workgroup of kScanWaves waves per item; the item's sub-tiles (kTileDocs docs) are taken in ROUNDS of
// one sub-tile per wave.  In a round every wave on its own streams its sub-tile's postings into its private LDS accumulators,
// then sweeps them: accept set, inner score, function membership (one 64-bit word per function and 64 docs, a wave-uniform
// load), final score, hit test, key -- and leaves the candidate keys in place of the accumulators.  One barrier; then the
// waves append their candidates to the shared buffer at positions every thread derives from the per-wave counts (no atomics),
// or, when the round's candidates do not fit, wave by wave with a top-k compaction (topk.hiph) wherever the buffer would
// overflow -- a compacted buffer (<= k keys) always takes one wave's sub-tile (plan.h: kFsCandCap).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "finalscore.hiph"

namespace nrtgpu {

struct FuncSmem {
  uint64_t acc[kScanWaves][kTileDocs];   // per wave: fixed-point sums of its sub-tile, then its candidate keys (0: none)
  FinalSmem<kScanWaves, kFsCandCap> t;
};
static_assert(sizeof(FuncSmem) <= 160 * 1024, "the workgroup owns one CU's 160 KiB LDS");

__global__ __launch_bounds__(kScanThreads, kScanWaves / 4)
void bm25_function_score_kernel(const DItem* __restrict__ items, const DPart* __restrict__ parts, const DTerm* __restrict__ terms,
                                const DQuery* __restrict__ queries, const float* __restrict__ caches,
                                const DFuncQuery* __restrict__ fqueries, const DFuncMasks* __restrict__ fmasks,
                                unsigned long long* __restrict__ theta_g, uint32_t* __restrict__ slice_sum, uint32_t* __restrict__ slice_past,
                                uint64_t* __restrict__ item_keys, uint32_t* __restrict__ item_counts, uint64_t* __restrict__ item_hits,
                                uint32_t k_stride) {
  __shared__ FuncSmem s;
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), lane = tid & 63u;
  uint64_t* const acc = &s.acc[wave][0];
  const DItem* const item = items + blockIdx.x;
  const uint32_t query = item->query, part_begin = item->part_begin, n_parts = item->n_parts;
  const int fx_E = item->fx_E;
  const DQuery* const q = queries + query;
  const uint32_t k = min(q->k, (uint32_t)kMaxK);
  const DFuncQuery* const fq = fqueries + query;
  const uint32_t n_functions = min((uint32_t)fq->n_functions, (uint32_t)kMaxFunctions);
  const bool multi_item = q->n_items > 1;
  unsigned long long* const my_theta_g = theta_g + query;
  // searchAfter compares FINAL scores: a hit at or above after_key was collected on an earlier page (it still counts)
  const uint64_t after_key = q->has_after ? pack_key(q->after_score, (uint32_t)q->after_doc) : ~0ull;

  final_prologue(s.t, acc, nullptr, item, caches, tid, lane);

  const uint32_t total_tiles = final_total_tiles(parts, part_begin, n_parts);
  uint64_t theta = 0;   // uniform: the k-th best FINAL key known (this item's compactions, the query's other items)
  uint32_t cnt = 0;     // uniform: keys in s.t.cand
  uint32_t pi = 0;      // the part of the wave's sub-tile (indices only grow)
  uint32_t par = 0;

  for (uint32_t g0 = 0; g0 < total_tiles; g0 += (uint32_t)kScanWaves, par ^= 1u) {
    if (multi_item) {   // what the query's other items have published (a bound on final keys: at least k docs of the query exceed it)
      const uint64_t t = __hip_atomic_load(my_theta_g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      theta = t > theta ? t : theta;
    }
    const uint32_t g = g0 + wave;
    uint32_t n_cand = 0;   // wave-uniform
    if (g < total_tiles) {
      const FinalTile tl = final_tile(parts, part_begin, n_parts, g, pi);
      const DPart* const part = tl.part;
      const uint32_t tile = tl.tile, base = tl.base, tile_len = tl.tile_len, gdoc0 = tl.gdoc0;

      // ---- (1) accumulate: every clause's postings of the sub-tile.  Lane l looks up the posting range of clause l (one memory
      //      round trip for all clauses); a clause's postings are then taken 4 x 64 at a time, the eight column loads of a lane
      //      in flight together.
      const uint32_t n_terms = min(part->n_terms, (uint32_t)kMaxTerms);
      const DTerm* const part_terms = terms + part->term_begin;
      uint32_t my_lo = 0, my_hi = 0;
      if (lane < n_terms) final_clause_range(part_terms + lane, tile, my_lo, my_hi);
      for (uint32_t t = 0; t < n_terms; ++t) {
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)my_lo, (int)t), hi = (uint32_t)__builtin_amdgcn_readlane((int)my_hi, (int)t);
        if (lo >= hi) continue;   // uniform
        final_stream_clause(part_terms + t, lo, hi, base, tile_len, lane, s.t.cache,
                            [acc](uint32_t off, float, unsigned long long v) { atomicAdd((unsigned long long*)&acc[off], v); });
      }

      // ---- (2) sweep: slot lane + 64 j is doc base + 64 j + lane, i.e. bit `lane` of word j of the sub-tile's mask words
      const NRT_GLOBAL uint64_t* const live_bits = (const NRT_GLOBAL uint64_t*)part->live_bits;
      const DFuncMasks* const fm = fmasks + part_begin + pi;
      const uint32_t word0 = base >> 6;
      uint32_t wave_hits = 0, wave_past = 0;
#pragma unroll 2
      for (int j = 0; j < kFinalSlots; ++j) {
        const uint32_t i = lane + 64u * (uint32_t)j;
        const uint64_t v = acc[i];
        uint64_t key = 0;
        if (64u * (uint32_t)j < tile_len) {   // uniform: the words below exist
          const uint32_t wi = word0 + (uint32_t)j;
          bool ok = v != 0ull;
          if (live_bits != nullptr) ok = ok && ((live_bits[wi] >> lane) & 1ull) != 0ull;
          uint32_t matched = 0;
          for (uint32_t fi = 0; fi < n_functions; ++fi) {
            const NRT_GLOBAL uint64_t* const m = (const NRT_GLOBAL uint64_t*)fm->mask[fi];
            const uint64_t mw = m != nullptr ? m[wi] : ~0ull;
            matched |= (uint32_t)((mw >> lane) & 1ull) << fi;
          }
          key = final_candidate_key(ok, gdoc0 + i, theta, after_key, wave_hits, wave_past,
                                    [fq, matched, v, fx_E](bool* hit) { return function_score_value(*fq, matched, acc_score<true>(v, fx_E), hit); });
        }
        acc[i] = key;
        n_cand += (uint32_t)__popcll(__ballot(key != 0ull));
      }
      final_count_slice(s.t, part, lane, wave_hits, wave_past);
    }
    if (lane == 0) s.t.wcount[par][wave] = n_cand;
    __syncthreads();

    // ---- (3) the round's candidates into the shared buffer
    uint32_t tot = 0, before = 0;
#pragma unroll
    for (uint32_t w2 = 0; w2 < (uint32_t)kScanWaves; ++w2) {
      const uint32_t c = s.t.wcount[par][w2];
      tot += c;
      before += w2 < wave ? c : 0u;
    }
    if (cnt + tot <= (uint32_t)kFsCandCap) {   // uniform
      final_push_candidates(s.t, acc, lane, cnt + before);
      cnt += tot;
    } else {
      for (uint32_t w2 = 0; w2 < (uint32_t)kScanWaves; ++w2) {
        const uint32_t c = s.t.wcount[par][w2];
        if (cnt + c > (uint32_t)kFsCandCap) {   // uniform; cnt > k here (kFsCandCap >= kMaxK + kTileDocs)
          __syncthreads();   // the keys appended so far are in place
          uint64_t thr = 0;
          cnt = topk_compact<kScanThreads, kFsCandCap>(s.t.cand, cnt, k, &s.t.sc, &thr);
          if (thr > theta) theta = thr;
          if (tid == 0) atomicMax(my_theta_g, (unsigned long long)thr);   // LazyMaxScoreAccumulator.accumulate analogue
        }
        if (wave == w2) final_push_candidates(s.t, acc, lane, cnt);
        cnt += c;
      }
    }
  }

  final_epilogue(s.t, cnt, k, q, tid, slice_sum, item_keys, item_counts, item_hits, k_stride, slice_past);
}

// slice_relation_past_kernel: slice_relation_kernel's rule (kernels.hip) for the routes that also count, per (query, slice), the
// hits BEHIND the query's cursor (finalscore.hiph: slice_past).  A collector with a cursor counts every hit but queues only those behind it, and publishes no
// min competitive score before its queue is full: the slice must hold more than the floor AND numHits of them behind the cursor.
// (slice_relation_kernel leaves that to its caller's test that the merged page is full -- which, with a cursor, several slices
// can fill together when none of them could alone.)
__global__ __launch_bounds__(256)
void slice_relation_past_kernel(const uint32_t* __restrict__ slice_sum, const uint32_t* __restrict__ slice_past, const DQuery* __restrict__ queries,
                                uint32_t n_slices, uint64_t* __restrict__ out_hits, uint32_t n) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n) return;
  if ((out_hits[q] >> 48) != 0ull) return;
  const uint32_t floor_ = queries[q].gte_floor;
  if (floor_ == 0xFFFFFFFFu) return;
  const uint32_t* sums = slice_sum + queries[q].slice_base;
  const uint32_t* past = slice_past + queries[q].slice_base;
  const bool cursor = queries[q].has_after != 0u;
  const uint32_t k = queries[q].k;
  bool gte = false;
  for (uint32_t i = 0; i < n_slices; ++i) gte = gte || (sums[i] > floor_ && (!cursor || past[i] >= k));
  if (gte) out_hits[q] += kHitsPrunedUnit;
}
void launch_slice_relation_past(hipStream_t stream, const uint32_t* slice_sum, const uint32_t* slice_past, const DQuery* queries, uint32_t n_slices,
                                uint64_t* out_hits, uint32_t n) {
  if (n == 0) return;
  hipLaunchKernelGGL(slice_relation_past_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, slice_sum, slice_past, queries, n_slices, out_hits, n);
}

void launch_bm25_function_score(hipStream_t stream, const FinalScoreArgs& a, const DFuncQuery* fqueries, const DFuncMasks* fmasks) {
  if (a.n_items == 0) return;
  hipLaunchKernelGGL(bm25_function_score_kernel, dim3(a.n_items), dim3(kScanThreads), 0, stream, a.items, a.parts, a.terms, a.queries, a.caches,
                     fqueries, fmasks, a.theta_g, a.slice_sum, a.slice_past, a.item_keys, a.item_counts, a.item_hits, a.k_stride);
}

}  // namespace nrtgpu
