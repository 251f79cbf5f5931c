// fieldsort.hip -- the gfx950 kernel of sort by field (include/nrtgpu.h: nrtgpu_search_sorted_batch; the reference's
// src/main/java/com/yelp/nrtsearch/server/search/collectors/SortFieldCollector.java: TopFieldCollectorManager over ONE int or
// float SortField).
//
//   bm25_field_sort_kernel   postings traversal that only COUNTS the matching clauses per doc, then per doc the hit test
//                            (clause count, accept set), the key from the doc's column value and the item's top-k of keys
//
// The skeleton is the final-score kernels' (finalscore.hiph; the shape of bm25_function_score_kernel, funcscore.hip): one
// workgroup of kScanWaves waves per item, rounds of one sub-tile per wave, the shared candidate buffer with the wave-by-wave
// compaction where a round's candidates do not fit, theta_g between a query's items, final_epilogue.  What differs:
//   accumulate  a clause's docid and code columns are streamed (the code carries the "doc is deleted" mark when liveDocs are
//               folded into the postings) and 1 is added per live posting to the doc's LDS slot: no BM25 arithmetic, no
//               normInverse tables
//   column      a sub-tile's codes -- one coalesced 4-byte load per lane and 64-doc word; the column is padded to whole sub-tiles:
//               no per-lane bounds test -- and its `has` words (lane j: word j) depend on nothing the postings bring: they are
//               requested BEFORE the accumulate phase and wait in registers: requested inside the sweep they would be dependent
//               memory round trips per sub-tile that nothing overlaps
//   sweep       per 64-doc word of the sub-tile: the `has` word by readlane, the lane's code, the key (plan.h: sort_key), the
//               theta / after test, the hit count
// The key's high word is the ORDER-PRESERVING CODE of the value (complemented for an ascending sort) where the other routes have
// score bits: it may have its top bit set, which topk.hiph, merge_topk_kernel and slice_relation_kernel do not mind (they compare
// keys as unsigned 64-bit integers and bucket high words by unsigned differences).  The route is integer compares only: exact.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "finalscore.hiph"

namespace nrtgpu {

struct SortSmem {
  uint64_t acc[kScanWaves][kTileDocs];   // per wave: clause counts of its sub-tile (low word), then its candidate keys (0: none)
  // The skeleton's shared state.  Its `cache` (the normInverse tables final_prologue stages on the scoring routes) is carried but
  // neither written nor read here: no score is computed.  One workgroup per CU either way.
  FinalSmem<kScanWaves, kFsCandCap> t;
};
static_assert(sizeof(SortSmem) <= 160 * 1024, "the workgroup owns one CU's 160 KiB LDS");

// The sweep's verdict on one doc: its key when it is a hit between theta and the cursor, else 0.  totalHits counts every hit,
// also those an earlier page returned.  All lanes of the wave call.
__device__ __forceinline__ uint64_t sort_candidate_key(bool hit, uint64_t doc_key, uint64_t theta, bool has_after, uint64_t after_key,
                                                       uint32_t& wave_hits) {
  uint64_t key = 0;
  if (hit && doc_key > theta && (!has_after || doc_key < after_key)) key = doc_key;
  wave_hits += (uint32_t)__popcll(__ballot(hit));
  return key;
}

__global__ __launch_bounds__(kScanThreads, kScanWaves / 4)
void bm25_field_sort_kernel(const DItem* __restrict__ items, const DPart* __restrict__ parts, const DTerm* __restrict__ terms,
                            const DQuery* __restrict__ queries, const DSortQuery* __restrict__ squeries,
                            const DSortPart* __restrict__ sparts, unsigned long long* __restrict__ theta_g,
                            uint32_t* __restrict__ slice_sum, uint64_t* __restrict__ item_keys, uint32_t* __restrict__ item_counts,
                            uint64_t* __restrict__ item_hits, uint32_t k_stride) {
  __shared__ SortSmem s;
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), lane = tid & 63u;
  uint64_t* const acc = &s.acc[wave][0];
  const DItem* const item = items + blockIdx.x;
  const uint32_t query = item->query, part_begin = item->part_begin, n_parts = item->n_parts;
  const DQuery* const q = queries + query;
  const uint32_t k = min(q->k, (uint32_t)kMaxK);
  const DSortQuery* const sq = squeries + query;
  const uint32_t reverse = sq->reverse, missing_code = sq->missing_code, need = max(sq->need, 1u);
  const bool has_after = sq->has_after != 0u;
  const uint64_t after_key = sq->after_key;
  const bool multi_item = q->n_items > 1;
  unsigned long long* const my_theta_g = theta_g + query;

  // ---- prologue: the wave's markers, the slice counters (no normInverse tables on this route); a barrier
  for (int j = 0; j < kFinalSlots; ++j) acc[lane + 64u * (uint32_t)j] = 0ull;
  if (tid < (uint32_t)kSliceSlots) s.t.slot_hits[tid] = s.t.slot_slice[tid] = 0u;
  __syncthreads();

  const uint32_t total_tiles = final_total_tiles(parts, part_begin, n_parts);
  uint64_t theta = 0;   // uniform: the k-th best key known (this item's compactions, the query's other items)
  uint32_t cnt = 0;     // uniform: keys in s.t.cand
  uint32_t pi = 0;      // the part of the wave's sub-tile (indices only grow)
  uint32_t par = 0;

  for (uint32_t g0 = 0; g0 < total_tiles; g0 += (uint32_t)kScanWaves, par ^= 1u) {
    if (multi_item) {   // what the query's other items have published (at least k docs of the query exceed it)
      const uint64_t t = __hip_atomic_load(my_theta_g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      theta = t > theta ? t : theta;
    }
    const uint32_t g = g0 + wave;
    uint32_t n_cand = 0;   // wave-uniform
    if (g < total_tiles) {
      const FinalTile tl = final_tile(parts, part_begin, n_parts, g, pi);
      const DPart* const part = tl.part;
      const uint32_t tile = tl.tile, base = tl.base, tile_len = tl.tile_len, gdoc0 = tl.gdoc0;

      // ---- (0) the sub-tile's column: its kFinalSlots codes per lane and its `has` words (lane j: word j) are requested now --
      //      they depend on nothing the postings bring, and their latency passes behind the accumulate phase.  The column is
      //      padded to whole sub-tiles: no bounds test.
      const DSortPart* const sp = sparts + part_begin + pi;
      const NRT_GLOBAL uint32_t* const col = (const NRT_GLOBAL uint32_t*)sp->code;
      const NRT_GLOBAL uint64_t* const has = (const NRT_GLOBAL uint64_t*)sp->has;
      const uint32_t word0 = base >> 6;
      uint32_t cv[kFinalSlots];
      uint64_t my_has = ~0ull;
      if (col != nullptr) {   // uniform
#pragma unroll
        for (int j = 0; j < kFinalSlots; ++j) cv[j] = col[base + lane + 64u * (uint32_t)j];
        if (has != nullptr && lane < (uint32_t)kFinalSlots) my_has = has[word0 + lane];
      } else {
#pragma unroll
        for (int j = 0; j < kFinalSlots; ++j) cv[j] = missing_code;
        my_has = 0ull;
      }

      // ---- (1) accumulate: every clause's postings of the sub-tile, one count per live posting
      const uint32_t n_terms = min(part->n_terms, (uint32_t)kMaxTerms);
      const DTerm* const part_terms = terms + part->term_begin;
      uint32_t my_lo = 0, my_hi = 0;
      if (lane < n_terms) final_clause_range(part_terms + lane, tile, my_lo, my_hi);
      for (uint32_t t = 0; t < n_terms; ++t) {
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)my_lo, (int)t), hi = (uint32_t)__builtin_amdgcn_readlane((int)my_hi, (int)t);
        if (lo >= hi) continue;   // uniform
        final_count_clause(part_terms + t, lo, hi, base, tile_len, lane, acc);
      }

      // ---- (2) sweep: slot lane + 64 j is doc base + 64 j + lane, i.e. bit `lane` of word j of the sub-tile's mask words
      const NRT_GLOBAL uint64_t* const live_bits = (const NRT_GLOBAL uint64_t*)part->live_bits;
      const uint32_t has_lo = (uint32_t)my_has, has_hi = (uint32_t)(my_has >> 32);
      uint32_t wave_hits = 0;
#pragma unroll
      for (int j = 0; j < kFinalSlots; ++j) {   // (unrolled: cv[j] is a register)
        const uint32_t i = lane + 64u * (uint32_t)j;
        uint64_t key = 0;
        if (64u * (uint32_t)j < tile_len) {   // uniform: the words below exist
          const uint32_t wi = word0 + (uint32_t)j;
          const uint64_t hw = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)has_hi, j) << 32) | (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)has_lo, j);
          const uint32_t code = ((hw >> lane) & 1ull) != 0ull ? cv[j] : missing_code;
          bool hit = (uint32_t)acc[i] >= need;   // (a slot beyond max_doc counted nothing)
          if (live_bits != nullptr) hit = hit && ((live_bits[wi] >> lane) & 1ull) != 0ull;
          key = sort_candidate_key(hit, sort_key(reverse, code, gdoc0 + i), theta, has_after, after_key, wave_hits);
        }
        acc[i] = key;
        n_cand += (uint32_t)__popcll(__ballot(key != 0ull));
      }
      final_count_slice(s.t, part, lane, wave_hits);
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

  final_epilogue(s.t, cnt, k, q, tid, slice_sum, item_keys, item_counts, item_hits, k_stride);
}

void launch_bm25_field_sort(hipStream_t stream, const FinalScoreArgs& a, const DSortQuery* squeries, const DSortPart* sparts) {
  if (a.n_items == 0) return;
  hipLaunchKernelGGL(bm25_field_sort_kernel, dim3(a.n_items), dim3(kScanThreads), 0, stream, a.items, a.parts, a.terms, a.queries, squeries, sparts,
                     a.theta_g, a.slice_sum, a.item_keys, a.item_counts, a.item_hits, a.k_stride);
}

}  // namespace nrtgpu
