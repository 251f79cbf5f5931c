// fieldsort64.hip -- the gfx950 kernel of sort by a 64-BIT field (include/nrtgpu.h: nrtgpu_search_sorted64_batch; the reference's
// DateTimeFieldDef / LongFieldDef / DoubleFieldDef.getSortField: SortField.Type.LONG / DOUBLE under TopFieldCollectorManager).
//
//   bm25_field_sort64_kernel   bm25_field_sort_kernel (fieldsort.hip) over a column of 64-bit codes
//
// The structure is that kernel's, line for line: one workgroup of kScanWaves waves per item, rounds of one sub-tile per wave, the
// clause counts in the wave's LDS slots, the shared candidate buffer with the wave-by-wave compaction, theta_g between a query's
// items, final_epilogue.  Three things differ:
//   column   a lane holds the sub-tile's kFinalSlots codes as 8-byte values (one coalesced 8-byte load per lane and 64-doc word,
//            requested BEFORE the accumulate phase like the 4-byte column's: DESIGN 4.1f) -- 32 more VGPRs than the 32-bit kernel,
//            inside the 168 of three waves per SIMD.  The column is padded to whole sub-tiles: no bounds test.
//   key      plan.h: sort_key64 -- the ordinal of the doc's code in the query's window [lo, lo + span] above a db-bit docid field
//            (DSort64Query); keys of one query are comparable across its items and leaves, because the packing is per query, so
//            theta_g, the merge and the per-slice relation are the unchanged ones
//   cursor   tested on (code, doc), not on keys (plan.h: sort64_behind): a cursor value outside the window must not collapse onto
//            a sentinel ordinal
// Integer compares only: exact.  No inline assembly; all global writes are the skeleton's vector stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "finalscore.hiph"

namespace nrtgpu {

struct Sort64Smem {
  uint64_t acc[kScanWaves][kTileDocs];   // per wave: clause counts of its sub-tile (low word), then its candidate keys (0: none)
  FinalSmem<kScanWaves, kFsCandCap> t;   // the skeleton's shared state (its `cache` is carried, neither written nor read)
};
static_assert(sizeof(Sort64Smem) <= 160 * 1024, "the workgroup owns one CU's 160 KiB LDS");

__global__ __launch_bounds__(kScanThreads, kScanWaves / 4)
void bm25_field_sort64_kernel(const DItem* __restrict__ items, const DPart* __restrict__ parts, const DTerm* __restrict__ terms,
                              const DQuery* __restrict__ queries, const DSort64Query* __restrict__ squeries,
                              const DSort64Part* __restrict__ sparts, unsigned long long* __restrict__ theta_g,
                              uint32_t* __restrict__ slice_sum, uint64_t* __restrict__ item_keys, uint32_t* __restrict__ item_counts,
                              uint64_t* __restrict__ item_hits, uint32_t k_stride) {
  __shared__ Sort64Smem s;
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), lane = tid & 63u;
  uint64_t* const acc = &s.acc[wave][0];
  const DItem* const item = items + blockIdx.x;
  const uint32_t query = item->query, part_begin = item->part_begin, n_parts = item->n_parts;
  const DQuery* const q = queries + query;
  const uint32_t k = min(q->k, (uint32_t)kMaxK);
  const DSort64Query* const sq = squeries + query;
  const uint64_t lo = sq->lo, span = sq->span, missing_code = sq->missing_code, after_code = sq->after_code;
  const uint32_t reverse = sq->reverse, need = max(sq->need, 1u), after_doc = sq->after_doc;
  const uint32_t db = min(max(sq->db, 1u), 31u);
  const bool has_after = sq->has_after != 0u;
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

      // ---- (0) the sub-tile's column: its kFinalSlots 8-byte codes per lane and its `has` words (lane j: word j), requested
      //      now -- their latency passes behind the accumulate phase.  The column is padded to whole sub-tiles: no bounds test.
      const DSort64Part* const sp = sparts + part_begin + pi;
      const NRT_GLOBAL uint64_t* const col = (const NRT_GLOBAL uint64_t*)sp->code64;
      const NRT_GLOBAL uint64_t* const has = (const NRT_GLOBAL uint64_t*)sp->has;
      const uint32_t word0 = base >> 6;
      uint64_t cv[kFinalSlots];
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
        const uint32_t plo = (uint32_t)__builtin_amdgcn_readlane((int)my_lo, (int)t), phi = (uint32_t)__builtin_amdgcn_readlane((int)my_hi, (int)t);
        if (plo >= phi) continue;   // uniform
        final_count_clause(part_terms + t, plo, phi, base, tile_len, lane, acc);
      }

      // ---- (2) sweep: slot lane + 64 j is doc base + 64 j + lane, i.e. bit `lane` of word j of the sub-tile's mask words
      const NRT_GLOBAL uint64_t* const live_bits = (const NRT_GLOBAL uint64_t*)part->live_bits;
      const uint32_t has_lo = (uint32_t)my_has, has_hi = (uint32_t)(my_has >> 32);
      uint32_t wave_hits = 0;
#pragma unroll
      for (int j = 0; j < kFinalSlots; ++j) {   // (unrolled: cv[j] is a register pair)
        const uint32_t i = lane + 64u * (uint32_t)j;
        uint64_t key = 0;
        if (64u * (uint32_t)j < tile_len) {   // uniform: the words below exist
          const uint32_t wi = word0 + (uint32_t)j;
          const uint64_t hw = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)has_hi, j) << 32) | (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)has_lo, j);
          const uint64_t code = ((hw >> lane) & 1ull) != 0ull ? cv[j] : missing_code;
          bool hit = (uint32_t)acc[i] >= need;   // (a slot beyond max_doc counted nothing)
          if (live_bits != nullptr) hit = hit && ((live_bits[wi] >> lane) & 1ull) != 0ull;
          const uint32_t gdoc = gdoc0 + i;
          const uint64_t doc_key = sort_key64(reverse, lo, span, db, code, gdoc);
          // totalHits counts every hit, also those an earlier page returned
          if (hit && doc_key > theta && (!has_after || sort64_behind(reverse, code, gdoc, after_code, after_doc))) key = doc_key;
          wave_hits += (uint32_t)__popcll(__ballot(hit));
        }
        acc[i] = key;
        n_cand += (uint32_t)__popcll(__ballot(key != 0ull));
      }
      final_count_slice(s.t, part, lane, wave_hits);
    }
    if (lane == 0) s.t.wcount[par][wave] = n_cand;
    __syncthreads();

    // ---- (3) the round's candidates into the shared buffer (fieldsort.hip's meeting)
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

void launch_bm25_field_sort64(hipStream_t stream, const FinalScoreArgs& a, const DSort64Query* squeries, const DSort64Part* sparts) {
  if (a.n_items == 0) return;
  hipLaunchKernelGGL(bm25_field_sort64_kernel, dim3(a.n_items), dim3(kScanThreads), 0, stream, a.items, a.parts, a.terms, a.queries, squeries, sparts,
                     a.theta_g, a.slice_sum, a.item_keys, a.item_counts, a.item_hits, a.k_stride);
}

}  // namespace nrtgpu
