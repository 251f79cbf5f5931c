// rangecount.hip -- the gfx950 kernel of the numeric range facet (include/nrtgpu.h: nrtgpu_count_ranges_batch; the reference's
// Facet.numericRange, clientlib/src/main/proto/yelp/nrtsearch/search.proto:1285-1327, served by DrillSidewaysImpl.java:334-409:
// LongRange[] -> LongRangeFacetCounts for INT / LONG fields, DoubleRange[] -> DoubleRangeFacetCounts for DOUBLE fields).
//
//   bm25_range_count_kernel<WIDE>   postings traversal that only COUNTS the matching clauses per doc (the terms route's
//                                   accumulate), then per doc the hit test and, for a hit with a value, +1 on the counter of
//                                   the ELEMENTARY INTERVAL its code lies in (plan.h: range_interval).  WIDE: the column holds
//                                   64-bit codes (LONG / DATE_TIME / DOUBLE), the cuts are 64-bit
//
// The frame is bm25_terms_count_kernel's (termscount.hip), statement for statement: one workgroup of kScanWaves waves per item,
// rounds of one sub-tile per wave, the column requested BEFORE the accumulate phase, final_count_clause into 4-byte slots, the
// per-word hit test and ballot, final_count_slice, the epilogue of an item without candidates.  Three things differ:
//   LDS      the 12 x 1024 clause counts, the query's cuts (at most 1 KiB, copied in the prologue) and n_cuts + 1 four-byte
//            counters.  No 64 KiB table, no probing, no overflow state
//   per hit  the lanes of a 64-doc word that holds a valued hit search their codes among the LDS cuts -- a search whose step
//            count depends on n_cuts alone -- and each hit's lane does ONE 4-byte LDS add on its interval's counter.  Two
//            experiments of this change's own, MEASURED and not in the tree: searching in the hit lanes alone made
//            no line faster and sparse doc sets 12 % slower; combining the lanes that share the first hit's interval into one add
//            (readlane, ballot, popcount) removes a cliff where every doc is a hit and nine hits in ten fall into one interval,
//            and costs every other case a quarter of the kernel's time
//   flush    behind the one barrier: one global atomicAdd per non-zero counter into the query's counters, which its items share
// A single-valued column counts a doc once: every counter stays below 2^31.  The host rolls the intervals up into the ranges
// (rangecount.cpp).  All writes are vector stores and atomics in plain HIP; every loop is bounded by a count known on entry.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "finalscore.hiph"

namespace nrtgpu {

template <class CODE>
struct RangeCountSmem {
  uint32_t acc[kScanWaves][kTileDocs];          // per wave: clause counts of its sub-tile
  CODE cuts[kMaxRangeCuts];                     // the query's cut points, ascending
  uint32_t counters[kMaxRangeCuts + 1];         // the item's hits per elementary interval, shared by the waves
  uint32_t slot_hits[kSliceSlots];              // what final_count_slice and the epilogue read (finalscore.hiph: FinalSmem)
  uint32_t slot_slice[kSliceSlots];
};
static_assert(sizeof(RangeCountSmem<uint64_t>) <= 64 * 1024, "two workgroups of the kernel share one CU's 160 KiB LDS");

template <bool WIDE>
__global__ __launch_bounds__(kScanThreads, kScanWaves / 4)
void bm25_range_count_kernel(const DItem* __restrict__ items, const DPart* __restrict__ parts, const DTerm* __restrict__ terms,
                             const DQuery* __restrict__ queries, const DRangeCountQuery* __restrict__ rqueries,
                             const DSortPart* __restrict__ sparts, const void* __restrict__ cuts_g, uint32_t* __restrict__ counters_g,
                             uint32_t* __restrict__ slice_sum, uint32_t* __restrict__ item_counts, uint64_t* __restrict__ item_hits) {
  typedef typename std::conditional<WIDE, uint64_t, uint32_t>::type CODE;
  __shared__ RangeCountSmem<CODE> s;
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), lane = tid & 63u;
  uint32_t* const acc = &s.acc[wave][0];
  const DItem* const item = items + blockIdx.x;
  const uint32_t query = item->query, part_begin = item->part_begin, n_parts = item->n_parts;
  const DQuery* const q = queries + query;
  const DRangeCountQuery* const rq = rqueries + query;
  const uint32_t need = max(rq->need, 1u), n_cuts = min(rq->n_cuts, (uint32_t)kMaxRangeCuts);
  const CODE* const my_cuts = (const CODE*)cuts_g + rq->cut_off;
  uint32_t* const my_counters = counters_g + rq->counter_off;

  // ---- prologue: the wave's counts, the query's cuts, the item's counters, the slice counters; a barrier
  for (int j = 0; j < kFinalSlots; ++j) acc[lane + 64u * (uint32_t)j] = 0u;
  if (tid < n_cuts) s.cuts[tid] = my_cuts[tid];
  if (tid <= (uint32_t)kMaxRangeCuts) s.counters[tid] = 0u;
  if (tid < (uint32_t)kSliceSlots) s.slot_hits[tid] = s.slot_slice[tid] = 0u;
  __syncthreads();

  const uint32_t total_tiles = final_total_tiles(parts, part_begin, n_parts);
  uint32_t pi = 0;      // the part of the wave's sub-tile (indices only grow)

  for (uint32_t g = wave; g < total_tiles; g += (uint32_t)kScanWaves) {
    const FinalTile tl = final_tile(parts, part_begin, n_parts, g, pi);
    const DPart* const part = tl.part;
    const uint32_t tile = tl.tile, base = tl.base, tile_len = tl.tile_len;

    // ---- (0) the sub-tile's column, requested now (fieldsort.hip / fieldsort64.hip).  DSortPart.code is the column of either
    //      width (a call's columns are of one width).  The column is padded to whole sub-tiles: no bounds test.
    const DSortPart* const sp = sparts + part_begin + pi;
    const NRT_GLOBAL CODE* const col = (const NRT_GLOBAL CODE*)sp->code;
    const NRT_GLOBAL uint64_t* const has = (const NRT_GLOBAL uint64_t*)sp->has;
    const uint32_t word0 = base >> 6;
    CODE cv[kFinalSlots];
    uint64_t my_has = ~0ull;
    if (col != nullptr) {   // uniform
#pragma unroll
      for (int j = 0; j < kFinalSlots; ++j) cv[j] = col[base + lane + 64u * (uint32_t)j];
      if (has != nullptr && lane < (uint32_t)kFinalSlots) my_has = has[word0 + lane];
    } else {   // the leaf lacks the column: its hits add to no range
#pragma unroll
      for (int j = 0; j < kFinalSlots; ++j) cv[j] = (CODE)0;
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
    for (int j = 0; j < kFinalSlots; ++j) {   // (unrolled: cv[j] is a register, or a pair)
      if (64u * (uint32_t)j >= tile_len) continue;   // uniform: the words below do not exist, the slots counted nothing
      const uint32_t i = lane + 64u * (uint32_t)j;
      const uint64_t hw = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)has_hi, j) << 32) | (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)has_lo, j);
      bool hit = acc[i] >= need;   // (a slot beyond max_doc counted nothing)
      acc[i] = 0u;
      if (live_bits != nullptr) hit = hit && ((live_bits[word0 + (uint32_t)j] >> lane) & 1ull) != 0ull;
      const unsigned long long hits = __ballot(hit);
      wave_hits += (uint32_t)__popcll(hits);
      const unsigned long long valued = hits & hw;   // uniform: the word's hits that have a value
      if (valued == 0ull) continue;                  // uniform
      // Every lane of a word with a valued hit searches, the hit lanes add.  Searching in the hit lanes alone was built and
      // MEASURED: no line got faster, a doc set at a permille accepted 12 % slower.
      const uint32_t iv = range_interval(s.cuts, n_cuts, cv[j]);
      if (((valued >> lane) & 1ull) != 0ull) atomicAdd(&s.counters[iv], 1u);
    }
    final_count_slice(s, part, lane, wave_hits);
  }

  // ---- the item's counters into the query's, once
  __syncthreads();
  if (tid <= n_cuts) {
    const uint32_t c = s.counters[tid];
    if (c != 0u) atomicAdd(&my_counters[tid], c);
  }

  // ---- epilogue: final_epilogue's for an item without candidates
  if (tid == 0) {
    item_counts[blockIdx.x] = 0u;
    uint32_t hits = 0;
    const uint32_t gte_floor = q->gte_floor, slice_base = q->slice_base;
    for (int i = 0; i < kSliceSlots; ++i) {
      const uint32_t h = s.slot_hits[i];
      hits += h;
      if (h != 0u && gte_floor != 0xFFFFFFFFu) atomicAdd(&slice_sum[slice_base + s.slot_slice[i]], h);
    }
    item_hits[blockIdx.x] = hits;
  }
}

void launch_bm25_range_count(hipStream_t stream, bool wide, const FinalScoreArgs& a, const DRangeCountQuery* rqueries, const DSortPart* sparts,
                             const void* cuts, uint32_t* counters) {
  if (a.n_items == 0) return;
  if (wide)
    hipLaunchKernelGGL(bm25_range_count_kernel<true>, dim3(a.n_items), dim3(kScanThreads), 0, stream, a.items, a.parts, a.terms, a.queries, rqueries, sparts,
                       cuts, counters, a.slice_sum, a.item_counts, a.item_hits);
  else
    hipLaunchKernelGGL(bm25_range_count_kernel<false>, dim3(a.n_items), dim3(kScanThreads), 0, stream, a.items, a.parts, a.terms, a.queries, rqueries, sparts,
                       cuts, counters, a.slice_sum, a.item_counts, a.item_hits);
}

}  // namespace nrtgpu
