// termscount.hip -- the gfx950 kernels of the terms aggregation (include/nrtgpu.h: nrtgpu_count_terms_batch; the reference's
// src/main/java/com/yelp/nrtsearch/server/search/collectors/additional/IntTermsCollectorManager.java:142-152 and
// FloatTermsCollectorManager.java:149-150: countsMap.addTo(value, 1) for every collected doc).
//
//   bm25_terms_count_kernel   postings traversal that only COUNTS the matching clauses per doc (the sorted route's accumulate),
//                             then per doc the hit test and, for a hit with a value, +1 in the count table under the value's code
//   terms_compact_kernel      per query: the occupied slots of its global table, packed into the call's entry list
//   bm25_terms_count_multi_kernel   the first for calls that count a MULTI-VALUED column: every value of a hit adds 1
//
// The decomposition is the final-score skeleton's (finalscore.hiph): one workgroup of kScanWaves waves per item, rounds of one
// sub-tile per wave, final_total_tiles / final_tile / final_clause_range / final_count_slice.  What the route does NOT have: a
// candidate buffer, a top-k, theta, 8-byte accumulators -- and so no meeting of the waves per round: a wave's slots are its own,
// the count tables are touched with atomics only, and the one barrier of the round loop's lifetime stands in front of the flush.
// The item reports 0 candidates and its hit count: merge_topk_kernel and slice_relation_kernel behind it return empty lists and
// the exact total_hits as on every route.
//   accumulate  the sorted route's (finalscore.hiph: final_count_clause), into 4-byte slots
//   column      the sub-tile's codes and `has` words are requested BEFORE the accumulate phase, as in fieldsort.hip
//   sweep       per 64-doc word: the hit test (clause count, liveDocs word), the hit count; every hit with a value (`has` bit)
//               adds 1 under its code, lane by lane.  Combining equal codes inside the wave first (leader broadcast, ballot,
//               popcount) was built and MEASURED: a round costs a tenth of the kernel's time and saves nothing,
//               also where 64 lanes share five slots -- there are none
//   tables      plan.h (DTermsQuery): LDS table -> (bounded probe failed) -> the query's global table; the LDS table is flushed
//               into the global one once, behind the item's last round.  No loop waits for another thread: a probe sequence ends
//               after a fixed number of steps, with the value placed, handed on, or the query's overflow flag raised.
// All writes are vector stores and atomics in plain HIP.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "finalscore.hiph"
#include "termstables.hiph"   // terms_lds_add, terms_global_add

namespace nrtgpu {

struct TermsSmem {
  uint32_t acc[kScanWaves][kTileDocs];          // per wave: clause counts of its sub-tile
  unsigned long long table[kTermsLdsSlots];     // the item's count table (plan.h), shared by the waves
  uint32_t slot_hits[kSliceSlots];              // what final_count_slice and the epilogue read (finalscore.hiph: FinalSmem)
  uint32_t slot_slice[kSliceSlots];
};
static_assert(sizeof(TermsSmem) <= 160 * 1024, "the workgroup owns one CU's 160 KiB LDS");

__global__ __launch_bounds__(kScanThreads, kScanWaves / 4)
void bm25_terms_count_kernel(const DItem* __restrict__ items, const DPart* __restrict__ parts, const DTerm* __restrict__ terms,
                             const DQuery* __restrict__ queries, const DTermsQuery* __restrict__ tqueries,
                             const DSortPart* __restrict__ sparts, DTermsState* __restrict__ states, unsigned long long* __restrict__ tables,
                             uint32_t* __restrict__ slice_sum, uint32_t* __restrict__ item_counts, uint64_t* __restrict__ item_hits) {
  __shared__ TermsSmem s;
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), lane = tid & 63u;
  uint32_t* const acc = &s.acc[wave][0];
  const DItem* const item = items + blockIdx.x;
  const uint32_t query = item->query, part_begin = item->part_begin, n_parts = item->n_parts;
  const DQuery* const q = queries + query;
  const DTermsQuery* const tq = tqueries + query;
  const uint32_t need = max(tq->need, 1u), max_buckets = tq->max_buckets, shift = tq->table_shift;
  const uint32_t mask = (1u << (32u - shift)) - 1u;
  unsigned long long* const table = tables + tq->table_off;
  DTermsState* const st = states + query;

  // ---- prologue: the wave's counts, the item's table, the slice counters; a barrier
  for (int j = 0; j < kFinalSlots; ++j) acc[lane + 64u * (uint32_t)j] = 0u;
  for (uint32_t i = tid; i < (uint32_t)kTermsLdsSlots; i += (uint32_t)kScanThreads) s.table[i] = 0ull;
  if (tid < (uint32_t)kSliceSlots) s.slot_hits[tid] = s.slot_slice[tid] = 0u;
  __syncthreads();

  const uint32_t total_tiles = final_total_tiles(parts, part_begin, n_parts);
  uint32_t pi = 0;      // the part of the wave's sub-tile (indices only grow)

  for (uint32_t g = wave; g < total_tiles; g += (uint32_t)kScanWaves) {
    const FinalTile tl = final_tile(parts, part_begin, n_parts, g, pi);
    const DPart* const part = tl.part;
    const uint32_t tile = tl.tile, base = tl.base, tile_len = tl.tile_len;

    // ---- (0) the sub-tile's column, requested now (fieldsort.hip).  The column is padded to whole sub-tiles: no bounds test.
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
    } else {   // the leaf lacks the column: its hits add to no bucket
#pragma unroll
      for (int j = 0; j < kFinalSlots; ++j) cv[j] = 0u;
      my_has = 0ull;
    }
    // an overflowed query's buckets are void: its items go on counting hits only (a flag read once, not waited for)
    const bool counting = __builtin_amdgcn_readfirstlane((int)__hip_atomic_load(&st->overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == 0;

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
      if (64u * (uint32_t)j >= tile_len) continue;   // uniform: the words below do not exist, the slots counted nothing
      const uint32_t i = lane + 64u * (uint32_t)j;
      const uint64_t hw = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)has_hi, j) << 32) | (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)has_lo, j);
      bool hit = acc[i] >= need;   // (a slot beyond max_doc counted nothing)
      acc[i] = 0u;
      if (live_bits != nullptr) hit = hit && ((live_bits[word0 + (uint32_t)j] >> lane) & 1ull) != 0ull;
      const unsigned long long hits = __ballot(hit);
      wave_hits += (uint32_t)__popcll(hits);
      const unsigned long long valued = counting ? (hits & hw) : 0ull;   // uniform: the word's hits that have a value
      if (((valued >> lane) & 1ull) != 0ull) terms_lds_add(s.table, table, shift, mask, max_buckets, st, cv[j], 1u);
    }
    final_count_slice(s, part, lane, wave_hits);
  }

  // ---- the item's table into the query's, once
  __syncthreads();
  if (__hip_atomic_load(&st->overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) {
    for (uint32_t i = tid; i < (uint32_t)kTermsLdsSlots; i += (uint32_t)kScanThreads) {
      const unsigned long long w = s.table[i];
      if (w != 0ull) terms_global_add(table, shift, mask, max_buckets, st, (uint32_t)w, (uint32_t)(w >> 32));
    }
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

// One workgroup per query: the occupied slots of its table, packed behind the other queries' in `out` (the order of the
// queries there is whatever order the workgroups arrive in: DTermsState.out_base says where; the host sorts a query's entries).
// states[n_queries].claimed is the call's cursor.  `out` holds sum(max_buckets) entries: a query that did not overflow has at
// most max_buckets.
constexpr int kCompactThreads = 256;
__global__ __launch_bounds__(kCompactThreads)
void terms_compact_kernel(const DTermsQuery* __restrict__ tqueries, DTermsState* __restrict__ states, const unsigned long long* __restrict__ tables,
                          unsigned long long* __restrict__ out, uint32_t n_queries, uint32_t out_cap) {
  __shared__ uint32_t s_n, s_base, s_pos;
  const uint32_t tid = threadIdx.x, query = blockIdx.x;
  const DTermsQuery* const tq = tqueries + query;
  DTermsState* const st = states + query;
  const uint32_t slots = 1u << (32u - tq->table_shift);
  const unsigned long long* const table = tables + tq->table_off;
  if (tid == 0) s_n = s_pos = 0u;
  __syncthreads();
  if (st->overflow != 0u) return;   // uniform: n_out stays 0
  uint32_t mine = 0;
  for (uint32_t i = tid; i < slots; i += (uint32_t)kCompactThreads) mine += table[i] != 0ull ? 1u : 0u;
  if (mine != 0u) atomicAdd(&s_n, mine);
  __syncthreads();
  const uint32_t n = s_n;   // (<= max_buckets: every claim was counted, and the claim that passed the bound raised the flag)
  if (tid == 0) s_base = atomicAdd(&states[n_queries].claimed, n);
  __syncthreads();
  const uint32_t base = s_base;
  for (uint32_t i = tid; i < slots; i += (uint32_t)kCompactThreads) {
    const unsigned long long w = table[i];
    if (w == 0ull) continue;
    const uint32_t at = base + atomicAdd(&s_pos, 1u);
    if (at < out_cap) out[at] = w;   // (always true)
  }
  if (tid == 0) {
    st->n_out = n;
    st->out_base = base;
  }
}

// bm25_terms_count_kernel for calls in which some query counts a MULTI-VALUED column (plan.h: DSortPart; the reference's
// IntTermsCollectorManager.java:142-152: for (i < docValues.size()) countsMap.addTo(docValues.get(i), 1) -- every value instance
// of every hit adds 1, a value a doc holds twice counts twice).  The arity is the QUERY's (DTermsQuery.need bit 31, uniform over
// the workgroup), so a batch that mixes arities is one launch; a query over a single-valued column takes the statements of the
// kernel above under the flag's branch.  What differs from the kernel above:
//   column      start[d] and start[d + 1] of the sub-tile's docs take the code column's place among the loads requested BEFORE the
//               accumulate phase (two loads per slot: the second falls into the first's cache lines but for one entry per 64);
//               they depend on nothing the postings bring
//   sweep       every hit lane walks its own codes[start[d] .. start[d + 1]) -- neighbouring docs' values are neighbours in
//               codes[], so the lanes' loads of one step fall into few cache lines -- and adds 1 per value.  The loop's bound is
//               the lane's count, read on entry; a word without a valued hit loads no code
// Everything else -- skeleton, accumulate, hit test, tables, flush, epilogue -- is the kernel's above, statement for statement.
__global__ __launch_bounds__(kScanThreads, kScanWaves / 4)
void bm25_terms_count_multi_kernel(const DItem* __restrict__ items, const DPart* __restrict__ parts, const DTerm* __restrict__ terms,
                                   const DQuery* __restrict__ queries, const DTermsQuery* __restrict__ tqueries,
                                   const DSortPart* __restrict__ sparts, DTermsState* __restrict__ states, unsigned long long* __restrict__ tables,
                                   uint32_t* __restrict__ slice_sum, uint32_t* __restrict__ item_counts, uint64_t* __restrict__ item_hits) {
  __shared__ TermsSmem s;
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), lane = tid & 63u;
  uint32_t* const acc = &s.acc[wave][0];
  const DItem* const item = items + blockIdx.x;
  const uint32_t query = item->query, part_begin = item->part_begin, n_parts = item->n_parts;
  const DQuery* const q = queries + query;
  const DTermsQuery* const tq = tqueries + query;
  const uint32_t need = max(tq->need & ~kTermsQueryMulti, 1u), max_buckets = tq->max_buckets, shift = tq->table_shift;
  const bool multi = (tq->need & kTermsQueryMulti) != 0u;   // uniform: the query's count column is multi-valued
  const uint32_t mask = (1u << (32u - shift)) - 1u;
  unsigned long long* const table = tables + tq->table_off;
  DTermsState* const st = states + query;

  for (int j = 0; j < kFinalSlots; ++j) acc[lane + 64u * (uint32_t)j] = 0u;
  for (uint32_t i = tid; i < (uint32_t)kTermsLdsSlots; i += (uint32_t)kScanThreads) s.table[i] = 0ull;
  if (tid < (uint32_t)kSliceSlots) s.slot_hits[tid] = s.slot_slice[tid] = 0u;
  __syncthreads();

  const uint32_t total_tiles = final_total_tiles(parts, part_begin, n_parts);
  uint32_t pi = 0;      // the part of the wave's sub-tile (indices only grow)

  for (uint32_t g = wave; g < total_tiles; g += (uint32_t)kScanWaves) {
    const FinalTile tl = final_tile(parts, part_begin, n_parts, g, pi);
    const DPart* const part = tl.part;
    const uint32_t tile = tl.tile, base = tl.base, tile_len = tl.tile_len;

    // ---- (0) the sub-tile's column, requested now.  Single-valued: cv = the docs' codes.  Multi-valued: cv = start[d],
    //      ce = start[d + 1] (start[] is padded to whole sub-tiles plus one: no bounds test).
    const DSortPart* const sp = sparts + part_begin + pi;
    const NRT_GLOBAL uint32_t* const col = (const NRT_GLOBAL uint32_t*)sp->code;
    const uint32_t word0 = base >> 6;
    uint32_t cv[kFinalSlots], ce[kFinalSlots];
    uint64_t my_has = ~0ull;
#pragma unroll
    for (int j = 0; j < kFinalSlots; ++j) cv[j] = ce[j] = 0u;
    if (col == nullptr) {   // uniform: the leaf lacks the column (or the column holds no value): its hits add to no bucket
      my_has = 0ull;
    } else if (multi) {     // uniform
      const NRT_GLOBAL uint32_t* const start = (const NRT_GLOBAL uint32_t*)sp->has;
#pragma unroll
      for (int j = 0; j < kFinalSlots; ++j) {
        cv[j] = start[base + lane + 64u * (uint32_t)j];
        ce[j] = start[base + lane + 64u * (uint32_t)j + 1u];
      }
    } else {
      const NRT_GLOBAL uint64_t* const has = (const NRT_GLOBAL uint64_t*)sp->has;
#pragma unroll
      for (int j = 0; j < kFinalSlots; ++j) cv[j] = col[base + lane + 64u * (uint32_t)j];
      if (has != nullptr && lane < (uint32_t)kFinalSlots) my_has = has[word0 + lane];
    }
    const bool counting = __builtin_amdgcn_readfirstlane((int)__hip_atomic_load(&st->overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == 0;

    // ---- (1) accumulate
    const uint32_t n_terms = min(part->n_terms, (uint32_t)kMaxTerms);
    const DTerm* const part_terms = terms + part->term_begin;
    uint32_t my_lo = 0, my_hi = 0;
    if (lane < n_terms) final_clause_range(part_terms + lane, tile, my_lo, my_hi);
    for (uint32_t t = 0; t < n_terms; ++t) {
      const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)my_lo, (int)t), hi = (uint32_t)__builtin_amdgcn_readlane((int)my_hi, (int)t);
      if (lo >= hi) continue;   // uniform
      final_count_clause(part_terms + t, lo, hi, base, tile_len, lane, acc);
    }

    // ---- (2) sweep
    const NRT_GLOBAL uint64_t* const live_bits = (const NRT_GLOBAL uint64_t*)part->live_bits;
    const uint32_t has_lo = (uint32_t)my_has, has_hi = (uint32_t)(my_has >> 32);
    uint32_t wave_hits = 0;
#pragma unroll
    for (int j = 0; j < kFinalSlots; ++j) {   // (unrolled: cv[j], ce[j] are registers)
      if (64u * (uint32_t)j >= tile_len) continue;   // uniform
      const uint32_t i = lane + 64u * (uint32_t)j;
      const uint64_t hw = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)has_hi, j) << 32) | (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)has_lo, j);
      bool hit = acc[i] >= need;   // (a slot beyond max_doc counted nothing)
      acc[i] = 0u;
      if (live_bits != nullptr) hit = hit && ((live_bits[word0 + (uint32_t)j] >> lane) & 1ull) != 0ull;
      const unsigned long long hits = __ballot(hit);
      wave_hits += (uint32_t)__popcll(hits);
      const unsigned long long valued = counting ? (hits & hw) : 0ull;   // uniform
      const bool mine = ((valued >> lane) & 1ull) != 0ull;
      if (multi) {   // uniform: the lane's values; its count, known here, bounds the walk
        const uint32_t n = mine ? ce[j] - cv[j] : 0u;
#pragma unroll 1
        for (uint32_t v = 0; v < n; ++v) terms_lds_add(s.table, table, shift, mask, max_buckets, st, col[cv[j] + v], 1u);
      } else if (mine) {   // the kernel's above, statement for statement (one loop for both arities cost a single-valued batch 15 %: DESIGN 4.1i)
        terms_lds_add(s.table, table, shift, mask, max_buckets, st, cv[j], 1u);
      }
    }
    final_count_slice(s, part, lane, wave_hits);
  }

  // ---- the item's table into the query's, once
  __syncthreads();
  if (__hip_atomic_load(&st->overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) {
    for (uint32_t i = tid; i < (uint32_t)kTermsLdsSlots; i += (uint32_t)kScanThreads) {
      const unsigned long long w = s.table[i];
      if (w != 0ull) terms_global_add(table, shift, mask, max_buckets, st, (uint32_t)w, (uint32_t)(w >> 32));
    }
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

// (also behind docset.hip's counting kernel)
void launch_terms_compact(hipStream_t stream, const DTermsQuery* tqueries, DTermsState* states, const unsigned long long* tables, unsigned long long* out,
                          uint32_t n_queries, uint32_t out_cap) {
  if (n_queries != 0)
    hipLaunchKernelGGL(terms_compact_kernel, dim3(n_queries), dim3(kCompactThreads), 0, stream, tqueries, states, tables, out, n_queries, out_cap);
}

void launch_bm25_terms_count(hipStream_t stream, const FinalScoreArgs& a, const DTermsQuery* tqueries, const DSortPart* sparts, DTermsState* states,
                             unsigned long long* tables, unsigned long long* out, uint32_t n_queries, uint32_t out_cap) {
  if (a.n_items != 0)
    hipLaunchKernelGGL(bm25_terms_count_kernel, dim3(a.n_items), dim3(kScanThreads), 0, stream, a.items, a.parts, a.terms, a.queries, tqueries, sparts,
                       states, tables, a.slice_sum, a.item_counts, a.item_hits);
  launch_terms_compact(stream, tqueries, states, tables, out, n_queries, out_cap);
}

void launch_bm25_terms_count_multi(hipStream_t stream, const FinalScoreArgs& a, const DTermsQuery* tqueries, const DSortPart* sparts, DTermsState* states,
                                   unsigned long long* tables, unsigned long long* out, uint32_t n_queries, uint32_t out_cap) {
  if (a.n_items != 0)
    hipLaunchKernelGGL(bm25_terms_count_multi_kernel, dim3(a.n_items), dim3(kScanThreads), 0, stream, a.items, a.parts, a.terms, a.queries, tqueries, sparts,
                       states, tables, a.slice_sum, a.item_counts, a.item_hits);
  launch_terms_compact(stream, tqueries, states, tables, out, n_queries, out_cap);
}

}  // namespace nrtgpu
