// termscount64.hip -- the gfx950 kernels of the terms aggregation over a 64-BIT column (include/nrtgpu.h:
// nrtgpu_count_terms64_batch; the reference's
// src/main/java/com/yelp/nrtsearch/server/search/collectors/additional/LongTermsCollectorManager.java:145-148 and
// DoubleTermsCollectorManager.java:147-150: countsMap.addTo(value, 1) for every collected doc).
//
//   bm25_terms_count64_kernel   bm25_terms_count_kernel (termscount.hip) over a column of 64-bit codes
//   terms_compact64_kernel      per query: the occupied slots of its global table -- and the reserved code's bucket, which lies
//                               beside the table -- packed into the call's entry list as (code, count)
//
// The first is that kernel's frame, statement for statement: the final-score skeleton (finalscore.hiph), final_count_clause into
// 4-byte slots, the hit test, the slice counts, the epilogue of an item without candidates, the one barrier of the round loop's
// lifetime in front of the flush.  Two things differ:
//   column   a lane holds the sub-tile's kFinalSlots codes as 8-byte values (fieldsort64.hip: one coalesced 8-byte load per lane
//            and 64-doc word, requested BEFORE the accumulate phase); the column is padded to whole sub-tiles: no bounds test.
//            Only a hit whose `has` bit is set reaches the add: a code never comes from a padding zero of the column
//   tables   termstables64.hiph: key words and count words in two arrays, the reserved code counted beside them.  The LDS table
//            takes 96 KiB beside the 48 KiB of the waves' counters
// All writes are vector stores and atomics in plain HIP.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "finalscore.hiph"
#include "termstables64.hiph"   // terms_lds_add64, terms_global_add64

namespace nrtgpu {

struct Terms64Smem {
  uint32_t acc[kScanWaves][kTileDocs];          // per wave: clause counts of its sub-tile
  Terms64Lds table;                             // the item's count table (plan.h), shared by the waves
  uint32_t slot_hits[kSliceSlots];              // what final_count_slice and the epilogue read (finalscore.hiph: FinalSmem)
  uint32_t slot_slice[kSliceSlots];
};
static_assert(sizeof(Terms64Smem) <= 160 * 1024, "the workgroup owns one CU's 160 KiB LDS");
static_assert(sizeof(Terms64Lds) <= 160 * 1024 - sizeof(uint32_t) * kScanWaves * kTileDocs - 1024, "the LDS table is sized to what the waves' counters leave");

__global__ __launch_bounds__(kScanThreads, kScanWaves / 4)
void bm25_terms_count64_kernel(const DItem* __restrict__ items, const DPart* __restrict__ parts, const DTerm* __restrict__ terms,
                               const DQuery* __restrict__ queries, const DTermsQuery* __restrict__ tqueries,
                               const DSort64Part* __restrict__ sparts, DTermsState64* __restrict__ states, unsigned long long* __restrict__ table_keys,
                               uint32_t* __restrict__ table_counts, uint32_t* __restrict__ slice_sum, uint32_t* __restrict__ item_counts,
                               uint64_t* __restrict__ item_hits) {
  __shared__ Terms64Smem s;
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), lane = tid & 63u;
  uint32_t* const acc = &s.acc[wave][0];
  const DItem* const item = items + blockIdx.x;
  const uint32_t query = item->query, part_begin = item->part_begin, n_parts = item->n_parts;
  const DQuery* const q = queries + query;
  const DTermsQuery* const tq = tqueries + query;
  const uint32_t need = max(tq->need, 1u), max_buckets = tq->max_buckets, shift = tq->table_shift;
  const uint32_t mask = (1u << (32u - shift)) - 1u;
  unsigned long long* const keys = table_keys + tq->table_off;
  uint32_t* const counts = table_counts + tq->table_off;
  DTermsState64* const st = states + query;

  // ---- prologue: the wave's counts, the item's table, the slice counters; a barrier
  for (int j = 0; j < kFinalSlots; ++j) acc[lane + 64u * (uint32_t)j] = 0u;
  terms_lds_clear64(s.table, tid, (uint32_t)kScanThreads);
  if (tid < (uint32_t)kSliceSlots) s.slot_hits[tid] = s.slot_slice[tid] = 0u;
  __syncthreads();

  const uint32_t total_tiles = final_total_tiles(parts, part_begin, n_parts);
  uint32_t pi = 0;      // the part of the wave's sub-tile (indices only grow)

  for (uint32_t g = wave; g < total_tiles; g += (uint32_t)kScanWaves) {
    const FinalTile tl = final_tile(parts, part_begin, n_parts, g, pi);
    const DPart* const part = tl.part;
    const uint32_t tile = tl.tile, base = tl.base, tile_len = tl.tile_len;

    // ---- (0) the sub-tile's column, requested now (fieldsort64.hip).  The column is padded to whole sub-tiles: no bounds test.
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
    } else {   // the leaf lacks the column: its hits add to no bucket
#pragma unroll
      for (int j = 0; j < kFinalSlots; ++j) cv[j] = 0ull;
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
    for (int j = 0; j < kFinalSlots; ++j) {   // (unrolled: cv[j] is a register pair)
      if (64u * (uint32_t)j >= tile_len) continue;   // uniform: the words below do not exist, the slots counted nothing
      const uint32_t i = lane + 64u * (uint32_t)j;
      const uint64_t hw = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)has_hi, j) << 32) | (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)has_lo, j);
      bool hit = acc[i] >= need;   // (a slot beyond max_doc counted nothing)
      acc[i] = 0u;
      if (live_bits != nullptr) hit = hit && ((live_bits[word0 + (uint32_t)j] >> lane) & 1ull) != 0ull;
      const unsigned long long hits = __ballot(hit);
      wave_hits += (uint32_t)__popcll(hits);
      const unsigned long long valued = counting ? (hits & hw) : 0ull;   // uniform: the word's hits that have a value
      if (((valued >> lane) & 1ull) != 0ull) terms_lds_add64(s.table, keys, counts, shift, mask, max_buckets, st, cv[j], 1u);
    }
    final_count_slice(s, part, lane, wave_hits);
  }

  // ---- the item's table into the query's, once
  __syncthreads();
  terms_lds_flush64(s.table, keys, counts, shift, mask, max_buckets, st, tid, (uint32_t)kScanThreads);

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

// One workgroup per query: the occupied slots of its table, and the reserved code's bucket where it counted, packed behind the
// other queries' in out_codes / out_counts (terms_compact_kernel's scheme: DTermsState64.out_base says where, the host sorts a
// query's entries; states[n_queries].claimed is the call's cursor).  The lists hold sum(max_buckets) entries: a query that did
// not overflow has at most max_buckets.
constexpr int kCompact64Threads = 256;
__global__ __launch_bounds__(kCompact64Threads)
void terms_compact64_kernel(const DTermsQuery* __restrict__ tqueries, DTermsState64* __restrict__ states, const unsigned long long* __restrict__ table_keys,
                            const uint32_t* __restrict__ table_counts, unsigned long long* __restrict__ out_codes, uint32_t* __restrict__ out_counts,
                            uint32_t n_queries, uint32_t out_cap) {
  __shared__ uint32_t s_n, s_base, s_pos;
  const uint32_t tid = threadIdx.x, query = blockIdx.x;
  const DTermsQuery* const tq = tqueries + query;
  DTermsState64* const st = states + query;
  const uint32_t slots = 1u << (32u - tq->table_shift);
  const unsigned long long* const keys = table_keys + tq->table_off;
  const uint32_t* const counts = table_counts + tq->table_off;
  if (tid == 0) s_n = s_pos = 0u;
  __syncthreads();
  if (st->overflow != 0u) return;   // uniform: n_out stays 0
  const uint32_t zero_count = st->zero_count;
  uint32_t mine = (tid == 0 && zero_count != 0u) ? 1u : 0u;
  for (uint32_t i = tid; i < slots; i += (uint32_t)kCompact64Threads) mine += keys[i] != 0ull ? 1u : 0u;
  if (mine != 0u) atomicAdd(&s_n, mine);
  __syncthreads();
  const uint32_t n = s_n;   // (<= max_buckets: every claim was counted, and the claim that passed the bound raised the flag)
  if (tid == 0) s_base = atomicAdd(&states[n_queries].claimed, n);
  __syncthreads();
  const uint32_t base = s_base;
  if (tid == 0 && zero_count != 0u) {
    const uint32_t at = base + atomicAdd(&s_pos, 1u);
    if (at < out_cap) {   // (always true)
      out_codes[at] = 0ull;
      out_counts[at] = zero_count;
    }
  }
  for (uint32_t i = tid; i < slots; i += (uint32_t)kCompact64Threads) {
    const unsigned long long k = keys[i];
    if (k == 0ull) continue;
    const uint32_t at = base + atomicAdd(&s_pos, 1u);
    if (at < out_cap) {   // (always true)
      out_codes[at] = k;
      out_counts[at] = counts[i];
    }
  }
  if (tid == 0) {
    st->n_out = n;
    st->out_base = base;
  }
}

// (also behind docset.hip's counting kernels)
void launch_terms_compact64(hipStream_t stream, const DTermsQuery* tqueries, DTermsState64* states, const unsigned long long* table_keys,
                            const uint32_t* table_counts, unsigned long long* out_codes, uint32_t* out_counts, uint32_t n_queries, uint32_t out_cap) {
  if (n_queries != 0)
    hipLaunchKernelGGL(terms_compact64_kernel, dim3(n_queries), dim3(kCompact64Threads), 0, stream, tqueries, states, table_keys, table_counts, out_codes,
                       out_counts, n_queries, out_cap);
}

void launch_bm25_terms_count64(hipStream_t stream, const FinalScoreArgs& a, const DTermsQuery* tqueries, const DSort64Part* sparts, DTermsState64* states,
                               unsigned long long* table_keys, uint32_t* table_counts, unsigned long long* out_codes, uint32_t* out_counts,
                               uint32_t n_queries, uint32_t out_cap) {
  if (a.n_items != 0)
    hipLaunchKernelGGL(bm25_terms_count64_kernel, dim3(a.n_items), dim3(kScanThreads), 0, stream, a.items, a.parts, a.terms, a.queries, tqueries, sparts,
                       states, table_keys, table_counts, a.slice_sum, a.item_counts, a.item_hits);
  launch_terms_compact64(stream, tqueries, states, table_keys, table_counts, out_codes, out_counts, n_queries, out_cap);
}

}  // namespace nrtgpu
