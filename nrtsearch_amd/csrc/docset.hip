// docset.hip -- the gfx950 kernels of the doc-set requests (include/nrtgpu.h: nrtgpu_search_docset_sorted_batch,
// nrtgpu_count_docset_terms_batch): a sort by field or a terms count whose hit set is a DOC SET -- liveDocs, FILTER / MUST_NOT
// masks, numeric range clauses (the reference's MatchAllDocsQuery, a BooleanQuery of FILTER clauses only, IntFieldDef /
// FloatFieldDef.getRangeQuery) -- and no text clause.
//
//   docset_sort_kernel          per sub-tile the accept words, the range clauses, then keys for the accepted docs and the item's top-k
//   docset_terms_count_kernel   the same hit set; every hit with a value adds 1 in the count table under the value's code
//   docset_sort_multi_kernel, docset_terms_count_multi_kernel   the two for calls that name a MULTI-VALUED column (at the end)
//   docset_sort64_kernel<MULTI> docset_sort_kernel / docset_sort_multi_kernel over a 64-BIT sort column (plan.h: sort_key64; behind them)
//   docset_range_count_kernel<WIDE, MULTI>   the same hit set; every hit with a value adds 1 to the elementary interval of its
//                               code among the query's cut points (nrtgpu_count_docset_ranges_batch; behind the 64-bit sort)
//   docset_terms_count64_kernel<MULTI>   docset_terms_count_kernel over a 64-BIT count column (termstables64.hiph;
//                               nrtgpu_count_docset_terms64_batch; behind the range facet)
//
// The decomposition is the final-score skeleton's (finalscore.hiph): one workgroup of kScanWaves waves per item, a wave takes
// kTileDocs-doc sub-tiles of the item's parts (final_total_tiles / final_tile), hits per slice through final_count_slice, the
// sorted kernel's candidates through the shared buffer with the wave-by-wave compaction, theta_g and final_epilogue; the count
// kernel's tables are termstables.hiph's and terms_compact_kernel (termscount.hip) packs them.  What the route does NOT have:
// postings, clause counters in LDS (the 96 KiB of the text kernels), an atomic per doc.  The hit set IS the accept words:
//   accept words  lane j loads word j of the sub-tile's 16 (DPart.live_bits: the query's combined accept set WITH liveDocs;
//                 nullptr: every doc), cut at max_doc.  A sub-tile without an accepted doc ends there.
//   lane's view   bit j of a lane's 16-bit mask is doc base + lane + 64 j (the words transposed by readlane).  A range clause
//                 narrows it: the lane's codes and `has` bits of the clause's column on the part's leaf, range_accepts_code.  Only
//                 the 64-doc words that still hold an accepted doc are loaded, and a clause is evaluated only while some doc of the
//                 sub-tile is accepted.  Columns are padded to whole sub-tiles: no bounds test.
//   hits          the wave sum of the masks' popcounts: total_hits reads no column but the range clauses'.
// A candidate key waits in a REGISTER for the round's meeting (16 keys per lane) where the text kernels leave it in the
// accumulator's slot.  All writes are vector stores and atomics in plain HIP; every loop is bounded by a count known on entry.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "finalscore.hiph"
#include "termstables.hiph"
#include "termstables64.hiph"

namespace nrtgpu {

static_assert(kFinalSlots <= 16 && kMaxRanges <= 8, "a lane's view of a sub-tile is a 16-bit mask");

// The lane's bit of each of the sub-tile's words: lane j (< kFinalSlots) holds word j as (lo, hi); bit j of the result is bit
// `lane` of word j, i.e. doc base + lane + 64 j.  All lanes of the wave call.
__device__ __forceinline__ uint32_t docset_lane_bits(uint32_t w_lo, uint32_t w_hi, uint32_t lane) {
  const uint32_t sh = lane & 31u;
  const bool low = lane < 32u;
  uint32_t m = 0;
#pragma unroll
  for (int j = 0; j < kFinalSlots; ++j) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)w_lo, j), hi = (uint32_t)__builtin_amdgcn_readlane((int)w_hi, j);
    m |= (((low ? lo : hi) >> sh) & 1u) << j;
  }
  return m;
}

// The sub-tile's accept words as the lane's view; words (uniform): bit j = word j holds an accepted doc.
__device__ __forceinline__ uint32_t docset_accept(const DPart* part, uint32_t word0, uint32_t tile_len, uint32_t lane, uint32_t& words) {
  const NRT_GLOBAL uint64_t* const live_bits = (const NRT_GLOBAL uint64_t*)part->live_bits;
  uint64_t w = 0ull;
  const uint32_t first = 64u * lane;   // the first doc of the lane's word inside the sub-tile
  if (lane < (uint32_t)kFinalSlots && first < tile_len) {
    w = live_bits != nullptr ? live_bits[word0 + lane] : ~0ull;
    const uint32_t n = tile_len - first;   // the word's docs below max_doc: the tail word admits nothing at or beyond it
    if (n < 64u) w &= (1ull << n) - 1ull;
  }
  words = (uint32_t)__ballot(w != 0ull) & ((1u << kFinalSlots) - 1u);
  if (words == 0u) return 0u;   // uniform
  return docset_lane_bits((uint32_t)w, (uint32_t)(w >> 32), lane);
}

// What is left of the lane's view: which words still hold an accepted doc, and the wave's accepted docs (both uniform).
__device__ __forceinline__ void docset_census(uint32_t m, uint32_t& words, uint32_t& hits) {
  words = 0u;
  hits = 0u;
#pragma unroll
  for (int j = 0; j < kFinalSlots; ++j) {
    const unsigned long long b = __ballot(((m >> j) & 1u) != 0u);
    words |= (b != 0ull ? 1u : 0u) << j;
    hits += (uint32_t)__popcll(b);
  }
}

// A column over the sub-tile: the lane's codes of the words in `words` (the others read 0 and are never looked at) and the
// lane's `has` bits; false: the leaf lacks the column.
__device__ __forceinline__ bool docset_column(const DSortPart* sp, uint32_t base, uint32_t word0, uint32_t lane, uint32_t words,
                                              uint32_t (&cv)[kFinalSlots], uint32_t& has_bits) {
  const NRT_GLOBAL uint32_t* const col = (const NRT_GLOBAL uint32_t*)sp->code;
  const NRT_GLOBAL uint64_t* const has = (const NRT_GLOBAL uint64_t*)sp->has;
  if (col == nullptr) {   // uniform
#pragma unroll
    for (int j = 0; j < kFinalSlots; ++j) cv[j] = 0u;
    has_bits = 0u;
    return false;
  }
  uint64_t hw = 0ull;
  if (has != nullptr && lane < (uint32_t)kFinalSlots) hw = has[word0 + lane];
#pragma unroll
  for (int j = 0; j < kFinalSlots; ++j) {
    cv[j] = 0u;
    if (((words >> j) & 1u) != 0u) cv[j] = col[base + lane + 64u * (uint32_t)j];   // uniform: a word without an accepted doc costs no load
  }
  has_bits = has != nullptr ? docset_lane_bits((uint32_t)hw, (uint32_t)(hw >> 32), lane) : (1u << kFinalSlots) - 1u;
  return true;
}

// The sub-tile's hit set as the lane's view: the accept words narrowed by every range clause of the query in turn.  rparts: the
// part's kMaxRanges column records.  words / hits: docset_census of the result.
__device__ __forceinline__ uint32_t docset_hit_set(const DPart* part, const DRangeQuery* rq, const DSortPart* rparts, uint32_t base, uint32_t tile_len,
                                                   uint32_t lane, uint32_t& words, uint32_t& hits) {
  const uint32_t word0 = base >> 6;
  hits = 0u;
  uint32_t m = docset_accept(part, word0, tile_len, lane, words);
  if (words == 0u) return 0u;   // uniform
  const uint32_t n_ranges = min(rq->n_ranges, (uint32_t)kMaxRanges);
#pragma unroll 1
  for (uint32_t r = 0; r < n_ranges; ++r) {
    uint32_t cv[kFinalSlots], has_bits;
    if (!docset_column(rparts + r, base, word0, lane, words, cv, has_bits)) {   // no doc of the leaf has a value: none passes
      words = hits = 0u;
      return 0u;
    }
    const uint32_t lo = rq->lo_code[r], hi = rq->hi_code[r];
    uint32_t pass = 0u;
#pragma unroll
    for (int j = 0; j < kFinalSlots; ++j) pass |= (range_accepts_code(lo, hi, cv[j]) ? 1u : 0u) << j;
    m &= has_bits & pass;
    docset_census(m, words, hits);
    if (words == 0u) return 0u;   // uniform: the later clauses load nothing
  }
  if (n_ranges == 0u) docset_census(m, words, hits);
  return m;
}

// The wave's candidate keys (registers; 0: none) into cand[pos ...], slot-major -- final_push_candidates for keys that never
// lay in LDS.
template <class S>
__device__ __forceinline__ void docset_push_candidates(S& s, const uint64_t (&key)[kFinalSlots], uint32_t lane, uint32_t pos) {
#pragma unroll
  for (int j = 0; j < kFinalSlots; ++j) {
    const unsigned long long b = __ballot(key[j] != 0ull);
    if (key[j] != 0ull) {
      const uint32_t at = pos + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
      if (at < (uint32_t)S::kCandCap) s.cand[at] = key[j];   // (always true: the caller made room)
    }
    pos += (uint32_t)__popcll(b);
  }
}

typedef FinalSmem<kScanWaves, kFsCandCap> DocsetSortSmem;   // (its `cache` is carried but neither written nor read: no score is computed)

__global__ __launch_bounds__(kScanThreads, kScanWaves / 4)
void docset_sort_kernel(const DItem* __restrict__ items, const DPart* __restrict__ parts, const DQuery* __restrict__ queries,
                        const DSortQuery* __restrict__ squeries, const DRangeQuery* __restrict__ rqueries, const DSortPart* __restrict__ sparts,
                        const DSortPart* __restrict__ rparts, unsigned long long* __restrict__ theta_g, uint32_t* __restrict__ slice_sum,
                        uint64_t* __restrict__ item_keys, uint32_t* __restrict__ item_counts, uint64_t* __restrict__ item_hits, uint32_t k_stride) {
  __shared__ DocsetSortSmem s;
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), lane = tid & 63u;
  const DItem* const item = items + blockIdx.x;
  const uint32_t query = item->query, part_begin = item->part_begin, n_parts = item->n_parts;
  const DQuery* const q = queries + query;
  const uint32_t k = min(q->k, (uint32_t)kMaxK);
  const DSortQuery* const sq = squeries + query;
  const DRangeQuery* const rq = rqueries + query;
  const uint32_t reverse = sq->reverse, missing_code = sq->missing_code;
  const bool has_after = sq->has_after != 0u;
  const uint64_t after_key = sq->after_key;
  const bool multi_item = q->n_items > 1;
  unsigned long long* const my_theta_g = theta_g + query;

  if (tid < (uint32_t)kSliceSlots) s.slot_hits[tid] = s.slot_slice[tid] = 0u;
  __syncthreads();

  const uint32_t total_tiles = final_total_tiles(parts, part_begin, n_parts);
  uint64_t theta = 0;   // uniform: the k-th best key known (this item's compactions, the query's other items)
  uint32_t cnt = 0;     // uniform: keys in s.cand
  uint32_t pi = 0;      // the part of the wave's sub-tile (indices only grow)
  uint32_t par = 0;

  for (uint32_t g0 = 0; g0 < total_tiles; g0 += (uint32_t)kScanWaves, par ^= 1u) {
    if (multi_item) {   // what the query's other items have published (at least k docs of the query exceed it)
      const uint64_t t = __hip_atomic_load(my_theta_g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      theta = t > theta ? t : theta;
    }
    const uint32_t g = g0 + wave;
    uint32_t n_cand = 0;   // wave-uniform
    uint64_t key[kFinalSlots];
#pragma unroll
    for (int j = 0; j < kFinalSlots; ++j) key[j] = 0ull;
    if (g < total_tiles) {
      const FinalTile tl = final_tile(parts, part_begin, n_parts, g, pi);
      const uint32_t base = tl.base, gdoc0 = tl.gdoc0;
      uint32_t words, hits;
      const uint32_t m = docset_hit_set(tl.part, rq, rparts + (size_t)(part_begin + pi) * (size_t)kMaxRanges, base, tl.tile_len, lane, words, hits);
      if (words != 0u) {   // uniform
        uint32_t cv[kFinalSlots], has_bits;
        docset_column(sparts + part_begin + pi, base, base >> 6, lane, words, cv, has_bits);   // (a leaf without the column: every doc sorts as the missing value)
#pragma unroll
        for (int j = 0; j < kFinalSlots; ++j) {
          if (((m >> j) & 1u) != 0u) {
            const uint32_t code = ((has_bits >> j) & 1u) != 0u ? cv[j] : missing_code;
            const uint64_t doc_key = sort_key(reverse, code, gdoc0 + lane + 64u * (uint32_t)j);
            if (doc_key > theta && (!has_after || doc_key < after_key)) key[j] = doc_key;   // (hits of earlier pages still count: `hits`)
          }
          n_cand += (uint32_t)__popcll(__ballot(key[j] != 0ull));
        }
        final_count_slice(s, tl.part, lane, hits);
      }
    }
    if (lane == 0) s.wcount[par][wave] = n_cand;
    __syncthreads();

    // ---- the round's candidates into the shared buffer (fieldsort.hip's meeting, the keys read from registers)
    uint32_t tot = 0, before = 0;
#pragma unroll
    for (uint32_t w2 = 0; w2 < (uint32_t)kScanWaves; ++w2) {
      const uint32_t c = s.wcount[par][w2];
      tot += c;
      before += w2 < wave ? c : 0u;
    }
    if (cnt + tot <= (uint32_t)kFsCandCap) {   // uniform
      docset_push_candidates(s, key, lane, cnt + before);
      cnt += tot;
    } else {
      for (uint32_t w2 = 0; w2 < (uint32_t)kScanWaves; ++w2) {
        const uint32_t c = s.wcount[par][w2];
        if (cnt + c > (uint32_t)kFsCandCap) {   // uniform; cnt > k here (kFsCandCap >= kMaxK + kTileDocs)
          __syncthreads();   // the keys appended so far are in place
          uint64_t thr = 0;
          cnt = topk_compact<kScanThreads, kFsCandCap>(s.cand, cnt, k, &s.sc, &thr);
          if (thr > theta) theta = thr;
          if (tid == 0) atomicMax(my_theta_g, (unsigned long long)thr);   // LazyMaxScoreAccumulator.accumulate analogue
        }
        if (wave == w2) docset_push_candidates(s, key, lane, cnt);
        cnt += c;
      }
    }
  }

  final_epilogue(s, cnt, k, q, tid, slice_sum, item_keys, item_counts, item_hits, k_stride);
}

struct DocsetTermsSmem {
  unsigned long long table[kTermsLdsSlots];     // the item's count table (plan.h), shared by the waves
  uint32_t slot_hits[kSliceSlots];              // what final_count_slice and the epilogue read (finalscore.hiph: FinalSmem)
  uint32_t slot_slice[kSliceSlots];
};

__global__ __launch_bounds__(kScanThreads, kScanWaves / 4)
void docset_terms_count_kernel(const DItem* __restrict__ items, const DPart* __restrict__ parts, const DQuery* __restrict__ queries,
                               const DTermsQuery* __restrict__ tqueries, const DRangeQuery* __restrict__ rqueries,
                               const DSortPart* __restrict__ sparts, const DSortPart* __restrict__ rparts, DTermsState* __restrict__ states,
                               unsigned long long* __restrict__ tables, uint32_t* __restrict__ slice_sum, uint32_t* __restrict__ item_counts,
                               uint64_t* __restrict__ item_hits) {
  __shared__ DocsetTermsSmem s;
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), lane = tid & 63u;
  const DItem* const item = items + blockIdx.x;
  const uint32_t query = item->query, part_begin = item->part_begin, n_parts = item->n_parts;
  const DQuery* const q = queries + query;
  const DTermsQuery* const tq = tqueries + query;
  const DRangeQuery* const rq = rqueries + query;
  const uint32_t max_buckets = tq->max_buckets, shift = tq->table_shift;
  const uint32_t mask = (1u << (32u - shift)) - 1u;
  unsigned long long* const table = tables + tq->table_off;
  DTermsState* const st = states + query;

  for (uint32_t i = tid; i < (uint32_t)kTermsLdsSlots; i += (uint32_t)kScanThreads) s.table[i] = 0ull;
  if (tid < (uint32_t)kSliceSlots) s.slot_hits[tid] = s.slot_slice[tid] = 0u;
  __syncthreads();

  const uint32_t total_tiles = final_total_tiles(parts, part_begin, n_parts);
  uint32_t pi = 0;      // the part of the wave's sub-tile (indices only grow)

  for (uint32_t g = wave; g < total_tiles; g += (uint32_t)kScanWaves) {
    const FinalTile tl = final_tile(parts, part_begin, n_parts, g, pi);
    const uint32_t base = tl.base;
    uint32_t words, hits;
    const uint32_t m = docset_hit_set(tl.part, rq, rparts + (size_t)(part_begin + pi) * (size_t)kMaxRanges, base, tl.tile_len, lane, words, hits);
    if (words == 0u) continue;   // uniform
    final_count_slice(s, tl.part, lane, hits);
    // an overflowed query's buckets are void: its items go on counting hits only (a flag read once, not waited for)
    if (__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(&st->overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != 0) continue;
    uint32_t cv[kFinalSlots], has_bits;
    if (!docset_column(sparts + part_begin + pi, base, base >> 6, lane, words, cv, has_bits)) continue;   // the leaf lacks the column: its hits add to no bucket
    const uint32_t valued = m & has_bits;
#pragma unroll
    for (int j = 0; j < kFinalSlots; ++j)
      if (((valued >> j) & 1u) != 0u) terms_lds_add(s.table, table, shift, mask, max_buckets, st, cv[j], 1u);
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
    uint32_t n = 0;
    const uint32_t gte_floor = q->gte_floor, slice_base = q->slice_base;
    for (int i = 0; i < kSliceSlots; ++i) {
      const uint32_t h = s.slot_hits[i];
      n += h;
      if (h != 0u && gte_floor != 0xFFFFFFFFu) atomicAdd(&slice_sum[slice_base + s.slot_slice[i]], h);
    }
    item_hits[blockIdx.x] = n;
  }
}

// ---- calls that name a MULTI-VALUED column (plan.h: DSortPart: codes[] behind start[]) ------------------------------------------
// The two kernels above for calls in which a range clause's column or the count column is multi-valued.  The arity is a wave-
// uniform flag -- per clause (DRangeQuery.multi), per query for the count column (DTermsQuery.need bit 31) -- so a batch that mixes
// arities is one launch, and a single-valued column goes through the functions above.  The reference's rules: a range clause
// keeps a doc iff ANY of its values lies in the range (SortedNumericDocValuesField.newSlowRangeQuery); every value instance of a
// hit adds 1 (IntTermsCollectorManager.java:142-152).  The kernels above keep their text: what follows repeats their frames.

// A lane's start[d] and start[d + 1] for the words in `words` (the others read 0: no value).  start[] is padded to whole
// sub-tiles plus one: no bounds test.
__device__ __forceinline__ void docset_value_spans(const DSortPart* sp, uint32_t base, uint32_t lane, uint32_t words, uint32_t (&s0)[kFinalSlots],
                                                   uint32_t (&s1)[kFinalSlots]) {
  const NRT_GLOBAL uint32_t* const start = (const NRT_GLOBAL uint32_t*)sp->has;
#pragma unroll
  for (int j = 0; j < kFinalSlots; ++j) {
    s0[j] = s1[j] = 0u;
    if (((words >> j) & 1u) != 0u) {   // uniform: a word without an accepted doc costs no load
      s0[j] = start[base + lane + 64u * (uint32_t)j];
      s1[j] = start[base + lane + 64u * (uint32_t)j + 1u];
    }
  }
}

// A multi-valued range clause over the lane's view m: the docs of m with SOME value in [lo, hi].  A lane walks the values of its
// accepted docs only and stops at the first that passes; the walk's bound is the doc's count, read on entry.
__device__ __forceinline__ uint32_t docset_range_any(const DSortPart* sp, uint32_t base, uint32_t lane, uint32_t words, uint32_t m, uint32_t lo, uint32_t hi) {
  const NRT_GLOBAL uint32_t* const codes = (const NRT_GLOBAL uint32_t*)sp->code;
  uint32_t s0[kFinalSlots], s1[kFinalSlots];
  docset_value_spans(sp, base, lane, words, s0, s1);
  uint32_t pass = 0u;
#pragma unroll
  for (int j = 0; j < kFinalSlots; ++j) {
    const uint32_t n = ((m >> j) & 1u) != 0u ? s1[j] - s0[j] : 0u;
    bool any = false;
#pragma unroll 1
    for (uint32_t v = 0; v < n && !any; ++v) any = range_accepts_code(lo, hi, codes[s0[j] + v]);
    pass |= (any ? 1u : 0u) << j;
  }
  return pass;
}

// docset_hit_set with the clause's arity read from rq->multi.
__device__ __forceinline__ uint32_t docset_hit_set_multi(const DPart* part, const DRangeQuery* rq, const DSortPart* rparts, uint32_t base, uint32_t tile_len,
                                                         uint32_t lane, uint32_t& words, uint32_t& hits) {
  const uint32_t word0 = base >> 6;
  hits = 0u;
  uint32_t m = docset_accept(part, word0, tile_len, lane, words);
  if (words == 0u) return 0u;   // uniform
  const uint32_t n_ranges = min(rq->n_ranges, (uint32_t)kMaxRanges), multi = rq->multi;
#pragma unroll 1
  for (uint32_t r = 0; r < n_ranges; ++r) {
    const uint32_t lo = rq->lo_code[r], hi = rq->hi_code[r];
    if (rparts[r].code == nullptr) {   // uniform: no doc of the leaf has a value: none passes
      words = hits = 0u;
      return 0u;
    }
    if (((multi >> r) & 1u) != 0u) {   // uniform
      m &= docset_range_any(rparts + r, base, lane, words, m, lo, hi);
    } else {
      uint32_t cv[kFinalSlots], has_bits;
      docset_column(rparts + r, base, word0, lane, words, cv, has_bits);
      uint32_t pass = 0u;
#pragma unroll
      for (int j = 0; j < kFinalSlots; ++j) pass |= (range_accepts_code(lo, hi, cv[j]) ? 1u : 0u) << j;
      m &= has_bits & pass;
    }
    docset_census(m, words, hits);
    if (words == 0u) return 0u;   // uniform: the later clauses load nothing
  }
  if (n_ranges == 0u) docset_census(m, words, hits);
  return m;
}

// docset_sort_kernel over docset_hit_set_multi (the sort's own column is single-valued: a sort names one value per doc).
__global__ __launch_bounds__(kScanThreads, kScanWaves / 4)
void docset_sort_multi_kernel(const DItem* __restrict__ items, const DPart* __restrict__ parts, const DQuery* __restrict__ queries,
                              const DSortQuery* __restrict__ squeries, const DRangeQuery* __restrict__ rqueries, const DSortPart* __restrict__ sparts,
                              const DSortPart* __restrict__ rparts, unsigned long long* __restrict__ theta_g, uint32_t* __restrict__ slice_sum,
                              uint64_t* __restrict__ item_keys, uint32_t* __restrict__ item_counts, uint64_t* __restrict__ item_hits, uint32_t k_stride) {
  __shared__ DocsetSortSmem s;
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), lane = tid & 63u;
  const DItem* const item = items + blockIdx.x;
  const uint32_t query = item->query, part_begin = item->part_begin, n_parts = item->n_parts;
  const DQuery* const q = queries + query;
  const uint32_t k = min(q->k, (uint32_t)kMaxK);
  const DSortQuery* const sq = squeries + query;
  const DRangeQuery* const rq = rqueries + query;
  const uint32_t reverse = sq->reverse, missing_code = sq->missing_code;
  const bool has_after = sq->has_after != 0u;
  const uint64_t after_key = sq->after_key;
  const bool multi_item = q->n_items > 1;
  unsigned long long* const my_theta_g = theta_g + query;

  if (tid < (uint32_t)kSliceSlots) s.slot_hits[tid] = s.slot_slice[tid] = 0u;
  __syncthreads();

  const uint32_t total_tiles = final_total_tiles(parts, part_begin, n_parts);
  uint64_t theta = 0;   // uniform: the k-th best key known (this item's compactions, the query's other items)
  uint32_t cnt = 0;     // uniform: keys in s.cand
  uint32_t pi = 0;      // the part of the wave's sub-tile (indices only grow)
  uint32_t par = 0;

  for (uint32_t g0 = 0; g0 < total_tiles; g0 += (uint32_t)kScanWaves, par ^= 1u) {
    if (multi_item) {
      const uint64_t t = __hip_atomic_load(my_theta_g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      theta = t > theta ? t : theta;
    }
    const uint32_t g = g0 + wave;
    uint32_t n_cand = 0;   // wave-uniform
    uint64_t key[kFinalSlots];
#pragma unroll
    for (int j = 0; j < kFinalSlots; ++j) key[j] = 0ull;
    if (g < total_tiles) {
      const FinalTile tl = final_tile(parts, part_begin, n_parts, g, pi);
      const uint32_t base = tl.base, gdoc0 = tl.gdoc0;
      uint32_t words, hits;
      const uint32_t m = docset_hit_set_multi(tl.part, rq, rparts + (size_t)(part_begin + pi) * (size_t)kMaxRanges, base, tl.tile_len, lane, words, hits);
      if (words != 0u) {   // uniform
        uint32_t cv[kFinalSlots], has_bits;
        docset_column(sparts + part_begin + pi, base, base >> 6, lane, words, cv, has_bits);
#pragma unroll
        for (int j = 0; j < kFinalSlots; ++j) {
          if (((m >> j) & 1u) != 0u) {
            const uint32_t code = ((has_bits >> j) & 1u) != 0u ? cv[j] : missing_code;
            const uint64_t doc_key = sort_key(reverse, code, gdoc0 + lane + 64u * (uint32_t)j);
            if (doc_key > theta && (!has_after || doc_key < after_key)) key[j] = doc_key;
          }
          n_cand += (uint32_t)__popcll(__ballot(key[j] != 0ull));
        }
        final_count_slice(s, tl.part, lane, hits);
      }
    }
    if (lane == 0) s.wcount[par][wave] = n_cand;
    __syncthreads();

    // ---- the round's candidates into the shared buffer (docset_sort_kernel's meeting)
    uint32_t tot = 0, before = 0;
#pragma unroll
    for (uint32_t w2 = 0; w2 < (uint32_t)kScanWaves; ++w2) {
      const uint32_t c = s.wcount[par][w2];
      tot += c;
      before += w2 < wave ? c : 0u;
    }
    if (cnt + tot <= (uint32_t)kFsCandCap) {   // uniform
      docset_push_candidates(s, key, lane, cnt + before);
      cnt += tot;
    } else {
      for (uint32_t w2 = 0; w2 < (uint32_t)kScanWaves; ++w2) {
        const uint32_t c = s.wcount[par][w2];
        if (cnt + c > (uint32_t)kFsCandCap) {   // uniform; cnt > k here (kFsCandCap >= kMaxK + kTileDocs)
          __syncthreads();   // the keys appended so far are in place
          uint64_t thr = 0;
          cnt = topk_compact<kScanThreads, kFsCandCap>(s.cand, cnt, k, &s.sc, &thr);
          if (thr > theta) theta = thr;
          if (tid == 0) atomicMax(my_theta_g, (unsigned long long)thr);
        }
        if (wave == w2) docset_push_candidates(s, key, lane, cnt);
        cnt += c;
      }
    }
  }

  final_epilogue(s, cnt, k, q, tid, slice_sum, item_keys, item_counts, item_hits, k_stride);
}

// docset_terms_count_kernel over docset_hit_set_multi, with the count column's arity read from the query's record: every value
// of a hit adds 1, each hit lane walking its own codes[start[d] .. start[d + 1]).
__global__ __launch_bounds__(kScanThreads, kScanWaves / 4)
void docset_terms_count_multi_kernel(const DItem* __restrict__ items, const DPart* __restrict__ parts, const DQuery* __restrict__ queries,
                                     const DTermsQuery* __restrict__ tqueries, const DRangeQuery* __restrict__ rqueries,
                                     const DSortPart* __restrict__ sparts, const DSortPart* __restrict__ rparts, DTermsState* __restrict__ states,
                                     unsigned long long* __restrict__ tables, uint32_t* __restrict__ slice_sum, uint32_t* __restrict__ item_counts,
                                     uint64_t* __restrict__ item_hits) {
  __shared__ DocsetTermsSmem s;
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), lane = tid & 63u;
  const DItem* const item = items + blockIdx.x;
  const uint32_t query = item->query, part_begin = item->part_begin, n_parts = item->n_parts;
  const DQuery* const q = queries + query;
  const DTermsQuery* const tq = tqueries + query;
  const DRangeQuery* const rq = rqueries + query;
  const uint32_t max_buckets = tq->max_buckets, shift = tq->table_shift;
  const bool multi = (tq->need & kTermsQueryMulti) != 0u;   // uniform: the query's count column is multi-valued
  const uint32_t mask = (1u << (32u - shift)) - 1u;
  unsigned long long* const table = tables + tq->table_off;
  DTermsState* const st = states + query;

  for (uint32_t i = tid; i < (uint32_t)kTermsLdsSlots; i += (uint32_t)kScanThreads) s.table[i] = 0ull;
  if (tid < (uint32_t)kSliceSlots) s.slot_hits[tid] = s.slot_slice[tid] = 0u;
  __syncthreads();

  const uint32_t total_tiles = final_total_tiles(parts, part_begin, n_parts);
  uint32_t pi = 0;      // the part of the wave's sub-tile (indices only grow)

  for (uint32_t g = wave; g < total_tiles; g += (uint32_t)kScanWaves) {
    const FinalTile tl = final_tile(parts, part_begin, n_parts, g, pi);
    const uint32_t base = tl.base;
    uint32_t words, hits;
    const uint32_t m = docset_hit_set_multi(tl.part, rq, rparts + (size_t)(part_begin + pi) * (size_t)kMaxRanges, base, tl.tile_len, lane, words, hits);
    if (words == 0u) continue;   // uniform
    final_count_slice(s, tl.part, lane, hits);
    if (__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(&st->overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != 0) continue;
    const DSortPart* const sp = sparts + part_begin + pi;
    if (multi) {   // uniform
      const NRT_GLOBAL uint32_t* const codes = (const NRT_GLOBAL uint32_t*)sp->code;
      if (codes == nullptr) continue;   // uniform: the leaf lacks the column (or the column holds no value)
      uint32_t s0[kFinalSlots], s1[kFinalSlots];
      docset_value_spans(sp, base, lane, words, s0, s1);
#pragma unroll
      for (int j = 0; j < kFinalSlots; ++j) {
        const uint32_t n = ((m >> j) & 1u) != 0u ? s1[j] - s0[j] : 0u;   // the lane's count bounds its walk
#pragma unroll 1
        for (uint32_t v = 0; v < n; ++v) terms_lds_add(s.table, table, shift, mask, max_buckets, st, codes[s0[j] + v], 1u);
      }
    } else {
      uint32_t cv[kFinalSlots], has_bits;
      if (!docset_column(sp, base, base >> 6, lane, words, cv, has_bits)) continue;
      const uint32_t valued = m & has_bits;
#pragma unroll
      for (int j = 0; j < kFinalSlots; ++j)
        if (((valued >> j) & 1u) != 0u) terms_lds_add(s.table, table, shift, mask, max_buckets, st, cv[j], 1u);
    }
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
    uint32_t n = 0;
    const uint32_t gte_floor = q->gte_floor, slice_base = q->slice_base;
    for (int i = 0; i < kSliceSlots; ++i) {
      const uint32_t h = s.slot_hits[i];
      n += h;
      if (h != 0u && gte_floor != 0xFFFFFFFFu) atomicAdd(&slice_sum[slice_base + s.slot_slice[i]], h);
    }
    item_hits[blockIdx.x] = n;
  }
}

// ---- a sort by a 64-BIT column (plan.h: DSort64Query / DSort64Part, sort_key64; nrtgpu_search_docset_sorted64_batch) --------------
// docset_column over a column of 64-bit codes: the lane's 8-byte codes of the words in `words` and its `has` bits.
__device__ __forceinline__ bool docset_column64(const DSort64Part* sp, uint32_t base, uint32_t word0, uint32_t lane, uint32_t words,
                                                uint64_t (&cv)[kFinalSlots], uint32_t& has_bits) {
  const NRT_GLOBAL uint64_t* const col = (const NRT_GLOBAL uint64_t*)sp->code64;
  const NRT_GLOBAL uint64_t* const has = (const NRT_GLOBAL uint64_t*)sp->has;
  if (col == nullptr) {   // uniform
#pragma unroll
    for (int j = 0; j < kFinalSlots; ++j) cv[j] = 0ull;
    has_bits = 0u;
    return false;
  }
  uint64_t hw = 0ull;
  if (has != nullptr && lane < (uint32_t)kFinalSlots) hw = has[word0 + lane];
#pragma unroll
  for (int j = 0; j < kFinalSlots; ++j) {
    cv[j] = 0ull;
    if (((words >> j) & 1u) != 0u) cv[j] = col[base + lane + 64u * (uint32_t)j];   // uniform: a word without an accepted doc costs no load
  }
  has_bits = has != nullptr ? docset_lane_bits((uint32_t)hw, (uint32_t)(hw >> 32), lane) : (1u << kFinalSlots) - 1u;
  return true;
}

// docset_sort_kernel (MULTI: docset_sort_multi_kernel -- the doc set's 32-bit range clauses may name multi-valued columns) with
// the sort's column read as 64-bit codes, the packed key and the cursor test on (code, doc).  Everything else is that kernel's.
template <bool MULTI>
__global__ __launch_bounds__(kScanThreads, kScanWaves / 4)
void docset_sort64_kernel(const DItem* __restrict__ items, const DPart* __restrict__ parts, const DQuery* __restrict__ queries,
                          const DSort64Query* __restrict__ squeries, const DRangeQuery* __restrict__ rqueries, const DSort64Part* __restrict__ sparts,
                          const DSortPart* __restrict__ rparts, unsigned long long* __restrict__ theta_g, uint32_t* __restrict__ slice_sum,
                          uint64_t* __restrict__ item_keys, uint32_t* __restrict__ item_counts, uint64_t* __restrict__ item_hits, uint32_t k_stride) {
  __shared__ DocsetSortSmem s;
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), lane = tid & 63u;
  const DItem* const item = items + blockIdx.x;
  const uint32_t query = item->query, part_begin = item->part_begin, n_parts = item->n_parts;
  const DQuery* const q = queries + query;
  const uint32_t k = min(q->k, (uint32_t)kMaxK);
  const DSort64Query* const sq = squeries + query;
  const DRangeQuery* const rq = rqueries + query;
  const uint64_t lo = sq->lo, span = sq->span, missing_code = sq->missing_code, after_code = sq->after_code;
  const uint32_t reverse = sq->reverse, after_doc = sq->after_doc;
  const uint32_t db = min(max(sq->db, 1u), 31u);
  const bool has_after = sq->has_after != 0u;
  const bool multi_item = q->n_items > 1;
  unsigned long long* const my_theta_g = theta_g + query;

  if (tid < (uint32_t)kSliceSlots) s.slot_hits[tid] = s.slot_slice[tid] = 0u;
  __syncthreads();

  const uint32_t total_tiles = final_total_tiles(parts, part_begin, n_parts);
  uint64_t theta = 0;   // uniform: the k-th best key known (this item's compactions, the query's other items)
  uint32_t cnt = 0;     // uniform: keys in s.cand
  uint32_t pi = 0;      // the part of the wave's sub-tile (indices only grow)
  uint32_t par = 0;

  for (uint32_t g0 = 0; g0 < total_tiles; g0 += (uint32_t)kScanWaves, par ^= 1u) {
    if (multi_item) {
      const uint64_t t = __hip_atomic_load(my_theta_g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      theta = t > theta ? t : theta;
    }
    const uint32_t g = g0 + wave;
    uint32_t n_cand = 0;   // wave-uniform
    uint64_t key[kFinalSlots];
#pragma unroll
    for (int j = 0; j < kFinalSlots; ++j) key[j] = 0ull;
    if (g < total_tiles) {
      const FinalTile tl = final_tile(parts, part_begin, n_parts, g, pi);
      const uint32_t base = tl.base, gdoc0 = tl.gdoc0;
      uint32_t words, hits;
      const DSortPart* const my_rparts = rparts + (size_t)(part_begin + pi) * (size_t)kMaxRanges;
      const uint32_t m = MULTI ? docset_hit_set_multi(tl.part, rq, my_rparts, base, tl.tile_len, lane, words, hits)
                               : docset_hit_set(tl.part, rq, my_rparts, base, tl.tile_len, lane, words, hits);
      if (words != 0u) {   // uniform
        uint64_t cv[kFinalSlots];
        uint32_t has_bits;
        docset_column64(sparts + part_begin + pi, base, base >> 6, lane, words, cv, has_bits);   // (a leaf without the column: every doc sorts as the missing value)
#pragma unroll
        for (int j = 0; j < kFinalSlots; ++j) {
          // Every lane computes its key and ONE select keeps or drops it (a doc outside the hit set reads code 0; hits of earlier
          // pages still count: `hits`).  Written as docset_sort_kernel writes it -- a store under two nested conditions -- the built
          // kernel kept no key at all behind a cursor and held 143 VGPRs; as a select it holds 95.
          const uint64_t code = ((has_bits >> j) & 1u) != 0u ? cv[j] : missing_code;
          const uint32_t gdoc = gdoc0 + lane + 64u * (uint32_t)j;
          const uint64_t doc_key = sort_key64(reverse, lo, span, db, code, gdoc);
          const bool behind = !has_after || sort64_behind(reverse, code, gdoc, after_code, after_doc);
          key[j] = (((m >> j) & 1u) != 0u && behind && doc_key > theta) ? doc_key : 0ull;
          n_cand += (uint32_t)__popcll(__ballot(key[j] != 0ull));
        }
        final_count_slice(s, tl.part, lane, hits);
      }
    }
    if (lane == 0) s.wcount[par][wave] = n_cand;
    __syncthreads();

    // ---- the round's candidates into the shared buffer (docset_sort_kernel's meeting)
    uint32_t tot = 0, before = 0;
#pragma unroll
    for (uint32_t w2 = 0; w2 < (uint32_t)kScanWaves; ++w2) {
      const uint32_t c = s.wcount[par][w2];
      tot += c;
      before += w2 < wave ? c : 0u;
    }
    if (cnt + tot <= (uint32_t)kFsCandCap) {   // uniform
      docset_push_candidates(s, key, lane, cnt + before);
      cnt += tot;
    } else {
      for (uint32_t w2 = 0; w2 < (uint32_t)kScanWaves; ++w2) {
        const uint32_t c = s.wcount[par][w2];
        if (cnt + c > (uint32_t)kFsCandCap) {   // uniform; cnt > k here (kFsCandCap >= kMaxK + kTileDocs)
          __syncthreads();   // the keys appended so far are in place
          uint64_t thr = 0;
          cnt = topk_compact<kScanThreads, kFsCandCap>(s.cand, cnt, k, &s.sc, &thr);
          if (thr > theta) theta = thr;
          if (tid == 0) atomicMax(my_theta_g, (unsigned long long)thr);
        }
        if (wave == w2) docset_push_candidates(s, key, lane, cnt);
        cnt += c;
      }
    }
  }

  final_epilogue(s, cnt, k, q, tid, slice_sum, item_keys, item_counts, item_hits, k_stride);
}

// ---- a numeric range facet over a doc set (plan.h: DRangeCountQuery, range_interval; nrtgpu_count_docset_ranges_batch) -------------
// docset_terms_count_kernel's frame with rangecount.hip's three replacements: the LDS holds the query's cuts and its n_cuts + 1
// four-byte interval counters instead of the 64 KiB table; a valued hit's lane searches its code among the LDS cuts and does one
// 4-byte LDS add; the flush is one global atomicAdd per non-zero counter behind the one barrier.  WIDE: the count column holds
// 64-bit codes (docset_column64) and the cuts are 64-bit.  MULTI concerns only the doc set's own 32-bit range clauses
// (docset_hit_set_multi), as in docset_sort64_kernel<MULTI>: the count column is single-valued.  A word without an accepted doc
// costs no load.
template <class CODE>
struct DocsetRangeSmem {
  CODE cuts[kMaxRangeCuts];                     // the query's cut points, ascending
  uint32_t counters[kMaxRangeCuts + 1];         // the item's hits per elementary interval, shared by the waves
  uint32_t slot_hits[kSliceSlots];              // what final_count_slice and the epilogue read (finalscore.hiph: FinalSmem)
  uint32_t slot_slice[kSliceSlots];
};
static_assert(sizeof(DSort64Part) == sizeof(DSortPart), "the count column's record is read as either");

template <bool WIDE, bool MULTI>
__global__ __launch_bounds__(kScanThreads, kScanWaves / 4)
void docset_range_count_kernel(const DItem* __restrict__ items, const DPart* __restrict__ parts, const DQuery* __restrict__ queries,
                               const DRangeCountQuery* __restrict__ cqueries, const DRangeQuery* __restrict__ rqueries,
                               const DSortPart* __restrict__ sparts, const DSortPart* __restrict__ rparts, const void* __restrict__ cuts_g,
                               uint32_t* __restrict__ counters_g, uint32_t* __restrict__ slice_sum, uint32_t* __restrict__ item_counts,
                               uint64_t* __restrict__ item_hits) {
  typedef typename std::conditional<WIDE, uint64_t, uint32_t>::type CODE;
  __shared__ DocsetRangeSmem<CODE> s;
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), lane = tid & 63u;
  const DItem* const item = items + blockIdx.x;
  const uint32_t query = item->query, part_begin = item->part_begin, n_parts = item->n_parts;
  const DQuery* const q = queries + query;
  const DRangeCountQuery* const cq = cqueries + query;
  const DRangeQuery* const rq = rqueries + query;
  const uint32_t n_cuts = min(cq->n_cuts, (uint32_t)kMaxRangeCuts);
  const CODE* const my_cuts = (const CODE*)cuts_g + cq->cut_off;
  uint32_t* const my_counters = counters_g + cq->counter_off;

  if (tid < n_cuts) s.cuts[tid] = my_cuts[tid];
  if (tid <= (uint32_t)kMaxRangeCuts) s.counters[tid] = 0u;
  if (tid < (uint32_t)kSliceSlots) s.slot_hits[tid] = s.slot_slice[tid] = 0u;
  __syncthreads();

  const uint32_t total_tiles = final_total_tiles(parts, part_begin, n_parts);
  uint32_t pi = 0;      // the part of the wave's sub-tile (indices only grow)

  for (uint32_t g = wave; g < total_tiles; g += (uint32_t)kScanWaves) {
    const FinalTile tl = final_tile(parts, part_begin, n_parts, g, pi);
    const uint32_t base = tl.base;
    uint32_t words, hits;
    const DSortPart* const my_rparts = rparts + (size_t)(part_begin + pi) * (size_t)kMaxRanges;
    const uint32_t m = MULTI ? docset_hit_set_multi(tl.part, rq, my_rparts, base, tl.tile_len, lane, words, hits)
                             : docset_hit_set(tl.part, rq, my_rparts, base, tl.tile_len, lane, words, hits);
    if (words == 0u) continue;   // uniform
    final_count_slice(s, tl.part, lane, hits);
    CODE cv[kFinalSlots];
    uint32_t has_bits;
    bool there;
    if constexpr (WIDE) there = docset_column64((const DSort64Part*)(sparts + part_begin + pi), base, base >> 6, lane, words, cv, has_bits);
    else there = docset_column(sparts + part_begin + pi, base, base >> 6, lane, words, cv, has_bits);
    if (!there) continue;   // uniform: the leaf lacks the column: its hits add to no range
    const uint32_t valued = m & has_bits;
#pragma unroll
    for (int j = 0; j < kFinalSlots; ++j) {
      if (__ballot(((valued >> j) & 1u) != 0u) == 0ull) continue;   // uniform: no valued hit in the word
      const uint32_t iv = range_interval(s.cuts, n_cuts, cv[j]);     // (every lane of the word searches: measured against the hit lanes alone, rangecount.hip)
      if (((valued >> j) & 1u) != 0u) atomicAdd(&s.counters[iv], 1u);
    }
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
    uint32_t n = 0;
    const uint32_t gte_floor = q->gte_floor, slice_base = q->slice_base;
    for (int i = 0; i < kSliceSlots; ++i) {
      const uint32_t h = s.slot_hits[i];
      n += h;
      if (h != 0u && gte_floor != 0xFFFFFFFFu) atomicAdd(&slice_sum[slice_base + s.slot_slice[i]], h);
    }
    item_hits[blockIdx.x] = n;
  }
}

// ---- a terms count over a 64-BIT column (plan.h: DTermsState64; termstables64.hiph; nrtgpu_count_docset_terms64_batch) ------------
// docset_terms_count_kernel (MULTI: the doc set's own 32-bit range clauses may name multi-valued columns -- docset_hit_set_multi,
// as in docset_sort64_kernel<MULTI>) with the count column read as 64-bit codes (docset_column64) and the 64-bit tables.  Only
// the counted column is wide, and it is single-valued.  Hits are taken by popcount; a word without an accepted doc costs no
// column load.  Everything else is that kernel's.
struct DocsetTerms64Smem {
  Terms64Lds table;                             // the item's count table (plan.h), shared by the waves
  uint32_t slot_hits[kSliceSlots];              // what final_count_slice and the epilogue read (finalscore.hiph: FinalSmem)
  uint32_t slot_slice[kSliceSlots];
};

template <bool MULTI>
__global__ __launch_bounds__(kScanThreads, kScanWaves / 4)
void docset_terms_count64_kernel(const DItem* __restrict__ items, const DPart* __restrict__ parts, const DQuery* __restrict__ queries,
                                 const DTermsQuery* __restrict__ tqueries, const DRangeQuery* __restrict__ rqueries,
                                 const DSort64Part* __restrict__ sparts, const DSortPart* __restrict__ rparts, DTermsState64* __restrict__ states,
                                 unsigned long long* __restrict__ table_keys, uint32_t* __restrict__ table_counts, uint32_t* __restrict__ slice_sum,
                                 uint32_t* __restrict__ item_counts, uint64_t* __restrict__ item_hits) {
  __shared__ DocsetTerms64Smem s;
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), lane = tid & 63u;
  const DItem* const item = items + blockIdx.x;
  const uint32_t query = item->query, part_begin = item->part_begin, n_parts = item->n_parts;
  const DQuery* const q = queries + query;
  const DTermsQuery* const tq = tqueries + query;
  const DRangeQuery* const rq = rqueries + query;
  const uint32_t max_buckets = tq->max_buckets, shift = tq->table_shift;
  const uint32_t mask = (1u << (32u - shift)) - 1u;
  unsigned long long* const keys = table_keys + tq->table_off;
  uint32_t* const counts = table_counts + tq->table_off;
  DTermsState64* const st = states + query;

  terms_lds_clear64(s.table, tid, (uint32_t)kScanThreads);
  if (tid < (uint32_t)kSliceSlots) s.slot_hits[tid] = s.slot_slice[tid] = 0u;
  __syncthreads();

  const uint32_t total_tiles = final_total_tiles(parts, part_begin, n_parts);
  uint32_t pi = 0;      // the part of the wave's sub-tile (indices only grow)

  for (uint32_t g = wave; g < total_tiles; g += (uint32_t)kScanWaves) {
    const FinalTile tl = final_tile(parts, part_begin, n_parts, g, pi);
    const uint32_t base = tl.base;
    uint32_t words, hits;
    const DSortPart* const my_rparts = rparts + (size_t)(part_begin + pi) * (size_t)kMaxRanges;
    const uint32_t m = MULTI ? docset_hit_set_multi(tl.part, rq, my_rparts, base, tl.tile_len, lane, words, hits)
                             : docset_hit_set(tl.part, rq, my_rparts, base, tl.tile_len, lane, words, hits);
    if (words == 0u) continue;   // uniform
    final_count_slice(s, tl.part, lane, hits);
    // an overflowed query's buckets are void: its items go on counting hits only (a flag read once, not waited for)
    if (__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(&st->overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != 0) continue;
    uint64_t cv[kFinalSlots];
    uint32_t has_bits;
    if (!docset_column64(sparts + part_begin + pi, base, base >> 6, lane, words, cv, has_bits)) continue;   // the leaf lacks the column: its hits add to no bucket
    const uint32_t valued = m & has_bits;
#pragma unroll
    for (int j = 0; j < kFinalSlots; ++j)
      if (((valued >> j) & 1u) != 0u) terms_lds_add64(s.table, keys, counts, shift, mask, max_buckets, st, cv[j], 1u);
  }

  // ---- the item's table into the query's, once
  __syncthreads();
  terms_lds_flush64(s.table, keys, counts, shift, mask, max_buckets, st, tid, (uint32_t)kScanThreads);

  // ---- epilogue: final_epilogue's for an item without candidates
  if (tid == 0) {
    item_counts[blockIdx.x] = 0u;
    uint32_t n = 0;
    const uint32_t gte_floor = q->gte_floor, slice_base = q->slice_base;
    for (int i = 0; i < kSliceSlots; ++i) {
      const uint32_t h = s.slot_hits[i];
      n += h;
      if (h != 0u && gte_floor != 0xFFFFFFFFu) atomicAdd(&slice_sum[slice_base + s.slot_slice[i]], h);
    }
    item_hits[blockIdx.x] = n;
  }
}

// terms_compact64_kernel's launch (termscount64.hip)
void launch_terms_compact64(hipStream_t stream, const DTermsQuery* tqueries, DTermsState64* states, const unsigned long long* table_keys,
                            const uint32_t* table_counts, unsigned long long* out_codes, uint32_t* out_counts, uint32_t n_queries, uint32_t out_cap);

void launch_docset_terms_count64(hipStream_t stream, bool multi, const FinalScoreArgs& a, const DTermsQuery* tqueries, const DRangeQuery* rqueries,
                                 const DSort64Part* sparts, const DSortPart* rparts, DTermsState64* states, unsigned long long* table_keys,
                                 uint32_t* table_counts, unsigned long long* out_codes, uint32_t* out_counts, uint32_t n_queries, uint32_t out_cap) {
  if (a.n_items != 0) {
    if (multi)
      hipLaunchKernelGGL(docset_terms_count64_kernel<true>, dim3(a.n_items), dim3(kScanThreads), 0, stream, a.items, a.parts, a.queries, tqueries, rqueries,
                         sparts, rparts, states, table_keys, table_counts, a.slice_sum, a.item_counts, a.item_hits);
    else
      hipLaunchKernelGGL(docset_terms_count64_kernel<false>, dim3(a.n_items), dim3(kScanThreads), 0, stream, a.items, a.parts, a.queries, tqueries, rqueries,
                         sparts, rparts, states, table_keys, table_counts, a.slice_sum, a.item_counts, a.item_hits);
  }
  launch_terms_compact64(stream, tqueries, states, table_keys, table_counts, out_codes, out_counts, n_queries, out_cap);
}

void launch_docset_range_count(hipStream_t stream, bool wide, bool multi, const FinalScoreArgs& a, const DRangeCountQuery* cqueries,
                               const DRangeQuery* rqueries, const DSortPart* sparts, const DSortPart* rparts, const void* cuts, uint32_t* counters) {
  if (a.n_items == 0) return;
#define NRT_LAUNCH_DOCSET_RANGE_COUNT(W, M)                                                                                                          \
  hipLaunchKernelGGL((docset_range_count_kernel<W, M>), dim3(a.n_items), dim3(kScanThreads), 0, stream, a.items, a.parts, a.queries, cqueries, rqueries, \
                     sparts, rparts, cuts, counters, a.slice_sum, a.item_counts, a.item_hits)
  if (wide && multi) NRT_LAUNCH_DOCSET_RANGE_COUNT(true, true);
  else if (wide) NRT_LAUNCH_DOCSET_RANGE_COUNT(true, false);
  else if (multi) NRT_LAUNCH_DOCSET_RANGE_COUNT(false, true);
  else NRT_LAUNCH_DOCSET_RANGE_COUNT(false, false);
#undef NRT_LAUNCH_DOCSET_RANGE_COUNT
}

void launch_docset_sort64(hipStream_t stream, const FinalScoreArgs& a, const DSort64Query* squeries, const DRangeQuery* rqueries, const DSort64Part* sparts,
                          const DSortPart* rparts) {
  if (a.n_items == 0) return;
  hipLaunchKernelGGL(docset_sort64_kernel<false>, dim3(a.n_items), dim3(kScanThreads), 0, stream, a.items, a.parts, a.queries, squeries, rqueries, sparts,
                     rparts, a.theta_g, a.slice_sum, a.item_keys, a.item_counts, a.item_hits, a.k_stride);
}

void launch_docset_sort64_multi(hipStream_t stream, const FinalScoreArgs& a, const DSort64Query* squeries, const DRangeQuery* rqueries,
                                const DSort64Part* sparts, const DSortPart* rparts) {
  if (a.n_items == 0) return;
  hipLaunchKernelGGL(docset_sort64_kernel<true>, dim3(a.n_items), dim3(kScanThreads), 0, stream, a.items, a.parts, a.queries, squeries, rqueries, sparts,
                     rparts, a.theta_g, a.slice_sum, a.item_keys, a.item_counts, a.item_hits, a.k_stride);
}

// terms_compact_kernel's launch (termscount.hip): the occupied slots of every query's table packed into `out`
void launch_terms_compact(hipStream_t stream, const DTermsQuery* tqueries, DTermsState* states, const unsigned long long* tables, unsigned long long* out,
                          uint32_t n_queries, uint32_t out_cap);

void launch_docset_sort(hipStream_t stream, const FinalScoreArgs& a, const DSortQuery* squeries, const DRangeQuery* rqueries, const DSortPart* sparts,
                        const DSortPart* rparts) {
  if (a.n_items == 0) return;
  hipLaunchKernelGGL(docset_sort_kernel, dim3(a.n_items), dim3(kScanThreads), 0, stream, a.items, a.parts, a.queries, squeries, rqueries, sparts, rparts,
                     a.theta_g, a.slice_sum, a.item_keys, a.item_counts, a.item_hits, a.k_stride);
}

void launch_docset_terms_count(hipStream_t stream, const FinalScoreArgs& a, const DTermsQuery* tqueries, const DRangeQuery* rqueries, const DSortPart* sparts,
                               const DSortPart* rparts, DTermsState* states, unsigned long long* tables, unsigned long long* out, uint32_t n_queries,
                               uint32_t out_cap) {
  if (a.n_items != 0)
    hipLaunchKernelGGL(docset_terms_count_kernel, dim3(a.n_items), dim3(kScanThreads), 0, stream, a.items, a.parts, a.queries, tqueries, rqueries, sparts,
                       rparts, states, tables, a.slice_sum, a.item_counts, a.item_hits);
  launch_terms_compact(stream, tqueries, states, tables, out, n_queries, out_cap);
}

void launch_docset_sort_multi(hipStream_t stream, const FinalScoreArgs& a, const DSortQuery* squeries, const DRangeQuery* rqueries, const DSortPart* sparts,
                              const DSortPart* rparts) {
  if (a.n_items == 0) return;
  hipLaunchKernelGGL(docset_sort_multi_kernel, dim3(a.n_items), dim3(kScanThreads), 0, stream, a.items, a.parts, a.queries, squeries, rqueries, sparts,
                     rparts, a.theta_g, a.slice_sum, a.item_keys, a.item_counts, a.item_hits, a.k_stride);
}

void launch_docset_terms_count_multi(hipStream_t stream, const FinalScoreArgs& a, const DTermsQuery* tqueries, const DRangeQuery* rqueries,
                                     const DSortPart* sparts, const DSortPart* rparts, DTermsState* states, unsigned long long* tables, unsigned long long* out,
                                     uint32_t n_queries, uint32_t out_cap) {
  if (a.n_items != 0)
    hipLaunchKernelGGL(docset_terms_count_multi_kernel, dim3(a.n_items), dim3(kScanThreads), 0, stream, a.items, a.parts, a.queries, tqueries, rqueries,
                       sparts, rparts, states, tables, a.slice_sum, a.item_counts, a.item_hits);
  launch_terms_compact(stream, tqueries, states, tables, out, n_queries, out_cap);
}

}  // namespace nrtgpu
