// docset.hip -- the gfx950 kernels of the doc-set requests (include/nrtgpu.h: nrtgpu_search_docset_sorted_batch,
// nrtgpu_count_docset_terms_batch and their 64-bit and range-facet siblings): a sort by field or a count whose hit set is a DOC
// SET -- liveDocs, FILTER / MUST_NOT masks, numeric range clauses (the reference's MatchAllDocsQuery, a BooleanQuery of FILTER
// clauses only, IntFieldDef / FloatFieldDef.getRangeQuery) -- and no text clause.
//
//   docset_sort_kernel<SORT, MULTI>    per sub-tile the hit set, then keys for its docs and the item's top-k.  SORT: the sort
//                                      column's width -- DocsetSort32 (plan.h: sort_key) or DocsetSort64 (sort_key64)
//   docset_count_kernel<COUNT, MULTI>  the same hit set; every hit with a value adds 1 under its value's code.  COUNT: what is
//                                      counted and where -- DocsetTerms32 (termstables.hiph) or DocsetRanges<WIDE> (the elementary
//                                      interval of the code among the query's cut points)
//   docset_terms_count_multi_kernel    the count frame written out for a 32-bit terms count in calls that name a multi-valued column
//   docset_terms_count64_kernel<MULTI> ... and over a 64-BIT count column (termstables64.hiph); neither meets the rules for a
//                                      refactor under the frame (behind it)
//
// MULTI (docset_terms_count_multi_kernel): some 32-bit range clause of the call names a MULTI-VALUED column (DRangeQuery.multi),
// or, for the 32-bit terms count alone, the count column is one (kTermsQueryMulti).  The arity is a wave-uniform flag per clause /
// per query, so a batch that mixes arities is one launch; a call without such a column launches the other form, which never
// reads the flags.  The reference's rules: a range clause keeps a doc iff ANY of its values lies in the range (SortedNumericDocValuesField.
// newSlowRangeQuery); every value instance of a hit adds 1 (IntTermsCollectorManager.java:142-152).
//
// A policy names its per-query record and per-part column types, loads the record's fields once into scalars, and is dissolved
// by the inlining: it holds nothing that outlives it (finalscore.hiph: everything __forceinline__, scalars by value).
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

// docset_column over a column of 64-bit codes (plan.h: DSort64Part): the lane's 8-byte codes of the words in `words` and its
// `has` bits.
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

// A MULTI-VALUED column (plan.h: DSortPart: codes[] behind start[]): a lane's start[d] and start[d + 1] for the words in `words`
// (the others read 0: no value).  start[] is padded to whole sub-tiles plus one: no bounds test.
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

// The sub-tile's hit set as the lane's view: the accept words narrowed by every range clause of the query in turn.  rparts: the
// part's kMaxRanges column records.  words / hits: docset_census of the result.  MULTI: a clause's arity is read from rq->multi.
// The two forms are written out and must be kept the same by hand, like the meeting of finalscore.hiph: every single text that
// was tried -- either form's order of loads and tests for both, the clause step as a helper, the two steps side by side under
// `if constexpr` -- rebuilt all kernels of at least one kind with other registers, spills and instruction counts.
template <bool MULTI>
__device__ __forceinline__ uint32_t docset_hit_set(const DPart* part, const DRangeQuery* rq, const DSortPart* rparts, uint32_t base, uint32_t tile_len,
                                                   uint32_t lane, uint32_t& words, uint32_t& hits);

template <>
__device__ __forceinline__ uint32_t docset_hit_set<false>(const DPart* part, const DRangeQuery* rq, const DSortPart* rparts, uint32_t base,
                                                          uint32_t tile_len, uint32_t lane, uint32_t& words, uint32_t& hits) {
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

template <>
__device__ __forceinline__ uint32_t docset_hit_set<true>(const DPart* part, const DRangeQuery* rq, const DSortPart* rparts, uint32_t base,
                                                         uint32_t tile_len, uint32_t lane, uint32_t& words, uint32_t& hits) {
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

// ---- the sort frame ---------------------------------------------------------------------------------------------------------------
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

// A SORT policy: Query / Part / Code (the per-query record, the sort column's per-part record, a code of it), column() (the lane's
// slice of the sort column) and the candidate key of slot j of the lane's view -- the doc's key where the doc is a hit above theta
// and behind the cursor, else 0 (hits of earlier pages still count: `hits`).  The key takes one of two forms, chosen by
// kKeyInPlace, because each width's kernel is built well from one of them only: DocsetSort32 stores into the frame's zeroed key[]
// under two nested conditions (returned as a value the compiler makes it a select and the two kernels others: 92 / 93 VGPRs for
// 124 / 125, not measured); DocsetSort64 returns one select (in place: 143 VGPRs for 95).

// A sort by a 32-bit column (plan.h: DSortQuery, sort_key): the packed key itself carries the cursor test.
struct DocsetSort32 {
  typedef DSortQuery Query;
  typedef DSortPart Part;
  typedef uint32_t Code;
  static constexpr bool kKeyInPlace = true;
  const uint32_t reverse, missing_code;
  const bool no_after;
  const uint64_t after_key;
  __device__ __forceinline__ explicit DocsetSort32(const Query* sq)
      : reverse(sq->reverse), missing_code(sq->missing_code), no_after(sq->has_after == 0u), after_key(sq->after_key) {}
  static __device__ __forceinline__ bool column(const Part* sp, uint32_t base, uint32_t word0, uint32_t lane, uint32_t words, Code (&cv)[kFinalSlots],
                                                uint32_t& has_bits) {
    return docset_column(sp, base, word0, lane, words, cv, has_bits);
  }
  // key[j] is 0 on entry
  __device__ __forceinline__ void candidate(uint32_t m, uint32_t has_bits, const Code (&cv)[kFinalSlots], uint32_t gdoc0, uint32_t lane, uint64_t theta, int j,
                                            uint64_t (&key)[kFinalSlots]) const {
    if (((m >> j) & 1u) != 0u) {
      const uint32_t code = ((has_bits >> j) & 1u) != 0u ? cv[j] : missing_code;
      const uint64_t doc_key = sort_key(reverse, code, gdoc0 + lane + 64u * (uint32_t)j);
      if (doc_key > theta && (no_after || doc_key < after_key)) key[j] = doc_key;
    }
  }
};

// A sort by a 64-bit column (plan.h: DSort64Query, sort_key64): the key packs the code's offset in the call's window, the cursor
// is tested on (code, doc).
struct DocsetSort64 {
  typedef DSort64Query Query;
  typedef DSort64Part Part;
  typedef uint64_t Code;
  static constexpr bool kKeyInPlace = false;
  const uint64_t lo, span, missing_code, after_code;
  const uint32_t reverse, after_doc, db;
  const bool no_after;
  __device__ __forceinline__ explicit DocsetSort64(const Query* sq)
      : lo(sq->lo), span(sq->span), missing_code(sq->missing_code), after_code(sq->after_code), reverse(sq->reverse), after_doc(sq->after_doc),
        db(min(max(sq->db, 1u), 31u)), no_after(sq->has_after == 0u) {}
  static __device__ __forceinline__ bool column(const Part* sp, uint32_t base, uint32_t word0, uint32_t lane, uint32_t words, Code (&cv)[kFinalSlots],
                                                uint32_t& has_bits) {
    return docset_column64(sp, base, word0, lane, words, cv, has_bits);
  }
  // Every lane computes its key and ONE select keeps or drops it (a doc outside the hit set reads code 0).
  __device__ __forceinline__ uint64_t candidate(uint32_t m, uint32_t has_bits, int j, Code value, uint32_t gdoc, uint64_t theta) const {
    const uint64_t code = ((has_bits >> j) & 1u) != 0u ? value : missing_code;
    const uint64_t doc_key = sort_key64(reverse, lo, span, db, code, gdoc);
    const bool behind = no_after || sort64_behind(reverse, code, gdoc, after_code, after_doc);
    return (((m >> j) & 1u) != 0u && behind && doc_key > theta) ? doc_key : 0ull;
  }
};

typedef FinalSmem<kScanWaves, kFsCandCap> DocsetSortSmem;   // (its `cache` is carried but neither written nor read: no score is computed)

template <class SORT, bool MULTI>
__global__ __launch_bounds__(kScanThreads, kScanWaves / 4)
void docset_sort_kernel(const DItem* __restrict__ items, const DPart* __restrict__ parts, const DQuery* __restrict__ queries,
                        const typename SORT::Query* __restrict__ squeries, const DRangeQuery* __restrict__ rqueries,
                        const typename SORT::Part* __restrict__ sparts, const DSortPart* __restrict__ rparts, unsigned long long* __restrict__ theta_g,
                        uint32_t* __restrict__ slice_sum, uint64_t* __restrict__ item_keys, uint32_t* __restrict__ item_counts,
                        uint64_t* __restrict__ item_hits, uint32_t k_stride) {
  __shared__ DocsetSortSmem s;
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), lane = tid & 63u;
  const DItem* const item = items + blockIdx.x;
  const uint32_t query = item->query, part_begin = item->part_begin, n_parts = item->n_parts;
  const DQuery* const q = queries + query;
  const uint32_t k = min(q->k, (uint32_t)kMaxK);
  const typename SORT::Query* const sq = squeries + query;
  const DRangeQuery* const rq = rqueries + query;
  const SORT sort(sq);
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
      const uint32_t m = docset_hit_set<MULTI>(tl.part, rq, rparts + (size_t)(part_begin + pi) * (size_t)kMaxRanges, base, tl.tile_len, lane, words, hits);
      if (words != 0u) {   // uniform
        typename SORT::Code cv[kFinalSlots];
        uint32_t has_bits;
        SORT::column(sparts + part_begin + pi, base, base >> 6, lane, words, cv, has_bits);   // (a leaf without the column: every doc sorts as the missing value)
#pragma unroll
        for (int j = 0; j < kFinalSlots; ++j) {
          if constexpr (SORT::kKeyInPlace) sort.candidate(m, has_bits, cv, gdoc0, lane, theta, j, key);
          else key[j] = sort.candidate(m, has_bits, j, cv[j], gdoc0 + lane + 64u * (uint32_t)j, theta);
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

// ---- the count frame --------------------------------------------------------------------------------------------------------------
// A COUNT policy: Query / Part (the per-query record, the count column's per-part record), Out0 / Out1 (what the call's two
// output pointers point at: each a __restrict__ kernel argument -- inside a struct argument they lose that and the built kernels
// change more), Smem (the workgroup's LDS: its combiner, and the slot_hits / slot_slice final_count_slice and the epilogue
// read, as in finalscore.hiph: FinalSmem), and
//   clear(s, tid)       the combiner emptied (all threads; the frame's barrier follows)
//   closed()            uniform: the query's buckets are void, its items go on counting hits only
//   add(s, ...)         the sub-tile's valued hits of m into the combiner
//   flush(s, tid)       the item's combiner into the query's output, once (all threads, behind the barrier after the last add)

// A terms count over a 32-bit column (termstables.hiph): the item's 64 KiB LDS table in front of the query's global one.
struct DocsetTerms32 {
  typedef DTermsQuery Query;
  typedef DSortPart Part;
  typedef DTermsState Out0;          // the queries' states
  typedef unsigned long long Out1;   // their tables
  struct Smem {
    unsigned long long table[kTermsLdsSlots];     // the item's count table (plan.h), shared by the waves
    uint32_t slot_hits[kSliceSlots];
    uint32_t slot_slice[kSliceSlots];
  };
  const uint32_t max_buckets, shift, mask;
  unsigned long long* const table;
  DTermsState* const st;
  __device__ __forceinline__ DocsetTerms32(const Query* tq, Out0* states, Out1* tables, uint32_t query)
      : max_buckets(tq->max_buckets), shift(tq->table_shift), mask((1u << (32u - tq->table_shift)) - 1u), table(tables + tq->table_off),
        st(states + query) {}
  __device__ __forceinline__ void clear(Smem& s, uint32_t tid) const {
    for (uint32_t i = tid; i < (uint32_t)kTermsLdsSlots; i += (uint32_t)kScanThreads) s.table[i] = 0ull;
  }
  // (a flag read once, not waited for)
  __device__ __forceinline__ bool closed() const {
    return __builtin_amdgcn_readfirstlane((int)__hip_atomic_load(&st->overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != 0;
  }
  __device__ __forceinline__ void add(Smem& s, const Part* sp, uint32_t base, uint32_t lane, uint32_t words, uint32_t m) const {
    uint32_t cv[kFinalSlots], has_bits;
    if (!docset_column(sp, base, base >> 6, lane, words, cv, has_bits)) return;   // the leaf lacks the column: its hits add to no bucket
    const uint32_t valued = m & has_bits;
#pragma unroll
    for (int j = 0; j < kFinalSlots; ++j)
      if (((valued >> j) & 1u) != 0u) terms_lds_add(s.table, table, shift, mask, max_buckets, st, cv[j], 1u);
  }
  __device__ __forceinline__ void flush(const Smem& s, uint32_t tid) const {
    if (__hip_atomic_load(&st->overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) {
      for (uint32_t i = tid; i < (uint32_t)kTermsLdsSlots; i += (uint32_t)kScanThreads) {
        const unsigned long long w = s.table[i];
        if (w != 0ull) terms_global_add(table, shift, mask, max_buckets, st, (uint32_t)w, (uint32_t)(w >> 32));
      }
    }
  }
};

// A numeric range facet (plan.h: DRangeCountQuery, range_interval; rangecount.hip's three replacements): the LDS holds the
// query's cuts and its n_cuts + 1 four-byte interval counters; a valued hit's lane searches its code among the LDS cuts and does
// one 4-byte LDS add; the flush is one global atomicAdd per non-zero counter.  WIDE: the count column holds 64-bit codes
// (docset_column64; its record is read as a DSort64Part, plan.h) and the cuts are 64-bit.  The column is single-valued.
template <bool WIDE>
struct DocsetRanges {
  typedef typename std::conditional<WIDE, uint64_t, uint32_t>::type Code;
  typedef DRangeCountQuery Query;
  typedef DSortPart Part;
  typedef const void Out0;   // the call's cuts
  typedef uint32_t Out1;     // its interval counters
  struct Smem {
    Code cuts[kMaxRangeCuts];                     // the query's cut points, ascending
    uint32_t counters[kMaxRangeCuts + 1];         // the item's hits per elementary interval, shared by the waves
    uint32_t slot_hits[kSliceSlots];
    uint32_t slot_slice[kSliceSlots];
  };
  const uint32_t n_cuts;
  const Code* const my_cuts;
  uint32_t* const my_counters;
  __device__ __forceinline__ DocsetRanges(const Query* cq, Out0* cuts, Out1* counters, uint32_t)
      : n_cuts(min(cq->n_cuts, (uint32_t)kMaxRangeCuts)), my_cuts((const Code*)cuts + cq->cut_off), my_counters(counters + cq->counter_off) {}
  __device__ __forceinline__ void clear(Smem& s, uint32_t tid) const {
    if (tid < n_cuts) s.cuts[tid] = my_cuts[tid];
    if (tid <= (uint32_t)kMaxRangeCuts) s.counters[tid] = 0u;
  }
  __device__ __forceinline__ bool closed() const { return false; }
  __device__ __forceinline__ void add(Smem& s, const Part* sp, uint32_t base, uint32_t lane, uint32_t words, uint32_t m) const {
    Code cv[kFinalSlots];
    uint32_t has_bits;
    bool there;
    if constexpr (WIDE) there = docset_column64((const DSort64Part*)sp, base, base >> 6, lane, words, cv, has_bits);
    else there = docset_column(sp, base, base >> 6, lane, words, cv, has_bits);
    if (!there) return;   // uniform: the leaf lacks the column: its hits add to no range
    const uint32_t valued = m & has_bits;
#pragma unroll
    for (int j = 0; j < kFinalSlots; ++j) {
      if (__ballot(((valued >> j) & 1u) != 0u) == 0ull) continue;   // uniform: no valued hit in the word
      const uint32_t iv = range_interval(s.cuts, n_cuts, cv[j]);     // (every lane of the word searches: measured against the hit lanes alone, rangecount.hip)
      if (((valued >> j) & 1u) != 0u) atomicAdd(&s.counters[iv], 1u);
    }
  }
  __device__ __forceinline__ void flush(const Smem& s, uint32_t tid) const {
    if (tid <= n_cuts) {
      const uint32_t c = s.counters[tid];
      if (c != 0u) atomicAdd(&my_counters[tid], c);
    }
  }
};

template <class COUNT, bool MULTI>
__global__ __launch_bounds__(kScanThreads, kScanWaves / 4)
void docset_count_kernel(const DItem* __restrict__ items, const DPart* __restrict__ parts, const DQuery* __restrict__ queries,
                         const typename COUNT::Query* __restrict__ cqueries, const DRangeQuery* __restrict__ rqueries,
                         const typename COUNT::Part* __restrict__ sparts, const DSortPart* __restrict__ rparts, typename COUNT::Out0* __restrict__ out0,
                         typename COUNT::Out1* __restrict__ out1, uint32_t* __restrict__ slice_sum, uint32_t* __restrict__ item_counts,
                         uint64_t* __restrict__ item_hits) {
  __shared__ typename COUNT::Smem s;
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), lane = tid & 63u;
  const DItem* const item = items + blockIdx.x;
  const uint32_t query = item->query, part_begin = item->part_begin, n_parts = item->n_parts;
  const DQuery* const q = queries + query;
  const typename COUNT::Query* const cq = cqueries + query;
  const DRangeQuery* const rq = rqueries + query;
  const COUNT count(cq, out0, out1, query);

  count.clear(s, tid);
  if (tid < (uint32_t)kSliceSlots) s.slot_hits[tid] = s.slot_slice[tid] = 0u;
  __syncthreads();

  const uint32_t total_tiles = final_total_tiles(parts, part_begin, n_parts);
  uint32_t pi = 0;      // the part of the wave's sub-tile (indices only grow)

  for (uint32_t g = wave; g < total_tiles; g += (uint32_t)kScanWaves) {
    const FinalTile tl = final_tile(parts, part_begin, n_parts, g, pi);
    const uint32_t base = tl.base;
    uint32_t words, hits;
    const uint32_t m = docset_hit_set<MULTI>(tl.part, rq, rparts + (size_t)(part_begin + pi) * (size_t)kMaxRanges, base, tl.tile_len, lane, words, hits);
    if (words == 0u) continue;   // uniform
    final_count_slice(s, tl.part, lane, hits);
    if (count.closed()) continue;
    count.add(s, sparts + part_begin + pi, base, lane, words, m);
  }

  // ---- the item's combiner into the query's output, once
  __syncthreads();
  count.flush(s, tid);
  final_epilogue_no_candidates(s, q, tid, slice_sum, item_counts, item_hits);
}

// ---- a 32-bit terms count in calls that name a MULTI-VALUED column -----------------------------------------------------------------
// The count frame WRITTEN OUT over DocsetTerms32's tables and docset_hit_set<true>, with the count column's arity read from the
// query's record (kTermsQueryMulti): every value of a hit adds 1, each hit lane walking its own codes[start[d] .. start[d + 1]).
// Under the frame (a multi-valued branch in DocsetTerms32::add) it timed 0.29 % over this text on one line of
// scripts/gpu_multi_values.py where this text's three runs lie within 0.27 %, and under it on the eleven others.
__global__ __launch_bounds__(kScanThreads, kScanWaves / 4)
void docset_terms_count_multi_kernel(const DItem* __restrict__ items, const DPart* __restrict__ parts, const DQuery* __restrict__ queries,
                                     const DTermsQuery* __restrict__ tqueries, const DRangeQuery* __restrict__ rqueries,
                                     const DSortPart* __restrict__ sparts, const DSortPart* __restrict__ rparts, DTermsState* __restrict__ states,
                                     unsigned long long* __restrict__ tables, uint32_t* __restrict__ slice_sum, uint32_t* __restrict__ item_counts,
                                     uint64_t* __restrict__ item_hits) {
  __shared__ DocsetTerms32::Smem s;
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
    const uint32_t m = docset_hit_set<true>(tl.part, rq, rparts + (size_t)(part_begin + pi) * (size_t)kMaxRanges, base, tl.tile_len, lane, words, hits);
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

  final_epilogue_no_candidates(s, q, tid, slice_sum, item_counts, item_hits);
}

// ---- a terms count over a 64-BIT column (plan.h: DTermsState64; termstables64.hiph; nrtgpu_count_docset_terms64_batch) ------------
// The count frame WRITTEN OUT, and to be kept the same as docset_count_kernel by hand: the count column read as 64-bit codes
// (docset_column64), the 64-bit tables, three output pointers.  Only the counted column is wide, and it is single-valued; MULTI
// concerns the doc set's own 32-bit range clauses.  As a policy under the frame (an object with its fields; its add as a free
// function that takes every scalar by value; the frame as a __forceinline__ function inside a forwarding kernel -- fields as the
// frame's locals are the same optimised IR) this kernel builds to 168 VGPRs and 1224 / 1432 B of scratch for 61 / 64 and none:
// the optimised IR is the parent's but for the place of the block behind the loop, and the register allocator falls over
// (DESIGN 4.1h).
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
    const uint32_t m = docset_hit_set<MULTI>(tl.part, rq, rparts + (size_t)(part_begin + pi) * (size_t)kMaxRanges, base, tl.tile_len, lane, words, hits);
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

  final_epilogue_no_candidates(s, q, tid, slice_sum, item_counts, item_hits);
}

// ---- launches: `multi` chooses the MULTI form --------------------------------------------------------------------------------------
template <class SORT>
static void launch_sort(hipStream_t stream, bool multi, const FinalScoreArgs& a, const typename SORT::Query* squeries, const DRangeQuery* rqueries,
                        const typename SORT::Part* sparts, const DSortPart* rparts) {
  if (a.n_items == 0) return;
  const auto kernel = multi ? docset_sort_kernel<SORT, true> : docset_sort_kernel<SORT, false>;
  hipLaunchKernelGGL(kernel, dim3(a.n_items), dim3(kScanThreads), 0, stream, a.items, a.parts, a.queries, squeries, rqueries, sparts, rparts, a.theta_g,
                     a.slice_sum, a.item_keys, a.item_counts, a.item_hits, a.k_stride);
}

void launch_docset_sort(hipStream_t stream, bool multi, const FinalScoreArgs& a, const DSortQuery* squeries, const DRangeQuery* rqueries,
                        const DSortPart* sparts, const DSortPart* rparts) {
  launch_sort<DocsetSort32>(stream, multi, a, squeries, rqueries, sparts, rparts);
}

void launch_docset_sort64(hipStream_t stream, bool multi, const FinalScoreArgs& a, const DSort64Query* squeries, const DRangeQuery* rqueries,
                          const DSort64Part* sparts, const DSortPart* rparts) {
  launch_sort<DocsetSort64>(stream, multi, a, squeries, rqueries, sparts, rparts);
}

// terms_compact_kernel's launch (termscount.hip): the occupied slots of every query's table packed into `out`
void launch_terms_compact(hipStream_t stream, const DTermsQuery* tqueries, DTermsState* states, const unsigned long long* tables, unsigned long long* out,
                          uint32_t n_queries, uint32_t out_cap);
// terms_compact64_kernel's launch (termscount64.hip)
void launch_terms_compact64(hipStream_t stream, const DTermsQuery* tqueries, DTermsState64* states, const unsigned long long* table_keys,
                            const uint32_t* table_counts, unsigned long long* out_codes, uint32_t* out_counts, uint32_t n_queries, uint32_t out_cap);

void launch_docset_terms_count(hipStream_t stream, bool multi, const FinalScoreArgs& a, const DTermsQuery* tqueries, const DRangeQuery* rqueries,
                               const DSortPart* sparts, const DSortPart* rparts, DTermsState* states, unsigned long long* tables, unsigned long long* out,
                               uint32_t n_queries, uint32_t out_cap) {
  if (a.n_items != 0) {
    const auto kernel = multi ? docset_terms_count_multi_kernel : docset_count_kernel<DocsetTerms32, false>;
    hipLaunchKernelGGL(kernel, dim3(a.n_items), dim3(kScanThreads), 0, stream, a.items, a.parts, a.queries, tqueries, rqueries, sparts, rparts, states, tables,
                       a.slice_sum, a.item_counts, a.item_hits);
  }
  launch_terms_compact(stream, tqueries, states, tables, out, n_queries, out_cap);
}

void launch_docset_terms_count64(hipStream_t stream, bool multi, const FinalScoreArgs& a, const DTermsQuery* tqueries, const DRangeQuery* rqueries,
                                 const DSort64Part* sparts, const DSortPart* rparts, DTermsState64* states, unsigned long long* table_keys,
                                 uint32_t* table_counts, unsigned long long* out_codes, uint32_t* out_counts, uint32_t n_queries, uint32_t out_cap) {
  if (a.n_items != 0) {
    const auto kernel = multi ? docset_terms_count64_kernel<true> : docset_terms_count64_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(a.n_items), dim3(kScanThreads), 0, stream, a.items, a.parts, a.queries, tqueries, rqueries, sparts, rparts, states,
                       table_keys, table_counts, a.slice_sum, a.item_counts, a.item_hits);
  }
  launch_terms_compact64(stream, tqueries, states, table_keys, table_counts, out_codes, out_counts, n_queries, out_cap);
}

void launch_docset_range_count(hipStream_t stream, bool wide, bool multi, const FinalScoreArgs& a, const DRangeCountQuery* cqueries,
                               const DRangeQuery* rqueries, const DSortPart* sparts, const DSortPart* rparts, const void* cuts, uint32_t* counters) {
  if (a.n_items == 0) return;
  const auto kernel = wide ? (multi ? docset_count_kernel<DocsetRanges<true>, true> : docset_count_kernel<DocsetRanges<true>, false>)
                           : (multi ? docset_count_kernel<DocsetRanges<false>, true> : docset_count_kernel<DocsetRanges<false>, false>);
  hipLaunchKernelGGL(kernel, dim3(a.n_items), dim3(kScanThreads), 0, stream, a.items, a.parts, a.queries, cqueries, rqueries, sparts, rparts, cuts, counters,
                     a.slice_sum, a.item_counts, a.item_hits);
}

}  // namespace nrtgpu
