// multimatch.hip -- the gfx950 kernel of multi-match queries: the two-level shapes the reference's multiMatchQuery builds
// (src/main/java/com/yelp/nrtsearch/server/query/QueryNodeMapper.java:429-528, .../multimatch/MatchCrossFieldsQuery.java:163-192).
//
//   bm25_multi_match_kernel   postings traversal + BM25Similarity GROUP BY GROUP: per doc the group's score from the group's
//                             clauses (plan.h: multi_match_group), folded into the doc's outer state (multi_match_fold); after
//                             the last group the final score and the hit test (multi_match_value), the item's top-k of FINAL scores
//
// A sibling of bm25_function_score_kernel (funcscore.hip), whose skeleton this is: nothing is pruned, theta bounds final keys only,
// the plan records are the scan's (DItem / DPart / DTerm / DQuery over the clauses as ONE SHOULD disjunction, so the parts cover
// every doc any clause matches), the item outputs are the scan's, expand_terms_kernel runs in front and merge_topk_kernel /
// slice_relation_kernel behind.  Fixed-point accumulators only (marker 0).  A clause's group rides in DTerm.tab_slot bits 24-28.
//
// Work decomposition: one workgroup of kMmWaves waves per item; the item's sub-tiles in ROUNDS of one sub-tile per wave.  Per
// sub-tile a wave goes group by group: it streams the postings of the group's clauses into its INNER accumulators -- per doc a u64
// fixed-point sum with the number of matching clauses above bit 56 (the sum stays below 2^53), and, for DisjunctionMax groups, a
// u32 maximum of the clause scores' float bits (a clause's shifted fixed-point value IS its float score, and positive floats order
// like their bits) -- then sweeps them: group score, fold, clear.  The OUTER state of a doc (double sum, float maximum, group
// count) lives in REGISTERS: in every sweep lane l owns the same 16 slots l + 64 j, and the sweeps are fully unrolled.  The groups
// are folded in group order, so the double sum over the groups is the same sequence of additions for every doc on every run.
// After the last group the final sweep leaves the candidate keys in place of the sums; from there on it is funcscore.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bm25_common.hiph"

namespace nrtgpu {

struct MmSmem {
  uint64_t sum[kMmWaves][kTileDocs];    // per wave: the current group's fixed-point sums | clause count << 56, then its candidate keys (0: none)
  uint32_t best[kMmWaves][kTileDocs];   // per wave: float bits of the current group's best clause score (kGroupsSumOfMax)
  uint64_t cand[kMmCandCap];            // candidate keys of the item, unordered
  float    cache[kLdsCaches][256];      // BM25 normInverse tables of the query's fields
  TopkScratch sc;
  uint32_t wcount[2][kMmWaves];         // candidates each wave holds in its sub-tile, by round parity
  uint32_t slot_hits[kSliceSlots];      // hits of this item per searcher slice it touches (plan.h: DPart.slice)
  uint32_t slot_slice[kSliceSlots];
};
static_assert(sizeof(MmSmem) <= 160 * 1024, "the workgroup owns one CU's 160 KiB LDS");

constexpr int kMmSlots = kTileDocs / 64;   // accumulator slots per lane
constexpr uint64_t kMmSumMask = (1ull << kMsmCountShift) - 1ull;

// The wave's candidate keys (left in its sub-tile by the final sweep) into cand[pos ...], slot-major; the sub-tile is all markers after.
__device__ __forceinline__ void mm_push_candidates(MmSmem& s, uint64_t* acc, uint32_t lane, uint32_t pos) {
#pragma unroll 4
  for (int j = 0; j < kMmSlots; ++j) {
    const uint32_t i = lane + 64u * (uint32_t)j;
    const uint64_t key = acc[i];
    const unsigned long long b = __ballot(key != 0ull);
    if (key != 0ull) {
      const uint32_t at = pos + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
      if (at < (uint32_t)kMmCandCap) s.cand[at] = key;   // (always true: the caller made room)
      acc[i] = 0ull;
    }
    pos += (uint32_t)__popcll(b);
  }
}

__global__ __launch_bounds__(kMmThreads, kMmWaves / 4)
void bm25_multi_match_kernel(const DItem* __restrict__ items, const DPart* __restrict__ parts, const DTerm* __restrict__ terms,
                             const DQuery* __restrict__ queries, const float* __restrict__ caches,
                             const DGroupQuery* __restrict__ gqueries, unsigned long long* __restrict__ theta_g,
                             uint32_t* __restrict__ slice_sum, uint64_t* __restrict__ item_keys, uint32_t* __restrict__ item_counts,
                             uint64_t* __restrict__ item_hits, uint32_t k_stride) {
  __shared__ MmSmem s;
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), lane = tid & 63u;
  uint64_t* const acc = &s.sum[wave][0];
  uint32_t* const best = &s.best[wave][0];
  const DItem* const item = items + blockIdx.x;
  const uint32_t query = item->query, part_begin = item->part_begin, n_parts = item->n_parts;
  const int fx_E = item->fx_E;
  const DQuery* const q = queries + query;
  const uint32_t k = min(q->k, (uint32_t)kMaxK);
  const DGroupQuery* const gq = gqueries + query;
  const uint32_t n_groups = min(gq->n_groups, (uint32_t)kMaxGroups);
  const bool want_best = gq->shape == kGroupsSumOfMax;
  const bool multi_item = q->n_items > 1;
  unsigned long long* const my_theta_g = theta_g + query;
  // searchAfter compares FINAL scores: a hit at or above after_key was collected on an earlier page (it still counts)
  const uint64_t after_key = q->has_after ? pack_key(q->after_score, (uint32_t)q->after_doc) : ~0ull;

  // ---- prologue: markers, normInverse tables, slice counters
  for (int j = 0; j < kMmSlots; ++j) {
    acc[lane + 64u * (uint32_t)j] = 0ull;
    best[lane + 64u * (uint32_t)j] = 0u;
  }
  {
    const uint32_t n_lds = min(item->n_caches, (uint32_t)kLdsCaches) * 256u;
    const uint32_t cache_off = item->cache_off;
    for (uint32_t i = tid; i < n_lds; i += kMmThreads) (&s.cache[0][0])[i] = caches[cache_off + i];
  }
  if (tid < (uint32_t)kSliceSlots) s.slot_hits[tid] = s.slot_slice[tid] = 0u;
  __syncthreads();

  uint32_t total_tiles = 0;   // sub-tiles of the item: its parts' tiles form one sequence (DPart.tile_offset)
  if (n_parts != 0) {
    const DPart* lp = parts + part_begin + n_parts - 1u;
    total_tiles = lp->tile_offset + (lp->tile_end - lp->tile_begin);
  }
  uint64_t theta = 0;   // uniform: the k-th best FINAL key known (this item's compactions, the query's other items)
  uint32_t cnt = 0;     // uniform: keys in s.cand
  uint32_t pi = 0;      // the part of the wave's sub-tile (indices only grow)
  uint32_t par = 0;

  for (uint32_t g0 = 0; g0 < total_tiles; g0 += (uint32_t)kMmWaves, par ^= 1u) {
    if (multi_item) {   // what the query's other items have published (a bound on final keys: at least k docs of the query exceed it)
      const uint64_t t = __hip_atomic_load(my_theta_g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      theta = t > theta ? t : theta;
    }
    const uint32_t gt = g0 + wave;
    uint32_t n_cand = 0;   // wave-uniform
    if (gt < total_tiles) {
      const DPart* part = parts + part_begin + pi;
      while (pi + 1u < n_parts && gt >= part->tile_offset + (part->tile_end - part->tile_begin)) {
        ++pi;
        ++part;
      }
      const uint32_t tile = gt - part->tile_offset + part->tile_begin;
      const uint32_t base = tile * (uint32_t)kTileDocs;
      const uint32_t max_doc = part->max_doc;
      const uint32_t tile_len = base < max_doc ? min((uint32_t)kTileDocs, max_doc - base) : 0u;
      const uint32_t gdoc0 = (uint32_t)(part->doc_base + (int32_t)base);

      // Lane l looks up the posting range and the group of clause l (one memory round trip for all clauses of all groups).
      const uint32_t n_terms = min(part->n_terms, (uint32_t)kMaxTerms);
      const DTerm* const part_terms = terms + part->term_begin;
      uint32_t my_lo = 0, my_hi = 0, my_group = 0xFFFFFFFFu;
      if (lane < n_terms) {
        const DTerm* mt = part_terms + lane;
        const gu32_ptr cells = (gu32_ptr)mt->cell_off;
        my_group = (mt->tab_slot >> kTabSlotGroupShift) & kTabSlotGroupMask;
        if (mt->docids != nullptr) {
          const uint32_t c = tile >> mt->shift;
          my_lo = cells[c];
          my_hi = cells[c + 1u];
        }
      }

      MmOuter outer[kMmSlots];   // registers: every loop over j below is fully unrolled
#pragma unroll
      for (int j = 0; j < kMmSlots; ++j) outer[j] = MmOuter{0.0, 0.0f, 0u};

      for (uint32_t g = 0; g < n_groups; ++g) {
        // ---- (1) accumulate: the postings of group g's clauses in the sub-tile; a group without any is skipped whole
        unsigned long long todo = __ballot(my_group == g && my_lo < my_hi);
        if (todo == 0ull) continue;   // uniform
        while (todo != 0ull) {
          const uint32_t t = (uint32_t)__ffsll((long long)todo) - 1u;
          todo &= todo - 1ull;
          const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)my_lo, (int)t), hi = (uint32_t)__builtin_amdgcn_readlane((int)my_hi, (int)t);
          const DTerm* T = part_terms + t;
          const uint64_t start = T->start;
          const gu32_ptr docids = (gu32_ptr)T->docids + start, codes = (gu32_ptr)T->fnorm + start;
          const float w = T->weight;
          const int fx_scale = T->fx_scale;
          const uint32_t fx_shift = T->fx_shift;
          const float* const cache = &s.cache[min(T->cache_slot, (uint32_t)kLdsCaches - 1u)][0];
          for (uint32_t p0 = lo; p0 < hi; p0 += 256u) {
            uint32_t doc[4], code[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const uint32_t p = p0 + 64u * (uint32_t)u + lane;
              const bool in = p < hi;
              doc[u] = in ? docids[p] : 0xFFFFFFFFu;   // (past the range: a doc outside every sub-tile)
              code[u] = in ? codes[p] : 0u;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const uint32_t off = doc[u] - base;   // a coarse cell's postings may lie outside the sub-tile (unsigned: below it wraps)
              // the score code (plan.h: DTerm.fnorm), as funcscore.hip reads it; both forms carry the "doc is deleted" mark
              const uint32_t cw = code[u];
              const bool esc = (cw >> 31) != 0u;
              const uint32_t f = esc ? ((cw >> 8) & 0x3FFFFFu) : ((cw >> 9) & 15u);
              const bool dead = esc ? ((cw >> 30) & 1u) != 0u : (cw >> 20) != 0u;
              const uint32_t nb = esc ? (cw & 255u) : ((cw >> 2) & 127u);
              if (off < tile_len && !dead) {
                const float sc = bm25_score(w, (float)(int32_t)f, cache[nb]);
                const uint32_t val = score_value<true>(sc, fx_scale);
                atomicAdd((unsigned long long*)&acc[off], ((unsigned long long)val << fx_shift) + (1ull << kMsmCountShift));
                if (want_best) atomicMax(&best[off], __float_as_uint(sc));
              }
            }
          }
        }

        // ---- (2) group sweep: the group's score of every doc it touched, folded into the doc's outer state; markers again after
#pragma unroll
        for (int j = 0; j < kMmSlots; ++j) {
          const uint32_t i = lane + 64u * (uint32_t)j;
          const uint64_t a = acc[i];
          if (a != 0ull) {
            const double sum = ldexp((double)(a & kMmSumMask), -fx_E);   // < 2^53: exact conversion, exact scaling
            float group_score;
            if (multi_match_group(*gq, g, sum, __uint_as_float(best[i]), (uint32_t)(a >> kMsmCountShift), &group_score))
              multi_match_fold(outer[j], group_score);
            acc[i] = 0ull;
            if (want_best) best[i] = 0u;
          }
        }
      }

      // ---- (3) final sweep: slot lane + 64 j is doc base + 64 j + lane, i.e. bit `lane` of word j of the sub-tile's mask words
      const NRT_GLOBAL uint64_t* const live_bits = (const NRT_GLOBAL uint64_t*)part->live_bits;
      const uint32_t word0 = base >> 6;
      uint32_t wave_hits = 0;
#pragma unroll
      for (int j = 0; j < kMmSlots; ++j) {
        const uint32_t i = lane + 64u * (uint32_t)j;
        uint64_t key = 0;
        if (64u * (uint32_t)j < tile_len) {   // uniform: the word below exists
          bool ok = outer[j].n != 0u;
          if (live_bits != nullptr) ok = ok && ((live_bits[word0 + (uint32_t)j] >> lane) & 1ull) != 0ull;
          bool hit = false;
          if (ok) {
            const float final_score = multi_match_value(*gq, outer[j], &hit);
            if (hit) {
              key = pack_key(final_score, gdoc0 + i);
              if (!(key > theta && key < after_key)) key = 0ull;
            }
          }
          wave_hits += (uint32_t)__popcll(__ballot(hit));   // totalHits counts every hit, also those skipped by `after`
        }
        acc[i] = key;
        n_cand += (uint32_t)__popcll(__ballot(key != 0ull));
      }
      if (lane == 0) {
        const uint32_t slot = min(part->slice >> 24, (uint32_t)kSliceSlots - 1u);
        s.slot_slice[slot] = part->slice & 0xFFFFFFu;
        if (wave_hits) atomicAdd(&s.slot_hits[slot], wave_hits);
      }
    }
    if (lane == 0) s.wcount[par][wave] = n_cand;
    __syncthreads();

    // ---- (4) the round's candidates into the shared buffer
    uint32_t tot = 0, before = 0;
#pragma unroll
    for (uint32_t w2 = 0; w2 < (uint32_t)kMmWaves; ++w2) {
      const uint32_t c = s.wcount[par][w2];
      tot += c;
      before += w2 < wave ? c : 0u;
    }
    if (cnt + tot <= (uint32_t)kMmCandCap) {   // uniform
      mm_push_candidates(s, acc, lane, cnt + before);
      cnt += tot;
    } else {
      for (uint32_t w2 = 0; w2 < (uint32_t)kMmWaves; ++w2) {
        const uint32_t c = s.wcount[par][w2];
        if (cnt + c > (uint32_t)kMmCandCap) {   // uniform; cnt > k here (kMmCandCap >= kMaxK + kTileDocs)
          __syncthreads();   // the keys appended so far are in place
          uint64_t thr = 0;
          cnt = topk_compact<kMmThreads, kMmCandCap>(s.cand, cnt, k, &s.sc, &thr);
          if (thr > theta) theta = thr;
          if (tid == 0) atomicMax(my_theta_g, (unsigned long long)thr);   // LazyMaxScoreAccumulator.accumulate analogue
        }
        if (wave == w2) mm_push_candidates(s, acc, lane, cnt);
        cnt += c;
      }
    }
  }

  // ---- epilogue: the item's final top-k, its hits per slice
  __syncthreads();
  if (cnt > k) {
    uint64_t thr = 0;
    cnt = topk_compact<kMmThreads, kMmCandCap>(s.cand, cnt, k, &s.sc, &thr);
  }
  __syncthreads();
  uint64_t* out = item_keys + (size_t)blockIdx.x * k_stride;
  const uint32_t n = min(cnt, k_stride);
  for (uint32_t i = tid; i < n; i += kMmThreads) out[i] = s.cand[i];
  if (tid == 0) {
    item_counts[blockIdx.x] = n;
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

void launch_bm25_multi_match(hipStream_t stream, uint32_t n_items, const DItem* items, const DPart* parts, const DTerm* terms,
                             const DQuery* queries, const float* caches, const DGroupQuery* gqueries, unsigned long long* theta_g,
                             uint32_t* slice_sum, uint64_t* item_keys, uint32_t* item_counts, uint64_t* item_hits, uint32_t k_stride) {
  if (n_items == 0) return;
  hipLaunchKernelGGL(bm25_multi_match_kernel, dim3(n_items), dim3(kMmThreads), 0, stream, items, parts, terms, queries, caches,
                     gqueries, theta_g, slice_sum, item_keys, item_counts, item_hits, k_stride);
}

}  // namespace nrtgpu
