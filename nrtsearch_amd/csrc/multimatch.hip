// multimatch.hip -- the gfx950 kernel of multi-match queries: the two-level shapes the reference's multiMatchQuery builds
// (src/main/java/com/yelp/nrtsearch/server/query/QueryNodeMapper.java:429-528, .../multimatch/MatchCrossFieldsQuery.java:163-192).
//
//   bm25_multi_match_kernel   postings traversal + BM25Similarity GROUP BY GROUP: per doc the group's score from the group's
//                             clauses (plan.h: multi_match_group), folded into the doc's outer state (multi_match_fold); after
//                             the last group the final score and the hit test (multi_match_value), the item's top-k of FINAL scores
//   bm25_multi_match_function_score_kernel
//                             the same body (multi_match_body<true>) for a function score over such a query: behind multi_match_value
//                             the final sweep puts function_score_value over the doc's function sets, as bm25_function_score_kernel's
//
// Like bm25_function_score_kernel (funcscore.hip) nothing is pruned and theta bounds final keys only; the plan records are the
// scan's (DItem / DPart / DTerm / DQuery over the clauses as ONE SHOULD disjunction, so the parts cover every doc any clause
// matches), the item outputs are the scan's, expand_terms_kernel runs in front and merge_topk_kernel / slice_relation_kernel
// behind.  Fixed-point accumulators only (marker 0).  A clause's group rides in DTerm.tab_slot bits 24-28.  What the two kernels
// share as code is finalscore.hiph.
//
// Work decomposition: one workgroup of kMmWaves waves per item; the item's sub-tiles in ROUNDS of one sub-tile per wave.  Per
// sub-tile a wave goes group by group: it streams the postings of the group's clauses into its INNER accumulators -- per doc a u64
// fixed-point sum with the number of matching clauses above bit 56 (the sum stays below 2^53), and, for DisjunctionMax groups, a
// u32 maximum of the clause scores' float bits (a clause's shifted fixed-point value IS its float score, and positive floats order
// like their bits) -- then sweeps them: group score, fold, clear.  The OUTER state of a doc (double sum, float maximum, group
// count) lives in REGISTERS: in every sweep lane l owns the same 16 slots l + 64 j, and the sweeps are fully unrolled.  The groups
// are folded in group order, so the double sum over the groups is the same sequence of additions for every doc on every run.
// After the last group the final sweep leaves the candidate keys in place of the sums; the rounds' candidates then meet in the
// shared buffer as in bm25_function_score_kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "finalscore.hiph"

namespace nrtgpu {

struct MmSmem {
  uint64_t sum[kMmWaves][kTileDocs];    // per wave: the current group's fixed-point sums | clause count << 56, then its candidate keys (0: none)
  uint32_t best[kMmWaves][kTileDocs];   // per wave: float bits of the current group's best clause score (kGroupsSumOfMax)
  FinalSmem<kMmWaves, kMmCandCap> t;
};
static_assert(sizeof(MmSmem) <= 160 * 1024, "the workgroup owns one CU's 160 KiB LDS");

constexpr uint64_t kMmSumMask = (1ull << kMsmCountShift) - 1ull;

// The body of both kernels.  FUNCTIONS: the final sweep also reads the doc's function sets and puts function_score_value behind
// multi_match_value (fqueries: one DFuncQuery per query, fmasks: one DFuncMasks per part); without it neither pointer is read and
// the instantiation is bm25_multi_match_kernel as it was written out before.
template <bool FUNCTIONS>
__device__ __forceinline__ void multi_match_body(const DItem* __restrict__ items, const DPart* __restrict__ parts,
                                                 const DTerm* __restrict__ terms, const DQuery* __restrict__ queries,
                                                 const float* __restrict__ caches, const DGroupQuery* __restrict__ gqueries,
                                                 const DFuncQuery* __restrict__ fqueries, const DFuncMasks* __restrict__ fmasks,
                                                 unsigned long long* __restrict__ theta_g, uint32_t* __restrict__ slice_sum, uint32_t* __restrict__ slice_past,
                                                 uint64_t* __restrict__ item_keys, uint32_t* __restrict__ item_counts,
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
  // The function record in LDS (this instantiation only): function_score_value reads it per doc slot inside the unrolled sweep,
  // and out of global memory every one of those reads was a dependent scalar round trip of its own.
  const DFuncQuery* fq = nullptr;
  uint32_t n_functions = 0u;
  if constexpr (FUNCTIONS) {
    __shared__ DFuncQuery s_fq;
    static_assert(sizeof(DFuncQuery) == 16 * sizeof(uint32_t), "copied below as 16 words");
    if (tid < 16u) ((uint32_t*)&s_fq)[tid] = ((const uint32_t*)(fqueries + query))[tid];   // (final_prologue ends with the barrier)
    fq = &s_fq;
    n_functions = min((uint32_t)fqueries[query].n_functions, (uint32_t)kMaxFunctions);
  }
  const bool multi_item = q->n_items > 1;
  unsigned long long* const my_theta_g = theta_g + query;
  // searchAfter compares FINAL scores: a hit at or above after_key was collected on an earlier page (it still counts)
  const uint64_t after_key = q->has_after ? pack_key(q->after_score, (uint32_t)q->after_doc) : ~0ull;

  final_prologue(s.t, acc, best, item, caches, tid, lane);

  const uint32_t total_tiles = final_total_tiles(parts, part_begin, n_parts);
  uint64_t theta = 0;   // uniform: the k-th best FINAL key known (this item's compactions, the query's other items)
  uint32_t cnt = 0;     // uniform: keys in s.t.cand
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
      const FinalTile tl = final_tile(parts, part_begin, n_parts, gt, pi);
      const DPart* const part = tl.part;
      const uint32_t tile = tl.tile, base = tl.base, tile_len = tl.tile_len, gdoc0 = tl.gdoc0;

      // Lane l looks up the posting range and the group of clause l (one memory round trip for all clauses of all groups).
      const uint32_t n_terms = min(part->n_terms, (uint32_t)kMaxTerms);
      const DTerm* const part_terms = terms + part->term_begin;
      uint32_t my_lo = 0, my_hi = 0, my_group = 0xFFFFFFFFu;
      if (lane < n_terms) {
        my_group = (part_terms[lane].tab_slot >> kTabSlotGroupShift) & kTabSlotGroupMask;
        final_clause_range(part_terms + lane, tile, my_lo, my_hi);
      }

      // The sub-tile's function sets, in flight while the groups are streamed: lane l holds word (l & 15) of the sub-tile's
      // 16 mask words of function (l >> 4) in fw0 and of function (l >> 4) + 4 in fw1 (nullptr: every doc); the final sweep
      // fetches a word from its lane.  One vector load per lane instead of a dependent scalar load per function and word.
      uint64_t fw0 = 0ull, fw1 = 0ull;
      if constexpr (FUNCTIONS) {
        const DFuncMasks* const fm = fmasks + part_begin + pi;
        const uint32_t wj = lane & 15u, f0 = lane >> 4;
        if (64u * wj < tile_len) {   // the word exists
          if (f0 < n_functions) {
            const NRT_GLOBAL uint64_t* const m = (const NRT_GLOBAL uint64_t*)fm->mask[f0];
            fw0 = m != nullptr ? m[(base >> 6) + wj] : ~0ull;
          }
          if (f0 + 4u < n_functions) {
            const NRT_GLOBAL uint64_t* const m = (const NRT_GLOBAL uint64_t*)fm->mask[f0 + 4u];
            fw1 = m != nullptr ? m[(base >> 6) + wj] : ~0ull;
          }
        }
      }

      MmOuter outer[kFinalSlots];   // registers: every loop over j below is fully unrolled
#pragma unroll
      for (int j = 0; j < kFinalSlots; ++j) outer[j] = MmOuter{0.0, 0.0f, 0u};

      for (uint32_t g = 0; g < n_groups; ++g) {
        // ---- (1) accumulate: the postings of group g's clauses in the sub-tile; a group without any is skipped whole
        unsigned long long todo = __ballot(my_group == g && my_lo < my_hi);
        if (todo == 0ull) continue;   // uniform
        while (todo != 0ull) {
          const uint32_t t = (uint32_t)__ffsll((long long)todo) - 1u;
          todo &= todo - 1ull;
          const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)my_lo, (int)t), hi = (uint32_t)__builtin_amdgcn_readlane((int)my_hi, (int)t);
          // (a clause's shifted fixed-point value IS its float score)
          final_stream_clause(part_terms + t, lo, hi, base, tile_len, lane, s.t.cache,
                              [acc, best, want_best](uint32_t off, float sc, unsigned long long v) {
                                atomicAdd((unsigned long long*)&acc[off], v + (1ull << kMsmCountShift));
                                if (want_best) atomicMax(&best[off], __float_as_uint(sc));
                              });
        }

        // ---- (2) group sweep: the group's score of every doc it touched, folded into the doc's outer state; markers again after
#pragma unroll
        for (int j = 0; j < kFinalSlots; ++j) {
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
      uint32_t wave_hits = 0, wave_past = 0;
#pragma unroll
      for (int j = 0; j < kFinalSlots; ++j) {
        const uint32_t i = lane + 64u * (uint32_t)j;
        uint64_t key = 0;
        if (64u * (uint32_t)j < tile_len) {   // uniform: the words below exist
          bool ok = outer[j].n != 0u;
          if (live_bits != nullptr) ok = ok && ((live_bits[word0 + (uint32_t)j] >> lane) & 1ull) != 0ull;
          const MmOuter& o = outer[j];
          if constexpr (FUNCTIONS) {
            uint32_t matched = 0;   // word j of function fi sits in lane 16 (fi & 3) + j: bit `lane` of it is this doc
#pragma unroll
            for (uint32_t fi = 0; fi < (uint32_t)kMaxFunctions; ++fi) {
              if (fi >= n_functions) break;   // uniform
              const uint64_t w = fi < 4u ? fw0 : fw1;
              const int src = (int)(16u * (fi & 3u)) + j;
              const uint64_t mw = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)w, src) |
                                  ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(w >> 32), src) << 32);
              matched |= (uint32_t)((mw >> lane) & 1ull) << fi;
            }
            // a doc the groups reject is no hit whatever the functions say; else the function score's own hit test decides
            key = final_candidate_key(ok, gdoc0 + i, theta, after_key, wave_hits, wave_past, [gq, fq, matched, &o](bool* hit) {
              const float inner = multi_match_value(*gq, o, hit);
              return *hit ? function_score_value(*fq, matched, inner, hit) : inner;
            });
          } else {
            key = final_candidate_key(ok, gdoc0 + i, theta, after_key, wave_hits, wave_past, [gq, &o](bool* hit) { return multi_match_value(*gq, o, hit); });
          }
        }
        acc[i] = key;
        n_cand += (uint32_t)__popcll(__ballot(key != 0ull));
      }
      final_count_slice(s.t, part, lane, wave_hits, wave_past);
    }
    if (lane == 0) s.t.wcount[par][wave] = n_cand;
    __syncthreads();

    // ---- (4) the round's candidates into the shared buffer
    uint32_t tot = 0, before = 0;
#pragma unroll
    for (uint32_t w2 = 0; w2 < (uint32_t)kMmWaves; ++w2) {
      const uint32_t c = s.t.wcount[par][w2];
      tot += c;
      before += w2 < wave ? c : 0u;
    }
    if (cnt + tot <= (uint32_t)kMmCandCap) {   // uniform
      final_push_candidates(s.t, acc, lane, cnt + before);
      cnt += tot;
    } else {
      for (uint32_t w2 = 0; w2 < (uint32_t)kMmWaves; ++w2) {
        const uint32_t c = s.t.wcount[par][w2];
        if (cnt + c > (uint32_t)kMmCandCap) {   // uniform; cnt > k here (kMmCandCap >= kMaxK + kTileDocs)
          __syncthreads();   // the keys appended so far are in place
          uint64_t thr = 0;
          cnt = topk_compact<kMmThreads, kMmCandCap>(s.t.cand, cnt, k, &s.t.sc, &thr);
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

__global__ __launch_bounds__(kMmThreads, kMmWaves / 4)
void bm25_multi_match_kernel(const DItem* __restrict__ items, const DPart* __restrict__ parts, const DTerm* __restrict__ terms,
                             const DQuery* __restrict__ queries, const float* __restrict__ caches,
                             const DGroupQuery* __restrict__ gqueries, unsigned long long* __restrict__ theta_g,
                             uint32_t* __restrict__ slice_sum, uint32_t* __restrict__ slice_past, uint64_t* __restrict__ item_keys, uint32_t* __restrict__ item_counts,
                             uint64_t* __restrict__ item_hits, uint32_t k_stride) {
  multi_match_body<false>(items, parts, terms, queries, caches, gqueries, nullptr, nullptr, theta_g, slice_sum, slice_past, item_keys, item_counts,
                          item_hits, k_stride);
}

__global__ __launch_bounds__(kMmThreads, kMmWaves / 4)
void bm25_multi_match_function_score_kernel(const DItem* __restrict__ items, const DPart* __restrict__ parts, const DTerm* __restrict__ terms,
                                            const DQuery* __restrict__ queries, const float* __restrict__ caches,
                                            const DGroupQuery* __restrict__ gqueries, const DFuncQuery* __restrict__ fqueries,
                                            const DFuncMasks* __restrict__ fmasks, unsigned long long* __restrict__ theta_g,
                                            uint32_t* __restrict__ slice_sum, uint32_t* __restrict__ slice_past, uint64_t* __restrict__ item_keys,
                                            uint32_t* __restrict__ item_counts, uint64_t* __restrict__ item_hits, uint32_t k_stride) {
  multi_match_body<true>(items, parts, terms, queries, caches, gqueries, fqueries, fmasks, theta_g, slice_sum, slice_past, item_keys, item_counts,
                         item_hits, k_stride);
}

void launch_bm25_multi_match(hipStream_t stream, const FinalScoreArgs& a, const DGroupQuery* gqueries) {
  if (a.n_items == 0) return;
  hipLaunchKernelGGL(bm25_multi_match_kernel, dim3(a.n_items), dim3(kMmThreads), 0, stream, a.items, a.parts, a.terms, a.queries, a.caches,
                     gqueries, a.theta_g, a.slice_sum, a.slice_past, a.item_keys, a.item_counts, a.item_hits, a.k_stride);
}

void launch_bm25_multi_match_function_score(hipStream_t stream, const FinalScoreArgs& a, const DGroupQuery* gqueries, const DFuncQuery* fqueries,
                                            const DFuncMasks* fmasks) {
  if (a.n_items == 0) return;
  hipLaunchKernelGGL(bm25_multi_match_function_score_kernel, dim3(a.n_items), dim3(kMmThreads), 0, stream, a.items, a.parts, a.terms, a.queries,
                     a.caches, gqueries, fqueries, fmasks, a.theta_g, a.slice_sum, a.slice_past, a.item_keys, a.item_counts, a.item_hits, a.k_stride);
}

}  // namespace nrtgpu
