// knnclauses.hip -- the gfx950 kernel of a text query beside knn clauses (include/nrtgpu.h: nrtgpu_search_text_knn_batch): the
// request's `query` and its resolved `knn` lists as SHOULD clauses of ONE BooleanQuery -- the reference resolves every knn query to
// a doc-and-score query over its top k and ORs those into the main query (SearchRequestProcessor.java:267-296,
// KnnUtils.resolveKnnQueryAndBoost).
//
//   bm25_text_knn_kernel   postings traversal + BM25Similarity + disjunction sum, then the TAG PASS over the listed docs of the
//                          sub-tile (plan.h: text_knn_value), then the item's top-k of FINAL scores
//
// bm25_function_score_kernel's structure on finalscore.hiph -- kScanWaves waves, the same LDS, kFsCandCap -- with one pass added
// between (1) accumulate and (2) sweep.  The host stages, per (query, leaf), the listed docs with duplicates across lists already
// merged: sorted leaf-local docids and their knn_sum doubles; per part a DKnnPart (plan.h) names the part's entries.
//
// The tag pass: the wave takes the entries that fall in its sub-tile, 64 per step.  Per entry it checks the leaf's liveDocs, reads
// the slot's fixed-point sum and the slot's accept bit, calls text_knn_value and writes back a TAGGED slot (plan.h: kKnnTag | the
// final float).  The sweep takes a tagged slot as a hit with that score, whatever the sum and the accept bit were; an untagged
// slot takes the function-score kernel's path (no functions).  A listed doc that is not live leaves its slot as it is -- and its
// postings never reached it or its accept bit is clear, so it is no hit.
//
// The wave does not search a list per sub-tile.  Its sub-tiles only grow, so it keeps a CURSOR into the part's entries: one binary
// search when it enters a part, then one coalesced load of the next 64 docids per sub-tile, issued beside the clause-range lookup --
// an empty sub-tile costs no extra dependent round trip.  Entries below the sub-tile (other waves' docs) are passed over in the
// same 64; only when all 64 lie below it does the wave search again.  A part without entries skips all of it by a uniform branch.
//
// The slot a lane tags was written by other lanes' ds_add_u64 of the SAME wave before: LDS operations of a wave complete in order,
// the pattern the sweep already relies on.  All global writes go through the skeleton.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "finalscore.hiph"

namespace nrtgpu {

struct TextKnnSmem {
  uint64_t acc[kScanWaves][kTileDocs];   // per wave: fixed-point sums of its sub-tile, tagged finals among them, then its candidate keys (0: none)
  FinalSmem<kScanWaves, kFsCandCap> t;
};
static_assert(sizeof(TextKnnSmem) <= 160 * 1024, "the workgroup owns one CU's 160 KiB LDS");

// first entry of docs[lo, hi) (ascending) that is >= doc; every lane asks the same question
__device__ __forceinline__ uint32_t knn_first_at_or_above(const uint32_t* __restrict__ docs, uint32_t lo, uint32_t hi, uint32_t doc) {
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (docs[mid] < doc) lo = mid + 1u;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kScanThreads, kScanWaves / 4)
void bm25_text_knn_kernel(const DItem* __restrict__ items, const DPart* __restrict__ parts, const DTerm* __restrict__ terms,
                          const DQuery* __restrict__ queries, const float* __restrict__ caches,
                          const DKnnPart* __restrict__ kparts, const uint32_t* __restrict__ kdocs, const double* __restrict__ ksums,
                          unsigned long long* __restrict__ theta_g, uint32_t* __restrict__ slice_sum, uint32_t* __restrict__ slice_past,
                          uint64_t* __restrict__ item_keys, uint32_t* __restrict__ item_counts, uint64_t* __restrict__ item_hits,
                          uint32_t k_stride) {
  __shared__ TextKnnSmem s;
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), lane = tid & 63u;
  uint64_t* const acc = &s.acc[wave][0];
  const DItem* const item = items + blockIdx.x;
  const uint32_t query = item->query, part_begin = item->part_begin, n_parts = item->n_parts;
  const int fx_E = item->fx_E;
  const DQuery* const q = queries + query;
  const uint32_t k = min(q->k, (uint32_t)kMaxK);
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
  uint32_t cur = 0, cur_pi = 0xFFFFFFFFu;   // uniform: the wave's cursor into the entries of part cur_pi

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

      // ---- the part's listed docs: the cursor (one search per part), then the next 64 docids -- in flight beside the lookup below
      const DKnnPart* const kp = kparts + part_begin + pi;
      const uint32_t e_end = kp->entry_end;
      const bool listed = e_end > kp->entry_begin;   // uniform
      uint32_t my_doc = 0xFFFFFFFFu;
      if (listed) {
        if (cur_pi != pi) {
          cur = knn_first_at_or_above(kdocs, kp->entry_begin, e_end, base);
          cur_pi = pi;
        }
        if (cur + lane < e_end) my_doc = kdocs[cur + lane];
      }

      // ---- (1) accumulate: every clause's postings of the sub-tile (as bm25_function_score_kernel)
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

      const NRT_GLOBAL uint64_t* const accept_bits = (const NRT_GLOBAL uint64_t*)part->live_bits;   // the query's accept set on the leaf

      // ---- (1b) tag: the entries inside the sub-tile, 64 per step
      if (listed) {
        const NRT_GLOBAL uint64_t* const leaf_live = (const NRT_GLOBAL uint64_t*)kp->live_bits;
        const uint32_t nested = kp->nested;
        const uint32_t limit = base + tile_len;   // (entries are docs of the leaf: below max_doc)
        while (true) {   // uniform
          const uint32_t off = my_doc - base;   // below the sub-tile: wraps
          const bool in = off < tile_len;
          if (in) {
            const uint32_t wi = my_doc >> 6, bit = my_doc & 63u;
            const bool live = leaf_live == nullptr || ((leaf_live[wi] >> bit) & 1ull) != 0ull;
            if (live) {
              const uint64_t v = acc[off];
              const bool text = v != 0ull && (accept_bits == nullptr || ((accept_bits[wi] >> bit) & 1ull) != 0ull);
              const float final_score = text_knn_value(nested, text, v, fx_E, ksums[cur + lane]);
              acc[off] = kKnnTag | (uint64_t)__float_as_uint(final_score);   // (no doc twice among a pair's entries: the slot is this lane's)
            }
          }
          const uint32_t n_passed = (uint32_t)__popcll(__ballot(my_doc < limit));   // below or inside: done with
          cur += n_passed;
          if (n_passed < 64u) break;
          if (__ballot(in) == 0ull) cur = knn_first_at_or_above(kdocs, cur, e_end, base);   // all 64 were other waves' docs
          my_doc = cur + lane < e_end ? kdocs[cur + lane] : 0xFFFFFFFFu;
        }
      }

      // ---- (2) sweep: slot lane + 64 j is doc base + 64 j + lane, i.e. bit `lane` of word j of the sub-tile's mask words
      const uint32_t word0 = base >> 6;
      uint32_t wave_hits = 0, wave_past = 0;
#pragma unroll 2
      for (int j = 0; j < kFinalSlots; ++j) {
        const uint32_t i = lane + 64u * (uint32_t)j;
        const uint64_t v = acc[i];
        uint64_t key = 0;
        if (64u * (uint32_t)j < tile_len) {   // uniform: the words below exist
          const bool tagged = (v & kKnnTag) != 0ull;
          bool ok = v != 0ull;
          if (accept_bits != nullptr) ok = ok && (tagged || ((accept_bits[word0 + (uint32_t)j] >> lane) & 1ull) != 0ull);
          key = final_candidate_key(ok, gdoc0 + i, theta, after_key, wave_hits, wave_past, [tagged, v, fx_E](bool* hit) {
            *hit = true;
            return tagged ? __uint_as_float((uint32_t)v) : acc_score<true>(v, fx_E);
          });
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

void launch_bm25_text_knn(hipStream_t stream, const FinalScoreArgs& a, const DKnnPart* kparts, const uint32_t* kdocs, const double* ksums) {
  if (a.n_items == 0) return;
  hipLaunchKernelGGL(bm25_text_knn_kernel, dim3(a.n_items), dim3(kScanThreads), 0, stream, a.items, a.parts, a.terms, a.queries, a.caches,
                     kparts, kdocs, ksums, a.theta_g, a.slice_sum, a.slice_past, a.item_keys, a.item_counts, a.item_hits, a.k_stride);
}

}  // namespace nrtgpu
