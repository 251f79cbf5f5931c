// funcscore.hip -- the gfx950 kernel of function-score queries (MultiFunctionScoreQuery with weight functions over a BM25
// disjunction; the reference's src/main/java/com/yelp/nrtsearch/server/query/multifunction/MultiFunctionScoreQuery.java).
//
//   bm25_function_score_kernel   postings traversal + BM25Similarity + disjunction sum, then PER DOC the function score
//                                (plan.h: function_score_value), the minScore test and the item's top-k of FINAL scores
//
// The reference creates the inner weight with ScoreMode.COMPLETE and its scorer answers getMaxScore = Float.MAX_VALUE
// (:168-174, :503-505): nothing is pruned, every live matching doc is scored and counted.  That is the exhaustive scan's
// contract (kernels.hip) with an epilogue between "sum of the clause scores" and "key into the top-k" -- which is why the scan
// itself cannot serve: it prunes in ACCUMULATOR space (acc_reaches(v, thr)) and derives candidate scores from accumulators at
// three places, and a per-doc factor breaks both.  Here theta bounds FINAL keys only and never meets an accumulator.
//
// It consumes the scan's plan records (DItem / DPart / DTerm / DQuery) and writes the scan's item outputs (item_keys unsorted,
// item_counts, item_hits, per-slice sums), so expand_terms_kernel in front and merge_topk_kernel / slice_relation_kernel behind
// are the existing ones.  Fixed-point accumulators only (ds_add_u64, marker 0): the sums are exact in any order.
//
// Work decomposition: one workgroup of kScanWaves waves per item; the item's sub-tiles (kTileDocs docs) are taken in ROUNDS of
// one sub-tile per wave.  In a round every wave on its own streams its sub-tile's postings into its private LDS accumulators,
// then sweeps them: accept set, inner score, function membership (one 64-bit word per function and 64 docs, a wave-uniform
// load), final score, hit test, key -- and leaves the candidate keys in place of the accumulators.  One barrier; then the
// waves append their candidates to the shared buffer at positions every thread derives from the per-wave counts (no atomics),
// or, when the round's candidates do not fit, wave by wave with a top-k compaction (topk.hiph) wherever the buffer would
// overflow -- a compacted buffer (<= k keys) always takes one wave's sub-tile (plan.h: kFsCandCap).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bm25_common.hiph"

namespace nrtgpu {

struct FuncSmem {
  uint64_t acc[kScanWaves][kTileDocs];   // per wave: fixed-point sums of its sub-tile, then its candidate keys (0: none)
  uint64_t cand[kFsCandCap];             // candidate keys of the item, unordered
  float    cache[kLdsCaches][256];       // BM25 normInverse tables of the query's fields
  TopkScratch sc;
  uint32_t wcount[2][kScanWaves];        // candidates each wave holds in its sub-tile, by round parity
  uint32_t slot_hits[kSliceSlots];       // hits of this item per searcher slice it touches (plan.h: DPart.slice)
  uint32_t slot_slice[kSliceSlots];
};
static_assert(sizeof(FuncSmem) <= 160 * 1024, "the workgroup owns one CU's 160 KiB LDS");

constexpr int kFsSlots = kTileDocs / 64;   // accumulator slots per lane

// The wave's candidate keys (left in its sub-tile by the sweep) into cand[pos ...], slot-major; the sub-tile is all markers after.
__device__ __forceinline__ void push_candidates(FuncSmem& s, uint64_t* acc, uint32_t lane, uint32_t pos) {
#pragma unroll 4
  for (int j = 0; j < kFsSlots; ++j) {
    const uint32_t i = lane + 64u * (uint32_t)j;
    const uint64_t key = acc[i];
    const unsigned long long b = __ballot(key != 0ull);
    if (key != 0ull) {
      const uint32_t at = pos + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
      if (at < (uint32_t)kFsCandCap) s.cand[at] = key;   // (always true: the caller made room)
      acc[i] = 0ull;
    }
    pos += (uint32_t)__popcll(b);
  }
}

__global__ __launch_bounds__(kScanThreads, kScanWaves / 4)
void bm25_function_score_kernel(const DItem* __restrict__ items, const DPart* __restrict__ parts, const DTerm* __restrict__ terms,
                                const DQuery* __restrict__ queries, const float* __restrict__ caches,
                                const DFuncQuery* __restrict__ fqueries, const DFuncMasks* __restrict__ fmasks,
                                unsigned long long* __restrict__ theta_g, uint32_t* __restrict__ slice_sum,
                                uint64_t* __restrict__ item_keys, uint32_t* __restrict__ item_counts, uint64_t* __restrict__ item_hits,
                                uint32_t k_stride) {
  __shared__ FuncSmem s;
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), lane = tid & 63u;
  uint64_t* const acc = &s.acc[wave][0];
  const DItem* const item = items + blockIdx.x;
  const uint32_t query = item->query, part_begin = item->part_begin, n_parts = item->n_parts;
  const int fx_E = item->fx_E;
  const DQuery* const q = queries + query;
  const uint32_t k = min(q->k, (uint32_t)kMaxK);
  const DFuncQuery* const fq = fqueries + query;
  const uint32_t n_functions = min((uint32_t)fq->n_functions, (uint32_t)kMaxFunctions);
  const bool multi_item = q->n_items > 1;
  unsigned long long* const my_theta_g = theta_g + query;
  // searchAfter compares FINAL scores: a hit at or above after_key was collected on an earlier page (it still counts)
  const uint64_t after_key = q->has_after ? pack_key(q->after_score, (uint32_t)q->after_doc) : ~0ull;

  // ---- prologue: markers, normInverse tables, slice counters
  for (int j = 0; j < kFsSlots; ++j) acc[lane + 64u * (uint32_t)j] = 0ull;
  {
    const uint32_t n_lds = min(item->n_caches, (uint32_t)kLdsCaches) * 256u;
    const uint32_t cache_off = item->cache_off;
    for (uint32_t i = tid; i < n_lds; i += kScanThreads) (&s.cache[0][0])[i] = caches[cache_off + i];
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

  for (uint32_t g0 = 0; g0 < total_tiles; g0 += (uint32_t)kScanWaves, par ^= 1u) {
    if (multi_item) {   // what the query's other items have published (a bound on final keys: at least k docs of the query exceed it)
      const uint64_t t = __hip_atomic_load(my_theta_g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      theta = t > theta ? t : theta;
    }
    const uint32_t g = g0 + wave;
    uint32_t n_cand = 0;   // wave-uniform
    if (g < total_tiles) {
      const DPart* part = parts + part_begin + pi;
      while (pi + 1u < n_parts && g >= part->tile_offset + (part->tile_end - part->tile_begin)) {
        ++pi;
        ++part;
      }
      const uint32_t tile = g - part->tile_offset + part->tile_begin;
      const uint32_t base = tile * (uint32_t)kTileDocs;
      const uint32_t max_doc = part->max_doc;
      const uint32_t tile_len = base < max_doc ? min((uint32_t)kTileDocs, max_doc - base) : 0u;
      const uint32_t gdoc0 = (uint32_t)(part->doc_base + (int32_t)base);

      // ---- (1) accumulate: every clause's postings of the sub-tile.  Lane l looks up the posting range of clause l (one memory
      //      round trip for all clauses); a clause's postings are then taken 4 x 64 at a time, the eight column loads of a lane
      //      in flight together.
      const uint32_t n_terms = min(part->n_terms, (uint32_t)kMaxTerms);
      const DTerm* const part_terms = terms + part->term_begin;
      uint32_t my_lo = 0, my_hi = 0;
      if (lane < n_terms) {
        const DTerm* mt = part_terms + lane;
        const gu32_ptr cells = (gu32_ptr)mt->cell_off;
        if (mt->docids != nullptr) {
          const uint32_t c = tile >> mt->shift;
          my_lo = cells[c];
          my_hi = cells[c + 1u];
        }
      }
      for (uint32_t t = 0; t < n_terms; ++t) {
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)my_lo, (int)t), hi = (uint32_t)__builtin_amdgcn_readlane((int)my_hi, (int)t);
        if (lo >= hi) continue;   // uniform
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
            // the score code (plan.h: DTerm.fnorm): table byte offset (freq << 7 | norm) << 2, or the escape word; both carry
            // apply_live_kernel's "doc is deleted" mark
            const uint32_t cw = code[u];
            const bool esc = (cw >> 31) != 0u;
            const uint32_t f = esc ? ((cw >> 8) & 0x3FFFFFu) : ((cw >> 9) & 15u);
            const bool dead = esc ? ((cw >> 30) & 1u) != 0u : (cw >> 20) != 0u;
            const uint32_t nb = esc ? (cw & 255u) : ((cw >> 2) & 127u);
            if (off < tile_len && !dead) {
              const uint32_t val = score_value<true>(bm25_score(w, (float)(int32_t)f, cache[nb]), fx_scale);
              atomicAdd((unsigned long long*)&acc[off], (unsigned long long)val << fx_shift);
            }
          }
        }
      }

      // ---- (2) sweep: slot lane + 64 j is doc base + 64 j + lane, i.e. bit `lane` of word j of the sub-tile's mask words
      const NRT_GLOBAL uint64_t* const live_bits = (const NRT_GLOBAL uint64_t*)part->live_bits;
      const DFuncMasks* const fm = fmasks + part_begin + pi;
      const uint32_t word0 = base >> 6;
      uint32_t wave_hits = 0;
#pragma unroll 2
      for (int j = 0; j < kFsSlots; ++j) {
        const uint32_t i = lane + 64u * (uint32_t)j;
        const uint64_t v = acc[i];
        uint64_t key = 0;
        if (64u * (uint32_t)j < tile_len) {   // uniform: the words below exist
          const uint32_t wi = word0 + (uint32_t)j;
          bool ok = v != 0ull;
          if (live_bits != nullptr) ok = ok && ((live_bits[wi] >> lane) & 1ull) != 0ull;
          uint32_t matched = 0;
          for (uint32_t fi = 0; fi < n_functions; ++fi) {
            const NRT_GLOBAL uint64_t* const m = (const NRT_GLOBAL uint64_t*)fm->mask[fi];
            const uint64_t mw = m != nullptr ? m[wi] : ~0ull;
            matched |= (uint32_t)((mw >> lane) & 1ull) << fi;
          }
          bool hit = false;
          if (ok) {
            const float inner = acc_score<true>(v, fx_E);
            const float final_score = function_score_value(*fq, matched, inner, &hit);
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

    // ---- (3) the round's candidates into the shared buffer
    uint32_t tot = 0, before = 0;
#pragma unroll
    for (uint32_t w2 = 0; w2 < (uint32_t)kScanWaves; ++w2) {
      const uint32_t c = s.wcount[par][w2];
      tot += c;
      before += w2 < wave ? c : 0u;
    }
    if (cnt + tot <= (uint32_t)kFsCandCap) {   // uniform
      push_candidates(s, acc, lane, cnt + before);
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
        if (wave == w2) push_candidates(s, acc, lane, cnt);
        cnt += c;
      }
    }
  }

  // ---- epilogue: the item's final top-k, its hits per slice
  __syncthreads();
  if (cnt > k) {
    uint64_t thr = 0;
    cnt = topk_compact<kScanThreads, kFsCandCap>(s.cand, cnt, k, &s.sc, &thr);
  }
  __syncthreads();
  uint64_t* out = item_keys + (size_t)blockIdx.x * k_stride;
  const uint32_t n = min(cnt, k_stride);
  for (uint32_t i = tid; i < n; i += kScanThreads) out[i] = s.cand[i];
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

void launch_bm25_function_score(hipStream_t stream, uint32_t n_items, const DItem* items, const DPart* parts, const DTerm* terms,
                                const DQuery* queries, const float* caches, const DFuncQuery* fqueries, const DFuncMasks* fmasks,
                                unsigned long long* theta_g, uint32_t* slice_sum, uint64_t* item_keys, uint32_t* item_counts,
                                uint64_t* item_hits, uint32_t k_stride) {
  if (n_items == 0) return;
  hipLaunchKernelGGL(bm25_function_score_kernel, dim3(n_items), dim3(kScanThreads), 0, stream, items, parts, terms, queries, caches,
                     fqueries, fmasks, theta_g, slice_sum, item_keys, item_counts, item_hits, k_stride);
}

}  // namespace nrtgpu
