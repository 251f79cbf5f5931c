// valuemask.hip -- the gfx950 kernel behind nrtgpu_segment_set_mask_from_values (include/nrtgpu.h): a FILTER / MUST_NOT mask of
// one leaf built from the leaf's resident doc value columns -- the docs that pass EVERY clause of the call (a numeric range, "has
// a value", "a value in a given set"; plan.h: DValueClause) as 64-bit words, bit d = doc d.  liveDocs are not looked at: the mask
// is independent of deletes, the routes that read it apply them.
//
//   value_mask_kernel   one launch per call.  A wave owns whole 64-doc words (word w: waves grid-stride), lane l of a word owns
//                       doc 64 w + l.  Per clause: the lane's code by one coalesced 4-byte load and the column's `has` word
//                       (a wave-uniform 8-byte load), the clause's test, __ballot of the verdicts ANDed into the word.  A word
//                       that is empty after a clause skips the later ones.  Columns are padded to whole sub-tiles (a multiple
//                       of 64 docs; start[] plus one): no bounds test on a load.  The word starts as the docs below max_doc,
//                       so bits at or beyond it are 0.  Lane 0 writes the word: one 64-bit vector store.
//   multi-valued        the lane walks codes[start[d] .. start[d + 1]) until a value passes (docset.hip: docset_range_any);
//                       only lanes whose doc is still in the word walk; the bound is the doc's count, read on entry.
//   in set              the call's code sets (sorted, duplicate-free: the host) are copied into the workgroup's LDS once; a
//                       value is looked up by value_set_has (plan.h), whose step count is the set's length's alone.
//   value_mask64_kernel the same walk over 64-BIT columns (nrtgpu_segment_set_mask_from_values64): range / exists clauses, one
//                       coalesced 8-byte load per lane and clause, no sets
// All writes are vector stores in plain HIP; every loop is bounded by a count known on entry.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bm25_common.hiph"

namespace nrtgpu {

// one clause's test of one code (set: the workgroup's LDS copy of the call's code sets; set_len is wave-uniform)
__device__ __forceinline__ bool value_clause_accepts(uint32_t lo, uint32_t hi, const uint32_t* set, uint32_t set_len, uint32_t code) {
  if (!range_accepts_code(lo, hi, code)) return false;
  return set_len == 0u || value_set_has(set, set_len, code);
}

__global__ __launch_bounds__(kValueMaskThreads)
void value_mask_kernel(const DValueClause* __restrict__ clauses, uint32_t n_clauses, const uint32_t* __restrict__ sets, uint32_t n_set_codes,
                       uint64_t* __restrict__ out, uint32_t n_words, uint32_t max_doc) {
  extern __shared__ uint32_t set_lds[];   // n_set_codes codes: the sets of the call's IN_SET clauses, back to back
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), lane = tid & 63u;
  for (uint32_t i = tid; i < n_set_codes; i += (uint32_t)kValueMaskThreads) set_lds[i] = sets[i];
  __syncthreads();

  constexpr uint32_t kWaves = (uint32_t)kValueMaskThreads / 64u;
  const uint32_t stride = gridDim.x * kWaves;
  n_clauses = min(n_clauses, (uint32_t)kMaxRanges);
  for (uint32_t w = blockIdx.x * kWaves + wave; w < n_words; w += stride) {   // (uniform)
    const uint32_t doc = 64u * w + lane;
    const uint32_t below = max_doc - 64u * w;   // the word's docs below max_doc (>= 1: w < n_words)
    uint64_t word = below < 64u ? (1ull << below) - 1ull : ~0ull;
#pragma unroll 1
    for (uint32_t c = 0; c < n_clauses && word != 0ull; ++c) {   // (uniform: a word that is empty reads no further column)
      const DValueClause* const cl = clauses + c;
      const NRT_GLOBAL uint32_t* const codes = (const NRT_GLOBAL uint32_t*)cl->code;
      const uint32_t lo = cl->lo_code, hi = cl->hi_code, set_len = cl->set_len;
      const uint32_t* const set = set_lds + cl->set_off;
      const bool mine = ((word >> lane) & 1ull) != 0ull;
      bool pass = false;
      if (codes == nullptr) {   // uniform: the column holds no value
        word = 0ull;
        break;
      }
      if (cl->multi != 0u) {   // uniform
        const NRT_GLOBAL uint32_t* const start = (const NRT_GLOBAL uint32_t*)cl->has;
        const uint32_t s0 = start[doc], s1 = start[doc + 1u];
        const uint32_t n = mine ? s1 - s0 : 0u;   // the lane's count bounds its walk
#pragma unroll 1
        for (uint32_t v = 0; v < n && !pass; ++v) pass = value_clause_accepts(lo, hi, set, set_len, codes[s0 + v]);
      } else {
        const NRT_GLOBAL uint64_t* const has = (const NRT_GLOBAL uint64_t*)cl->has;
        const uint32_t code = codes[doc];
        const uint64_t hw = has != nullptr ? has[w] : ~0ull;   // uniform
        pass = ((hw >> lane) & 1ull) != 0ull && value_clause_accepts(lo, hi, set, set_len, code);
      }
      word &= __ballot(pass);
    }
    if (lane == 0u) out[w] = word;
  }
}

// value_mask_kernel's wave-per-word walk over 64-BIT columns (nrtgpu_segment_set_mask_from_values64; plan.h: DValueClause64):
// range / exists clauses over single-valued columns -- per clause one coalesced 8-byte load per lane, the `has` word, the test
// through range_accepts_code64.  No sets, no LDS.
__global__ __launch_bounds__(kValueMaskThreads)
void value_mask64_kernel(const DValueClause64* __restrict__ clauses, uint32_t n_clauses, uint64_t* __restrict__ out, uint32_t n_words, uint32_t max_doc) {
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), lane = tid & 63u;
  constexpr uint32_t kWaves = (uint32_t)kValueMaskThreads / 64u;
  const uint32_t stride = gridDim.x * kWaves;
  n_clauses = min(n_clauses, (uint32_t)kMaxRanges);
  for (uint32_t w = blockIdx.x * kWaves + wave; w < n_words; w += stride) {   // (uniform)
    const uint32_t doc = 64u * w + lane;
    const uint32_t below = max_doc - 64u * w;   // the word's docs below max_doc (>= 1: w < n_words)
    uint64_t word = below < 64u ? (1ull << below) - 1ull : ~0ull;
#pragma unroll 1
    for (uint32_t c = 0; c < n_clauses && word != 0ull; ++c) {   // (uniform: a word that is empty reads no further column)
      const DValueClause64* const cl = clauses + c;
      const NRT_GLOBAL uint64_t* const codes = (const NRT_GLOBAL uint64_t*)cl->code64;
      const NRT_GLOBAL uint64_t* const has = (const NRT_GLOBAL uint64_t*)cl->has;
      if (codes == nullptr) {   // uniform: the column holds no value
        word = 0ull;
        break;
      }
      const uint64_t code = codes[doc];   // (the column is padded to whole sub-tiles, a multiple of 64 docs: no bounds test)
      const uint64_t hw = has != nullptr ? has[w] : ~0ull;   // uniform
      const bool pass = ((hw >> lane) & 1ull) != 0ull && range_accepts_code64(cl->lo_code, cl->hi_code, code);
      word &= __ballot(pass);
    }
    if (lane == 0u) out[w] = word;
  }
}

void launch_value_mask64(hipStream_t stream, const DValueClause64* clauses, uint32_t n_clauses, uint64_t* out, uint32_t n_words, uint32_t max_doc) {
  if (n_words == 0) return;
  constexpr uint32_t kWaves = (uint32_t)kValueMaskThreads / 64u;
  const uint32_t blocks = std::min<uint32_t>((n_words + kWaves - 1u) / kWaves, 2048u);
  hipLaunchKernelGGL(value_mask64_kernel, dim3(blocks), dim3(kValueMaskThreads), 0, stream, clauses, n_clauses, out, n_words, max_doc);
}

void launch_value_mask(hipStream_t stream, const DValueClause* clauses, uint32_t n_clauses, const uint32_t* sets, uint32_t n_set_codes, uint64_t* out,
                       uint32_t n_words, uint32_t max_doc) {
  if (n_words == 0) return;
  constexpr uint32_t kWaves = (uint32_t)kValueMaskThreads / 64u;
  const uint32_t blocks = std::min<uint32_t>((n_words + kWaves - 1u) / kWaves, 2048u);   // 8 workgroups per CU, the rest by the grid stride
  hipLaunchKernelGGL(value_mask_kernel, dim3(blocks), dim3(kValueMaskThreads), (size_t)n_set_codes * sizeof(uint32_t), stream, clauses, n_clauses, sets,
                     n_set_codes, out, n_words, max_doc);
}

}  // namespace nrtgpu
