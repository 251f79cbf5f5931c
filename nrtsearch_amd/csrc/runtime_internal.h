// runtime_internal.h -- shared declarations of the host runtime behind include/nrtgpu.h (not part of the ABI).
//
// The runtime is split by concern: runtime.cpp (errors, context, workspaces, statistics, exchange table, host
// helpers), segment.cpp (the segment store: upload, seal, liveDocs, masks), planner.cpp (queries -> launch
// plan), search.cpp (BM25 entry points, hybrid tail, merge), coalescer.h (request coalescing: the leader/follower mechanism behind
// the single-query entries of search.cpp and vectors.cpp; standard library only), finalscore.cpp (the host
// path of the final-score routes), funcscore.cpp (function-score queries), multimatch.cpp (multi-match queries),
// fieldsort.cpp (a text query's hits sorted by a doc value column), fieldsort64.cpp (by a 64-bit one), termscount.cpp (its hits counted per value of one),
// docset.cpp (both over a doc set without a text clause), valuemask.cpp (filter masks built from doc value columns), vectors.cpp (exact kNN, vector rescoring).  Types the ABI names opaquely (nrtgpu_ctx, nrtgpu_seg) live in the global namespace;
// everything else in nrtgpu::rt.
#pragma once
#include <hip/hip_runtime.h>
#include <fcntl.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <sys/mman.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <climits>
#include <cmath>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <optional>
#include <shared_mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/nrtgpu.h"
#ifdef NRTGPU_DEV
#include "../../include/nrtgpu_dev.h"
#endif
#include "coalescer.h"
#include "host_math.h"
#include "plan.h"

namespace nrtgpu {
void launch_bm25_scan(hipStream_t stream, bool fixed_point, bool pipelined, bool packed, int ablation, uint32_t n_items, const DItem* items,
                      const DPart* parts, const DTerm* terms, const DQuery* queries, const float* caches, unsigned long long* theta_g,
                      unsigned long long* quant_g, const DExchange* xch, uint32_t* slice_sum, uint64_t* item_keys, uint32_t* item_counts,
                      uint64_t* item_hits, uint32_t k_stride, uint64_t* item_prof);
void launch_bm25_maxscore(hipStream_t stream, bool profile, bool packed, int shapes, const MsArgs& args, const MsArgs* args_d);
// the final-score kernels (finalscore.hiph): one workgroup per item over the scan's plan records, the scan's item outputs
// function-score queries (funcscore.hip): one DFuncQuery per query, one DFuncMasks per part
void launch_bm25_function_score(hipStream_t stream, const FinalScoreArgs& a, const DFuncQuery* fqueries, const DFuncMasks* fmasks);
// multi-match queries (multimatch.hip): one DGroupQuery per query, a clause's group in DTerm.tab_slot bits 24-28
void launch_bm25_multi_match(hipStream_t stream, const FinalScoreArgs& a, const DGroupQuery* gqueries);
// a function score over multi-match queries (multimatch.hip): the records of both
void launch_bm25_multi_match_function_score(hipStream_t stream, const FinalScoreArgs& a, const DGroupQuery* gqueries, const DFuncQuery* fqueries,
                                            const DFuncMasks* fmasks);
// a text query beside knn clauses (knnclauses.hip): one DKnnPart per part, the listed docs and their knn_sum per (query, leaf)
void launch_bm25_text_knn(hipStream_t stream, const FinalScoreArgs& a, const DKnnPart* kparts, const uint32_t* kdocs, const double* ksums);
// sort by field (fieldsort.hip): one DSortQuery per query, one DSortPart per part
void launch_bm25_field_sort(hipStream_t stream, const FinalScoreArgs& a, const DSortQuery* squeries, const DSortPart* sparts);
// terms aggregation (termscount.hip): one DTermsQuery per query, one DSortPart per part; the scorer, then the compaction of the
// queries' tables into `out` (out_cap entries)
void launch_bm25_terms_count(hipStream_t stream, const FinalScoreArgs& a, const DTermsQuery* tqueries, const DSortPart* sparts, DTermsState* states,
                             unsigned long long* tables, unsigned long long* out, uint32_t n_queries, uint32_t out_cap);
// doc-set requests (docset.hip): the sorted / counting route's per-query record, one DRangeQuery per query, one DSortPart per part
// for the sort / count column and kMaxRanges per part for the range clauses' columns.  multi: the call names a multi-valued
// column (a range clause's, the 32-bit count's): a column's arity is the clause's / the query's flag (plan.h: DRangeQuery.multi,
// kTermsQueryMulti), so a batch that mixes arities is one launch.  Their siblings over 64-bit columns and the range facets: below
void launch_docset_sort(hipStream_t stream, bool multi, const FinalScoreArgs& a, const DSortQuery* squeries, const DRangeQuery* rqueries,
                        const DSortPart* sparts, const DSortPart* rparts);
void launch_docset_terms_count(hipStream_t stream, bool multi, const FinalScoreArgs& a, const DTermsQuery* tqueries, const DRangeQuery* rqueries,
                               const DSortPart* sparts, const DSortPart* rparts, DTermsState* states, unsigned long long* tables, unsigned long long* out,
                               uint32_t n_queries, uint32_t out_cap);
// the text route's terms count over calls that name a multi-valued column (termscount.hip: bm25_terms_count_multi_kernel)
void launch_bm25_terms_count_multi(hipStream_t stream, const FinalScoreArgs& a, const DTermsQuery* tqueries, const DSortPart* sparts, DTermsState* states,
                                   unsigned long long* tables, unsigned long long* out, uint32_t n_queries, uint32_t out_cap);
// a filter mask of one leaf from its doc value columns (valuemask.hip): n_clauses DValueClause, the IN_SET clauses' code sets
// (n_set_codes codes in all, staged in LDS), n_words words out
void launch_value_mask(hipStream_t stream, const DValueClause* clauses, uint32_t n_clauses, const uint32_t* sets, uint32_t n_set_codes, uint64_t* out,
                       uint32_t n_words, uint32_t max_doc);
// the same over 64-bit columns (valuemask.hip: value_mask64_kernel): range / exists clauses, no sets
void launch_value_mask64(hipStream_t stream, const DValueClause64* clauses, uint32_t n_clauses, uint64_t* out, uint32_t n_words, uint32_t max_doc);
// sort by a 64-bit column (fieldsort64.hip, docset.hip): one DSort64Query per query, one DSort64Part per part; the doc-set form
// with the doc set's DRangeQuery per query and its kMaxRanges 32-bit DSortPart per part
void launch_bm25_field_sort64(hipStream_t stream, const FinalScoreArgs& a, const DSort64Query* squeries, const DSort64Part* sparts);
void launch_docset_sort64(hipStream_t stream, bool multi, const FinalScoreArgs& a, const DSort64Query* squeries, const DRangeQuery* rqueries,
                          const DSort64Part* sparts, const DSortPart* rparts);
// numeric range facets (rangecount.hip, docset.hip): one DRangeCountQuery per query, the call's cut array (uint32 codes, or uint64
// when `wide`), one DSortPart per part whose `code` is the count column at that width, the call's uint32 interval counters
void launch_bm25_range_count(hipStream_t stream, bool wide, const FinalScoreArgs& a, const DRangeCountQuery* rqueries, const DSortPart* sparts,
                             const void* cuts, uint32_t* counters);
void launch_docset_range_count(hipStream_t stream, bool wide, bool multi, const FinalScoreArgs& a, const DRangeCountQuery* cqueries,
                               const DRangeQuery* rqueries, const DSortPart* sparts, const DSortPart* rparts, const void* cuts, uint32_t* counters);
// terms aggregation over a 64-bit column (termscount64.hip, docset.hip): one DTermsQuery per query, one DSort64Part per part, the
// queries' DTermsState64 records, the tables' key and count arrays; the scorer, then the compaction into out_codes / out_counts
// (out_cap entries).  The doc-set form with the doc set's DRangeQuery per query and its kMaxRanges 32-bit DSortPart per part
// (multi: some range clause names a multi-valued column)
void launch_bm25_terms_count64(hipStream_t stream, const FinalScoreArgs& a, const DTermsQuery* tqueries, const DSort64Part* sparts, DTermsState64* states,
                               unsigned long long* table_keys, uint32_t* table_counts, unsigned long long* out_codes, uint32_t* out_counts,
                               uint32_t n_queries, uint32_t out_cap);
void launch_docset_terms_count64(hipStream_t stream, bool multi, const FinalScoreArgs& a, const DTermsQuery* tqueries, const DRangeQuery* rqueries,
                                 const DSort64Part* sparts, const DSortPart* rparts, DTermsState64* states, unsigned long long* table_keys,
                                 uint32_t* table_counts, unsigned long long* out_codes, uint32_t* out_counts, uint32_t n_queries, uint32_t out_cap);
#ifdef NRTGPU_DEV
void launch_debug_wave_kth(hipStream_t stream, const uint64_t* keys, uint32_t n, uint32_t r, uint64_t* out);   // (maxscore.hip: topk_kth_wave on its own)
void launch_debug_walk_value(hipStream_t stream, float weight, const uint32_t* freq, const uint32_t* norm, const float* table, int fx_scale,
                             uint32_t fx_shift, uint32_t n, uint64_t* out);   // (kernels.hip: one posting's fixed-point value)
#endif
void launch_term_frontier(hipStream_t stream, const uint32_t* fnorm, const uint64_t* t_start, const uint32_t* t_count,
                          const uint64_t* t_look, const uint32_t* t_meta, const void* look_base, uint32_t n_terms, DTermAux* out);
void launch_term_bits(hipStream_t stream, const uint32_t* docids, const uint64_t* t_start, const uint32_t* t_count, const uint64_t* t_look,
                      const uint32_t* which, uint32_t n_which, uint32_t max_count, void* look_base);
void launch_term_cells(hipStream_t stream, const uint32_t* docids, const uint64_t* t_start, const uint32_t* t_count, const uint64_t* t_look,
                       const uint32_t* t_meta, const uint32_t* which, uint32_t n_which, uint32_t max_cells, uint32_t max_doc, void* look_base);
void launch_expand_terms(hipStream_t stream, const DQExpand* qx, const DQTerm* qterms, const uint32_t* out_begin, uint32_t n_queries,
                         uint32_t n_leaves, DTerm* out);   // (qx: behind the batch's DExpandHead, plan.h)
void launch_slice_relation_past(hipStream_t stream, const uint32_t* slice_sum, const uint32_t* slice_past, const DQuery* queries, uint32_t n_slices,
                                uint64_t* out_hits, uint32_t n);
void launch_slice_relation(hipStream_t stream, const uint32_t* slice_sum, const DQuery* queries, uint32_t n_slices, uint64_t* out_hits,
                           uint32_t n);
void launch_patch_hits(hipStream_t stream, const uint64_t* lower, uint64_t* hits, uint32_t n);
void launch_merge_topk(hipStream_t stream, uint32_t n_queries, const uint64_t* in_keys, const uint32_t* in_counts,
                       const uint64_t* in_hits, const uint32_t* list_idx, const uint32_t* q_base,
                       const uint32_t* q_nlists, uint32_t k_stride_in, const uint32_t* q_k, uint64_t* out_keys,
                       uint32_t* out_counts, uint64_t* out_hits, uint32_t k_stride_out, const uint32_t* help_query = nullptr,
                       uint32_t n_help = 0, uint32_t help_slot_base = 0, const unsigned long long* spec_g = nullptr);
void launch_fold_norms(hipStream_t stream, const uint32_t* docids, const uint32_t* freqs, const uint8_t* norms,
                       uint32_t* fnorm, uint64_t n, uint32_t* overflow);
void launch_pack_count(hipStream_t stream, const uint32_t* fnorm, uint64_t n, uint32_t n_blocks, uint32_t* counts);
void launch_pack_write(hipStream_t stream, const uint32_t* docids, const uint32_t* fnorm, uint64_t n, uint32_t n_blocks,
                       const uint32_t* dir, uint32_t* exceptions, uint32_t* packed);
void launch_apply_live(hipStream_t stream, const uint32_t* docids, uint32_t* fnorm, uint64_t n, const uint64_t* live);
void launch_knn_row_norms(hipStream_t st, const float* vecs, int32_t dim, int64_t n, float* norm2);
int launch_knn_score(hipStream_t st, uint32_t blocks, const float* vecs, const float* vnorm2, const int32_t* ord_to_doc,
                     const uint64_t* live_bits, int32_t dim, int64_t row_begin, int64_t row_end, int32_t doc_base,
                     const float* qpanel, const float* qnorm2, int32_t n_q, int32_t sim, float boost,
                     const unsigned long long* theta, uint64_t* cand, uint32_t* cand_cnt, uint32_t cap, int32_t append_only = 0,
                     const uint64_t* const* accept_of = nullptr);   // this leaf's row of the pass's accept table (plan.h: kKnnAcceptCols)
void launch_knn_select(hipStream_t st, uint32_t n_q, uint64_t* topk, uint32_t* topk_cnt, uint32_t k_stride, uint32_t k,
                       const uint64_t* cand, uint32_t* cand_cnt, uint32_t cap, unsigned long long* theta,
                       uint32_t* overflow);
void launch_knn_refine_select(hipStream_t st, uint32_t n_q, uint64_t* topk, uint32_t* topk_cnt, uint32_t k_stride, uint32_t k,
                              const uint64_t* cand, uint32_t* cand_cnt, uint32_t cap, unsigned long long* theta, uint32_t* overflow,
                              const DVecSeg* segs, int32_t n_segs, int32_t dim, int32_t sim, const float* qpanel, const float* qnorm2,
                              float boost, const float* ebound, float erel, const float* min_score /* per query */, uint32_t k_int, int32_t certify,
                              uint32_t* cert);
void launch_knn_norm_max(hipStream_t st, const float* norm2, int64_t n, uint32_t* out_bits);
void launch_knn_norm_min(hipStream_t st, const float* norm2, int64_t n, uint32_t* out_bits);
void launch_knn_absmax(hipStream_t st, const float* vecs, int64_t n_elems, uint32_t* out_bits);
size_t knn_sketch_bytes(int32_t dim, int64_t n);
size_t knn_sketch_lds_bytes(int32_t dim, int32_t n_q);
bool knn_sketch_fits(int32_t dim, int32_t n_q);   // the sketch kernel's LDS: panel + queue + its static tables within 160 KB
void launch_knn_panel_fp16(hipStream_t st, const float* qpanel, const float* qscale, int32_t dim, int32_t n_q, void* panel16);
void launch_knn_sketch_build(hipStream_t st, const float* vecs, int32_t dim, int64_t n, float scale, void* sketch);
int launch_knn_sketch(hipStream_t st, uint32_t blocks, const DKnnLeaf* leaves, int32_t n_leaves, int32_t dim, int64_t tile_begin,
                      int64_t tile_end, const void* panel16, const float* qnorm2, const float* qscale, int32_t n_q, int32_t sim,
                      float boost, const unsigned long long* theta, uint64_t* cand, uint32_t* cand_cnt, uint32_t cap, int32_t append_only = 0);
void launch_rescore_vectors(hipStream_t st, const float* vecs, const float* vnorm2, int32_t dim, const float* query,
                            float qnorm2, int32_t sim, float boost, const int64_t* vec_row, const float* first_scores,
                            int32_t n, double qw, double rw, float* out_scores);
void launch_hybrid_rescore(hipStream_t st, uint32_t n_queries, const uint64_t* first_keys, const uint32_t* first_counts,
                           uint32_t k_stride, const DVecSeg* segs, int32_t n_segs, int32_t dim, const float* qvecs,
                           const float* qnorm2, int32_t sim, float boost, double qw, double rw, uint32_t window,
                           uint64_t* out_keys, uint32_t* out_counts, uint32_t w_stride, int32_t drop_foreign = 0);
void launch_hybrid_hits(hipStream_t st, const uint64_t* first_hits, const uint32_t* first_counts, const uint32_t* q_k, int32_t carries,
                        uint64_t* out_hits, uint32_t n);
// byte (int8) vector fields (knn_bytes.hip)
int32_t knn_bytes_steps(int32_t dim);                     // 64-dimension steps a row is resident with
size_t knn_bytes_tile_bytes(int32_t dim, int64_t n);      // the rows of a field in tile order
size_t knn_bytes_panel_bytes(int32_t dim, int32_t n_q);   // a query panel in operand order: [steps][1 or 4 panels][64 lanes] x 16 bytes
void launch_knn_bytes_pack(hipStream_t st, const int8_t* rows, int32_t dim, int64_t row0, int64_t n_chunk, void* tiles, int32_t* norm2);
int launch_knn_bytes(hipStream_t st, uint32_t blocks, const DKnnBytesLeaf* leaves, int32_t n_leaves, int32_t dim, int64_t tile_begin,
                     int64_t tile_end, const void* panel, const int32_t* qnorm2, int32_t n_q, int32_t sim, float boost, float min_score,
                     const unsigned long long* theta, uint64_t* cand, uint32_t* cand_cnt, uint32_t cap, int32_t append_only = 0,
                     const float* min_scores = nullptr);   // a pass of knn requests: n_q thresholds; the leaves bring accept_of (plan.h)
// the rescorers over a byte field; query / qvecs: int8 in piece order = the query, zero-padded to 64 * knn_bytes_steps(dim) bytes
void launch_rescore_byte_vectors(hipStream_t st, const void* tiles, const int32_t* vnorm2, int32_t dim, const void* query, int32_t qnorm2,
                                 int32_t sim, float boost, const int64_t* vec_row, const float* first_scores, int32_t n, double qw, double rw,
                                 float* out_scores);
void launch_hybrid_rescore_bytes(hipStream_t st, uint32_t n_queries, const uint64_t* first_keys, const uint32_t* first_counts,
                                 uint32_t k_stride, const DByteVecSeg* segs, int32_t n_segs, int32_t dim, const void* qvecs,
                                 const int32_t* qnorm2, int32_t sim, float boost, double qw, double rw, uint32_t window, uint64_t* out_keys,
                                 uint32_t* out_counts, uint32_t w_stride);
// the gather route of the filtered knn entries (knn.hip, knn_bytes.hip; vectors_gather.cpp).  max_rows: an upper bound of *count
int launch_knn_accept_rows(hipStream_t st, const DKnnGatherLeaf* leaves, int32_t n_leaves, int64_t total_rows, uint64_t* list, uint32_t* count,
                           uint32_t cap);
int launch_knn_gather_score(hipStream_t st, const DKnnGatherLeaf* leaves, const uint64_t* list, const uint32_t* count, uint32_t max_rows,
                            int32_t dim, const float* qpanel, const float* qnorm2, int32_t n_q, int32_t sim, float boost, float min_score,
                            uint64_t* cand, uint32_t* cand_cnt, uint32_t cap);
int launch_knn_gather_bytes(hipStream_t st, const DKnnGatherLeaf* leaves, const uint64_t* list, const uint32_t* count, uint32_t max_rows,
                            int32_t dim, const void* queries, const int32_t* qnorm2, int32_t n_q, int32_t sim, float boost, float min_score,
                            uint64_t* cand, uint32_t* cand_cnt, uint32_t cap);
}  // namespace nrtgpu

namespace nrtgpu {
namespace rt {

// ---- errors (runtime.cpp) ----------------------------------------------------------------------
extern thread_local std::string g_last_error;
extern thread_local int64_t g_deadline_ns;           // nrtgpu_set_thread_deadline_ns: 0 = none
extern thread_local nrtgpu_diagnostics g_diag;       // nrtgpu_last_diagnostics
extern thread_local std::vector<int32_t> g_thread_slices;   // nrtgpu_set_thread_slices: the caller's slice of every leaf of its next calls
int64_t monotonic_ns();
inline bool deadline_passed(int64_t deadline_ns) { return deadline_ns != 0 && monotonic_ns() >= deadline_ns; }
// clear != false: the calling thread runs without its deadline until the scope ends, then has it back
struct DeadlineScope {
  int64_t saved;
  explicit DeadlineScope(bool clear) : saved(g_deadline_ns) { if (clear) g_deadline_ns = 0; }
  ~DeadlineScope() { g_deadline_ns = saved; }
};
#define NRT_CHECK_DEADLINE(what)                                                                             \
  do {                                                                                                       \
    if (deadline_passed(g_deadline_ns)) return fail(NRTGPU_ERR_TIMEOUT, "deadline passed %s", what);        \
  } while (0)
int fail(int code, const char* fmt, ...);
double now_ms();
// Experiment knobs: the DEVELOPMENT build (-DNRTGPU_DEV, libnrtgpu_dev.so) reads them from the environment for A/B runs; the
// product library is configured through nrtgpu_config and the nrtgpu_set_* calls only, and always takes the default.
inline long dev_env_int(const char* name, long dflt) {
#ifdef NRTGPU_DEV
  if (const char* e = getenv(name)) return atol(e);
#else
  (void)name;
#endif
  return dflt;
}
inline const char* dev_env_str(const char* name, const char* dflt) {
#ifdef NRTGPU_DEV
  if (const char* e = getenv(name)) return e;
#else
  (void)name;
#endif
  return dflt;
}

#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t _e = (expr);                                                                        \
    if (_e != hipSuccess)                                                                          \
      return fail(_e == hipErrorOutOfMemory ? NRTGPU_ERR_OOM : NRTGPU_ERR_HIP, "%s failed: %s (%s:%d)", #expr, \
                  hipGetErrorString(_e), __FILE__, __LINE__);                                      \
  } while (0)

// ------------------------------------------------------------------------------------------------
// growable device / pinned buffers
// ------------------------------------------------------------------------------------------------
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  int reserve(size_t bytes) {
    if (bytes <= cap) return 0;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    size_t want = bytes + bytes / 4 + 4096;
    HIP_TRY(hipMalloc(&p, want));
    cap = want;
    return 0;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};
struct PinBuf {
  void* p = nullptr;
  size_t cap = 0;
  int reserve(size_t bytes) {
    if (bytes <= cap) return 0;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
    size_t want = bytes + bytes / 4 + 4096;
    HIP_TRY(hipHostMalloc(&p, want, hipHostMallocDefault));
    cap = want;
    return 0;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
};

// ------------------------------------------------------------------------------------------------
// segment store
// ------------------------------------------------------------------------------------------------
struct TermEntry {
  uint32_t group;      // which upload group holds the columns
  uint64_t start;      // first posting in the group's columns
  uint32_t count;
  uint32_t shift;      // doc-range cell = tile >> shift
  uint64_t cell_start; // first entry of the term's cell table inside the group's table buffer
  uint32_t aux_idx;    // the term's DTermAux record inside the group's d_aux (written at seal)
};

struct TermGroup {
  uint32_t* d_docids = nullptr;
  uint32_t* d_freqs = nullptr;   // raw freq column, only between add_terms and seal (nullptr => freq == 1)
  uint32_t* d_fnorm = nullptr;   // score-code column (same allocation as d_docids), filled at seal
  bool folded = false;
  bool packed = false;           // NRTGPU_FLAG_PACKED_POSTINGS, after the seal: d_docids = packed column, d_fnorm = d_dict
  uint32_t* d_dict = nullptr;    // packed postings: the group's exception list (header, directory, escape words)
  uint32_t* d_cells = nullptr;   // concatenated per-term cell tables
  DTermAux* d_aux = nullptr;     // MaxScore route: one record per term of the group (impact frontier, lookup structure), seal
  char* d_look = nullptr;        // the lookup structures of the group's terms (plan.h: kLookMap / kLookCells), one buffer
  uint64_t look_bytes = 0;
  uint32_t n_look[3] = {0, 0, 0};   // terms per lookup kind (plan.h: kLook*; diagnostics)
  uint32_t n_terms = 0;
  std::vector<uint64_t> h_start;  // per term of the group (add order): first posting, postings -- kept until the seal
  std::vector<uint32_t> h_count;
  bool has_freqs = false;
  uint64_t n_postings = 0;
#ifdef NRTGPU_DEV
  // what build_term_aux gave each term of the group (add order): kind | log2 docs per cell << 8, and the structure's bytes --
  // the host's copy, for nrtgpu_debug_term_lookup (include/nrtgpu_dev.h)
  std::vector<uint32_t> h_look_meta;
  std::vector<uint64_t> h_look_cost;
#endif
};

// Read-only open-addressing view of a field's term dictionary (built at seal): the planner does
// one lookup per (query clause, leaf), ~50k per batch, so a probe should touch one cache line.
struct FlatDict {
  struct Cell { int64_t key; uint32_t idx; uint32_t used; };
  std::vector<Cell> cells;
  std::vector<TermEntry> entries;
  uint32_t shift = 64;
  static inline uint64_t mix(int64_t k) { return (uint64_t)k * 0x9E3779B97F4A7C15ull; }
  void build(const std::unordered_map<int64_t, TermEntry>& d) {
    size_t cap = 16;
    uint32_t bits = 4;
    while (cap < d.size() * 2 + 2) { cap <<= 1; ++bits; }
    cells.assign(cap, Cell{0, 0, 0});
    entries.clear();
    entries.reserve(d.size());
    shift = 64 - bits;
    for (const auto& kv : d) {
      size_t h = (size_t)(mix(kv.first) >> shift);
      while (cells[h].used) h = (h + 1) & (cap - 1);
      cells[h] = Cell{kv.first, (uint32_t)entries.size(), 1u};
      entries.push_back(kv.second);
    }
  }
  inline const TermEntry* find(int64_t key) const {
    if (cells.empty()) return nullptr;
    const size_t mask = cells.size() - 1;
    size_t h = (size_t)(mix(key) >> shift);
    for (;;) {
      const Cell& c = cells[h];
      if (!c.used) return nullptr;
      if (c.key == key) return &entries[c.idx];
      h = (h + 1) & mask;
    }
  }
};

struct FieldData {
  uint8_t* d_norms = nullptr;    // nullptr => norms omitted
  uint32_t max_norm = 1;         // largest norm byte of the field in this segment (longest doc); 1 when omitted
  std::unordered_map<int64_t, TermEntry> dict;   // build-time (duplicate detection); searches use `flat`
  FlatDict flat;
  std::vector<TermGroup> groups;
  float* d_vectors = nullptr;
  float* d_vnorm2 = nullptr;            // |v|^2 per row (cosine / euclidean)
  int32_t* d_ord_to_doc = nullptr;
  std::vector<int32_t> h_ord_to_doc;     // host copy: docid -> row lookups of the rescore path
  int32_t dim = 0, n_vec = 0;   // dim: the rows' dimension AS RESIDENT -- the field's own (dim_user) rounded up to a multiple of 16,
                                // the extra elements zero (they add nothing to any of the four similarities' sums)
  int32_t dim_user = 0;
  float vnorm2_max = 0.f;                // largest |v|^2 of the rows
  void* d_sketch = nullptr;              // the rows in fp16, matrix-core operand order (knn.hip); nullptr: none (yet)
  int sketch_state = -1;                 // 0: to be built by the first exact search over the field (segment.cpp: ensure_vector_sketch), 1: built, -1: never
  float sketch_scale = 1.f;              // the power of two the rows were multiplied by before rounding
  float absmax = 0.f, vnorm2_min = 0.f;  // largest |element|, smallest non-zero |v|^2 (the sketch's error bound)
  // A byte (int8) vector field (nrtgpu_segment_add_byte_vectors; a field holds float rows or byte rows, never both): the rows as
  // tiles of 16 in the i8 matrix instruction's operand order, zero-padded to whole 64-dimension steps (knn_bytes.hip), and |v|^2
  // per row as int32.  n_vec, dim_user, d_ord_to_doc, h_ord_to_doc and live_vec serve both kinds; dim = 64 x the resident steps.
  bool byte_rows = false;
  void* d_btiles = nullptr;
  int32_t* d_bnorm2 = nullptr;
  // A per-doc value column (nrtgpu_segment_add_doc_values), independent of whatever else the field id holds: the values'
  // order-preserving codes (plan.h: doc_value_code), one per doc, padded to whole sub-tiles, and which docs have a value
  // (nullptr: every doc has).  dv_kind < 0: the field has no column.
  // A MULTI-VALUED column (nrtgpu_segment_add_doc_values_multi; a field holds a column of one arity): d_dv_start != nullptr --
  // one uint32 per doc, padded to whole sub-tiles, plus one; doc d's values are d_dv_code[d_dv_start[d] .. d_dv_start[d + 1]),
  // their codes in upload order; the padding entries hold the number of values.  d_dv_code is nullptr when the column holds no
  // value; d_dv_has is unused.
  uint32_t* d_dv_code = nullptr;
  uint64_t* d_dv_has = nullptr;
  uint32_t* d_dv_start = nullptr;
  int32_t dv_kind = -1;
  // A 64-BIT column (nrtgpu_segment_add_doc_values64; dv_kind is kDocValuesInt64 / kDocValuesFloat64, single-valued): the codes
  // (plan.h: doc_value_code64) live in d_dv_code64, d_dv_has says which docs have a value, and d_dv_code stays nullptr -- what
  // reads 32-bit codes (doc_values_column) finds no column to read at the wrong width.  dv_min_code / dv_max_code: the least and
  // the greatest code among the dv_n values uploaded (dv_n == 0: no bound): the window a sort's packed keys are built in.
  uint64_t* d_dv_code64 = nullptr;
  uint64_t dv_min_code = 0, dv_max_code = 0;
  int32_t dv_n = 0;
  // rows whose doc is live under the segment's current liveDocs (what an exact vector query matches), counted on first
  // use per liveDocs version
  mutable std::atomic<int64_t> live_vec{-1};
  mutable std::atomic<uint64_t> live_vec_version{0};
  FieldData() = default;
  FieldData(const FieldData& o)
      : d_norms(o.d_norms), max_norm(o.max_norm), dict(o.dict), flat(o.flat), groups(o.groups), d_vectors(o.d_vectors),
        d_vnorm2(o.d_vnorm2), d_ord_to_doc(o.d_ord_to_doc), h_ord_to_doc(o.h_ord_to_doc), dim(o.dim), n_vec(o.n_vec),
        vnorm2_max(o.vnorm2_max), d_sketch(o.d_sketch), sketch_state(o.sketch_state), sketch_scale(o.sketch_scale), absmax(o.absmax),
        vnorm2_min(o.vnorm2_min), byte_rows(o.byte_rows), d_btiles(o.d_btiles), d_bnorm2(o.d_bnorm2), d_dv_code(o.d_dv_code),
        d_dv_has(o.d_dv_has), d_dv_start(o.d_dv_start), dv_kind(o.dv_kind), d_dv_code64(o.d_dv_code64), dv_min_code(o.dv_min_code),
        dv_max_code(o.dv_max_code), dv_n(o.dv_n) {}
};

}  // namespace rt
}  // namespace nrtgpu

using namespace nrtgpu;      // (internal header: every translation unit of the runtime wants both)
using namespace nrtgpu::rt;

struct nrtgpu_ctx;
// The immutable part of a segment -- posting columns, norms, vectors, the seal-time structures -- shared by the handles
// of its reader versions (nrtgpu_segment_fork): freed with the last of them.
struct SegCore {
  int device = 0;
  std::map<int32_t, FieldData> fields;
  // the liveDocs folded into the posting columns (apply_live_kernel), if any: once a core is shared nobody folds again,
  // and every handle's liveDocs must be a subset of these (Lucene's deletes only accumulate)
  std::vector<uint64_t> folded_live;
  bool folded = false;
  std::mutex sketch_mu;   // the lazy build of a vector field's sketch
  std::atomic<int64_t> shared_extra_bytes{0};   // device memory added to the core after the seal (the sketches): counted for every handle
  ~SegCore();
};
struct nrtgpu_seg {
  nrtgpu_ctx* ctx = nullptr;
  uint64_t uid = 0;              // unique over the process (never reused, unlike the handle's address): keys the planner's caches;
                                 // the forks of a segment share it (and with it the resident term tables)
  int32_t max_doc = 0;
  uint32_t n_tiles = 0;
  bool sealed = false;
  std::shared_ptr<SegCore> core;
  std::map<int32_t, FieldData>& fields;   // == core->fields
  nrtgpu_seg() : core(std::make_shared<SegCore>()), fields(core->fields) {}
  explicit nrtgpu_seg(std::shared_ptr<SegCore> c) : core(std::move(c)), fields(core->fields) {}
  uint64_t* d_live = nullptr;
  int32_t n_deleted = 0;         // docs cleared in liveDocs (host pop-count at set_live_docs)
  uint64_t live_version = 1;     // a fresh process-wide number at every set_live_docs / fork (keys per-liveDocs caches in the shared core)
  int64_t device_bytes = 0;
  // FILTER / MUST_NOT clauses as doc-set masks: host copies of the registered masks and of liveDocs,
  // and the combined accept sets (live & filter & ~must_not) the scan reads, built on first use
  std::vector<uint64_t> h_live;                      // empty = all live
  bool live_folded = false;  // the posting columns carry the current liveDocs (apply_live_kernel): the scan needs no mask for them
  // The content lock.  Searches hold it SHARED from planning until their kernels have finished; set_live_docs / set_mask
  // take it exclusively, so a reader-version change never rewrites columns or masks under a running scan.  Not a
  // std::shared_mutex: a search begun on one thread may be waited for on another (nrtgpu_search_bm25_batch_device_begin /
  // nrtgpu_pending_wait -- unlocking a std::shared_mutex from a thread that does not hold it is undefined), and
  // nrtgpu_segment_release under running searches must not free what they read (ShardState.java:506-527 closes readers
  // while SEARCH-pool threads run): the handle is then freed by the LAST search that lets go of it.
  mutable std::mutex content_m;
  mutable std::condition_variable content_cv;
  mutable int content_readers = 0;          // searches in flight over this handle
  mutable int content_writers_waiting = 0;  // pending exclusive owners: new SYNCHRONOUS searches let them go first (no writer
                                            // starvation under overlapping request threads).  A PIPELINED search
                                            // (nrtgpu_search_bm25_batch_device_begin) passes a waiting writer while other searches
                                            // are in flight: its thread may be the one that must still wait for one of them --
                                            // begin i + 1 before wait i -- and parking it behind the writer that waits for search
                                            // i is a deadlock (a bounded number of passes only postpones it:
                                            // tests/test_exchange_gpu.py found that on the CPU).  The price: a pipeline that never
                                            // drains can delay set_mask / set_live_docs on the handles it searches -- reader
                                            // versions are forks (no writer), masks are registered before a handle is searched
  mutable bool content_writing = false;
  mutable bool content_released = false;    // nrtgpu_segment_release came while searches were in flight: the last one frees
  void content_lock_shared(bool pipelined) const;
  void content_unlock_shared() const;       // may free the handle (content_released)
  std::map<int32_t, std::vector<uint64_t>> masks;
  mutable std::mutex accept_mu;
  struct AcceptSet { uint64_t* bits; uint64_t used; int64_t count; };   // used: the cache's clock at the last lookup (least recently used goes first); count: set bits below max_doc
  mutable std::map<std::vector<int32_t>, AcceptSet> accept;   // key: the filter mask ids ascending, 0, the must_not mask ids ascending
  mutable uint64_t accept_clock = 0;
  mutable std::vector<uint64_t*> accept_retired;              // evicted, maybe still read by a search in flight: freed by the last reader out
  bool accept_retired_empty() const {
    std::lock_guard<std::mutex> lk(accept_mu);
    return accept_retired.empty();
  }
};

// Exclusive ownership of a segment's content (liveDocs, masks, the posting columns' liveness coding).
struct SegWriteLock {
  nrtgpu_seg* seg;
  explicit SegWriteLock(nrtgpu_seg* s);
  ~SegWriteLock();
  SegWriteLock(const SegWriteLock&) = delete;
  SegWriteLock& operator=(const SegWriteLock&) = delete;
};

// Shared locks on the content of every (distinct) segment of a call, taken in address order.
struct SegReadLocks {
  std::vector<const nrtgpu_seg*> held;
  // pipelined: the caller returns to its own caller holding the locks (begin / wait); see nrtgpu_seg::content_writers_waiting.
  // A thread must not start a synchronous search over handles it holds un-waited pipelined searches on.
  SegReadLocks(const nrtgpu_seg* const* segs, int32_t n, bool pipelined = false) {
    for (int32_t i = 0; i < n; ++i)
      if (segs && segs[i]) held.push_back(segs[i]);
    std::sort(held.begin(), held.end());
    held.erase(std::unique(held.begin(), held.end()), held.end());
    for (const nrtgpu_seg* s : held) s->content_lock_shared(pipelined);
  }
  ~SegReadLocks() {   // (any thread: nrtgpu_pending_wait may run on another one than the begin)
    for (const nrtgpu_seg* s : held) s->content_unlock_shared();
  }
  SegReadLocks(const SegReadLocks&) = delete;
  SegReadLocks& operator=(const SegReadLocks&) = delete;
};

namespace nrtgpu {
namespace rt {
// ------------------------------------------------------------------------------------------------
// per-call workspace
// ------------------------------------------------------------------------------------------------
struct Slot {
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;
  hipEvent_t ev_turn = nullptr;   // recorded behind this call's whole-GPU kernels (nrtgpu_ctx::last_turn)
  hipEvent_t ev_wait = nullptr;   // hipEventBlockingSync: what a caller sleeps on under NRTGPU_FLAG_BLOCKING_WAIT
  PinBuf h_plan;     // host staging of the plan blob
  DevBuf d_plan;     // device copy
  DevBuf d_work;     // theta + item outputs + merge outputs
  DevBuf d_aux;      // hybrid tail: leaf table, query vectors, rescored windows
  PinBuf h_aux;
  PinBuf h_out;      // merged results on the host
  std::vector<hipEvent_t> round_ev;   // collect_timing: start / stop of every knn_score launch of a panel
  bool busy = false;
};

// The caller's wait for its stream: a spin inside hipStreamSynchronize by default (lowest latency; it keeps a CPU busy), a
// sleep on a blocking event under NRTGPU_FLAG_BLOCKING_WAIT (several ranks sharing the host's CPUs: one process per GPU
// with a few calls in flight each would otherwise spin on more CPUs than the box has).
// hipGetLastError() is the CALLING THREAD's: a runtime call of somebody else on this thread (the caller's own GPU code, another
// library) that failed and was never asked about leaves its error there, and the first of OUR functions that checks its launches
// with hipGetLastError() would report it as its own.  Entry points that launch kernels forget it first.
inline void forget_foreign_hip_error() { (void)hipGetLastError(); }

inline hipError_t wait_for_stream(bool blocking, hipStream_t st, hipEvent_t blocking_event) {
  if (!blocking) return hipStreamSynchronize(st);
  const hipError_t e = hipEventRecord(blocking_event, st);
  return e != hipSuccess ? e : hipEventSynchronize(blocking_event);
}

}  // namespace rt
}  // namespace nrtgpu

namespace nrtgpu {
namespace rt {
struct LeafSetCache;

// The context's helper threads (cfg.host_threads - 1 of them, started at nrtgpu_create): run(n, fn) executes
// fn(0) .. fn(n - 1) on the caller and whichever helpers are free, and returns when all are done.  Several
// callers may run jobs at the same time (two batches in flight).  Replaces a std::thread per planner chunk per
// batch: thread creation alone cost more than the work once term lookups came from the cache.
class WorkPool {
 public:
  explicit WorkPool(int helpers);
  ~WorkPool();
  void run(int n, const std::function<void(int)>& fn);
  int helpers() const { return (int)threads_.size(); }

 private:
  struct Job {
    const std::function<void(int)>* fn;
    int n;
    std::atomic<int> next{0}, done{0};
  };
  void loop();
  std::vector<std::thread> threads_;
  std::mutex mu_;
  std::condition_variable cv_;
  std::vector<std::shared_ptr<Job>> jobs_;
  bool stop_ = false;
};
}  // namespace rt
}  // namespace nrtgpu

struct nrtgpu_dist;   // dist.cpp: RCCL communicator of this context (nrtgpu_dist_init)

// The context's LAUNCHER: one thread that enqueues the searches begun with nrtgpu_search_bm25_*_begin, in the order they were begun
// (search.cpp: device_begin_impl).  A submitting thread then only PLANS -- the plan of batch i + 1 is being built while batch i's
// plan is packed, copied and its seven launches are issued (0.1 ms per 1024-query batch: a quarter of a step of one rank of an
// 8-GPU job, whose scorer runs for 0.3 ms).  Created by the first _begin, joined by nrtgpu_destroy.
struct Launcher {
  std::thread th;
  std::mutex mu;
  std::condition_variable cv;
  std::deque<std::function<void()>> q;
  bool stop = false;
  explicit Launcher(int device);
  ~Launcher();
  void push(std::function<void()> f);
};

struct nrtgpu_ctx {
  nrtgpu_config cfg{};
  nrtgpu_dist* dist = nullptr;
  int device = 0;
  int n_cus = 0;
  std::mutex mu;
  std::condition_variable cv;
  std::vector<std::unique_ptr<Slot>> slots;
  hipEvent_t last_turn = nullptr;   // (under gpu_mu) recorded behind the whole-GPU kernels enqueued last: the next ones wait for it ON THE DEVICE
  hipEvent_t last_knn_turn = nullptr;   // (under gpu_mu) the same behind the exact vector search's stage enqueued last (vectors.cpp)
  std::mutex gpu_mu;    // device execution of one batch at a time: a scan kernel wants the whole GPU,
                        // overlapping two only stretches both (host-side planning/unpacking still overlap)
  std::mutex stats_mu;
  nrtgpu_stats stats{};
  std::atomic<int32_t> knn_gather_permille{0};   // nrtgpu_set_knn_gather: filtered knn requests that accept at most this share of the rows read only those (0: never)
  std::atomic<int> knn_sketch_skip[4] = {};   // per similarity: panels that go straight to the fp32 rows (the sketch did not certify lately)
  double prof[16] = {0};
  std::vector<uint64_t> last_walls;   // NRTGPU_FLAG_PROFILE: {start, end, item, windows} per output slot of the last MaxScore launch
  int64_t last_walls_items = 0;       // ... whose first this-many slots are the items' owners (helpers behind the scan's slots)
  double ms_prof[16] = {0};   // the same for the items of the MaxScore route (nrtgpu_get_maxscore_profile)
  int64_t ms_meetings[5] = {0};   // ... and their meetings, overflow meetings, compactions, one-wave estimates (nrtgpu_debug_maxscore_meetings),
                                  // guesses that raised theta in a meeting (nrtgpu_debug_maxscore_meeting_guesses)
  // request coalescing (coalescer.h): the single-query entries' callers merged into batches (nrtgpu_search_bm25_coalesced, search.cpp)
  // and into panels (nrtgpu_knn_exact_coalesced on kco, nrtgpu_knn_search_coalesced on rco: vectors.cpp)
  // (the same two over byte fields: nrtgpu_knn_exact_bytes_coalesced on bkco, nrtgpu_knn_search_bytes_coalesced on brco -- queues of
  //  their own, so float and byte callers never share a panel)
  nrtgpu::rt::Coalescer co, kco, rco, bkco, brco;
  int32_t co_linger_us = 150;   // (under co.mu: nrtgpu_set_coalescing)
  // speculative thresholds (plan.h: kHitsSpecInvalid; nrtgpu_debug_spec_counters): queries run under speculation, queries whose guess
  // failed and were run again, and the switch the library throws itself when too many fail (docs not spread like a sample)
  std::atomic<int64_t> spec_queries{0}, spec_reruns{0};   // (sums over the context's leaf sets since nrtgpu_set_speculation: nrtgpu_stats)
  std::atomic<int> spec_off{0};                            // ... 1 once SOME leaf set has had its speculation switched off
  std::atomic<int> spec_scattered{0};                      // ... 1 once SOME leaf set has been moved to the scattered window order
  std::atomic<uint64_t> spec_epoch{1};                     // nrtgpu_set_speculation calls (the leaf sets' verdicts start over)
  std::atomic<int> spec_z16{5 * 16};   // the guess's margin x 16 (nrtgpu_set_speculation)
  std::atomic<int64_t> shard_docs{0}, index_docs{0};   // nrtgpu_set_shard_share: this context's share of a sharded index (0: equal shards)
  std::atomic<int64_t> live_segments{0};   // segment handles (uploads and forks) that have not been freed yet (nrtgpu_debug_live_segments)
  // MyIndexSearcher.SlicingParams of the searcher this context serves (nrtgpu_set_slicing)
  std::atomic<int32_t> slice_max_docs{250000}, slice_max_segments{5}, virtual_shards{1};
  std::unique_ptr<nrtgpu::rt::WorkPool> pool;   // helper threads of the host side (planning, unpacking results)
  std::mutex launcher_mu;
  std::unique_ptr<Launcher> launcher;           // (search.cpp: device_begin_impl)
  // planner caches, one per leaf set seen lately (most recent first)
  std::mutex lsc_mu;
  std::vector<std::shared_ptr<nrtgpu::rt::LeafSetCache>> leaf_sets;
  // cross-GPU bound exchange (nrtgpu_exchange_open)
  void* xch_host = nullptr;                 // mmap of the shared table
  unsigned long long* xch_dev = nullptr;    // the same memory as the GPU sees it
  size_t xch_bytes = 0;
  int32_t xch_world = 0, xch_rank = 0;
};

namespace nrtgpu {
namespace rt {

// layout helper: carve 256-byte aligned regions out of one blob
struct Carver {
  size_t off = 0;
  size_t take(size_t bytes) {
    const size_t o = off;
    off += (bytes + 255) & ~(size_t)255;
    return o;
  }
};

// ---- planner caches ----------------------------------------------------------------------------
// One term over one leaf set, resolved once: the per-leaf dictionary lookups and the static half of every DTerm.
// A batch of 1024 five-clause queries over 10 leaves otherwise pays 51 k dictionary probes; query terms repeat
// across batches (and within them), the leaf set changes only when the searcher is refreshed.
struct TermLeaves {
  const DTerm* d_table = nullptr;  // resident copy of the per-leaf records (columns, cell table, aux record, posting count in
                                   // `weight`; docids == nullptr: the leaf lacks the term) -- what DQTerm.table points at
  std::vector<uint32_t> count;     // postings per leaf
  int64_t total = 0;
  uint32_t max_norm = 0;           // largest norm byte of the field over the leaves that hold the term
};
struct LeafSetCache {
  std::vector<uint64_t> uids;    // the leaf set this cache belongs to (segment uids, in call order)
  struct Key {
    int32_t field;
    int64_t hash;
    bool operator==(const Key& o) const { return field == o.field && hash == o.hash; }
  };
  struct KeyHash {
    size_t operator()(const Key& k) const { return (size_t)(((uint64_t)k.hash ^ ((uint64_t)(uint32_t)k.field << 40)) * 0x9E3779B97F4A7C15ull >> 7); }
  };
  static const int kStripes = 64;
  static const size_t kMaxEntries = 1 << 20;  // then the context starts a fresh cache for the leaf set (bounds the memory)
  struct Stripe {
    std::shared_mutex mu;
    std::unordered_map<Key, std::shared_ptr<const TermLeaves>, KeyHash> map;
  };
  Stripe stripes[kStripes];
  // the terms' resident tables: carved out of 1 MiB device chunks that live as long as the cache (a plan in flight
  // holds a reference to the cache)
  int device = 0;
  std::mutex arena_mu;
  std::vector<void*> chunks;
  size_t chunk_used = 0;
  static const size_t kChunkBytes = 1 << 20;
  static const size_t kMaxChunks = 256;       // then the context starts a fresh cache for the leaf set
  bool full() {
    {
      std::lock_guard<std::mutex> lk(arena_mu);
      if (chunks.size() > kMaxChunks) return true;
    }
    return entries() > kMaxEntries;
  }
  void* alloc_tables(size_t stride, size_t want, size_t* got);
  ~LeafSetCache();
  // Entries are never freed while the cache lives (a full cache is replaced as a whole, leaf_set_cache()), so a raw
  // pointer stays valid for as long as the caller holds the cache -- which lets every planner thread keep a private
  // front cache and take no lock and no reference count on a hit (four threads bouncing the stripes' lock words cost
  // more than the lookups themselves).
  uint64_t id = 0;   // unique per cache object: tags the threads' front-cache entries
  // Speculative thresholds (plan.h: kHitsSpecInvalid) are judged PER LEAF SET: the queries run under them over these leaves, the
  // ones whose guess failed and were run again, and the switch the library throws for this leaf set when too many fail (an
  // index whose docid order defeats the estimate must not cost the context's other indexes their speculation; a refresh brings
  // a new leaf set and a fresh verdict).  spec_epoch: the context's nrtgpu_set_speculation count these numbers belong to.
  std::atomic<int64_t> spec_queries{0}, spec_reruns{0};
  std::atomic<int64_t> spec_calls{0}, spec_calls_rerun{0};   // calls judged, calls that needed a second pass (a second pass costs per CALL)
  std::atomic<int> spec_scattered{0};   // the leaf set's windows are walked in the scattered order (maxscore.hip): the second chance
  std::atomic<int> spec_off{0};
  std::atomic<uint64_t> spec_epoch{0};
  const TermLeaves* get(const nrtgpu_seg* const* segs, int32_t n_segs, int32_t field, int64_t hash);
  void get_many(const nrtgpu_seg* const* segs, int32_t n_segs, const Key* keys, size_t n, const TermLeaves** out);
  size_t entries();
};
std::shared_ptr<LeafSetCache> leaf_set_cache(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs);

// ---- workspaces (runtime.cpp) ------------------------------------------------------------------
int acquire_slot(nrtgpu_ctx* ctx, Slot** out);
void release_slot(nrtgpu_ctx* ctx, Slot* s);

// ---- segment store (segment.cpp) ---------------------------------------------------------------
// The doc set a query's hits must lie in: liveDocs & FILTER mask & ~MUST_NOT mask, resident in HBM
// ((0, 0): liveDocs itself, or nullptr once they are folded into the posting columns).
// count (optional): the set's docs -- its bits below max_doc, counted where the set is built and kept with it
int accept_set_of(const nrtgpu_seg* seg, int32_t filter_mask, int32_t must_not_mask, const uint64_t** out, int64_t* count = nullptr);
int accept_set_of(const nrtgpu_seg* seg, const nrtgpu_bm25_query& q, const uint64_t** out);   // all of the query's FILTER / MUST_NOT masks
// segment.cpp: every combined accept set of the handle freed -- a mask or liveDocs changed.  The caller holds the content
// exclusively (SegWriteLock), is its last reader, or destroys the handle.
void drop_accept_sets(nrtgpu_seg* seg);
// vectors of the field whose doc is live (the hits of an exact vector query over the segment)
int64_t live_vector_count(const nrtgpu_seg* seg, const FieldData& f);
int ensure_vector_sketch(const nrtgpu_seg* seg, int32_t field_id);

// ---- vectors (vectors.cpp) ---------------------------------------------------------------------
// nrtgpu_knn_exact with device-resident results (per query k_stride sorted keys, count, live-vector total): the multi-GPU path
int knn_exact_device(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs, int32_t field_id,
                     int32_t sim, const float* queries, int32_t n_queries, int32_t dim, int32_t k, float boost, int32_t k_stride,
                     void* d_keys, void* d_counts, void* d_hits);

// A workspace slot for the length of a scope.
struct SlotGuard {
  nrtgpu_ctx* c;
  Slot* s;
  ~SlotGuard() { release_slot(c, s); }
};

// ---- one description of a vector search, and what the float and the byte searches share around their kernels --------------------
constexpr uint32_t kKnnCap = 1u << 18;   // candidate keys per query and round (2 MiB): the float, the byte and the gather lists alike
constexpr int kKnnMaxQ = 64;   // queries per pass over the rows, and the widest panel a coalescer forms (float: two panels of 32 on
                               // paired workgroups up to 1280 dimensions, knn.hip; byte: four panels of 16, knn_bytes.hip)
// What the queries of a search ask, one value per query: query q's are at [q * stride].  stride 0 is ONE value for every query --
// nrtgpu_knn_search's request, or an ExactVectorQuery's k and boost -- so a uniform request is an array like any other and the
// searches read nothing else.
struct KnnAsk {
  const int32_t* ks;
  const float* boosts;
  const int32_t* masks;       // pre-filter mask ids (0: none)
  const float* min_scores;    // thresholds on the unboosted score (0: none)
  int32_t stride;
  int32_t k(int q) const { return ks[(size_t)q * stride]; }
  float boost(int q) const { return boosts[(size_t)q * stride]; }
  int32_t mask(int q) const { return masks[(size_t)q * stride]; }
  float min_score(int q) const { return min_scores[(size_t)q * stride]; }
  KnnAsk from(int q0) const { return {ks + (size_t)q0 * stride, boosts + (size_t)q0 * stride, masks + (size_t)q0 * stride, min_scores + (size_t)q0 * stride, stride}; }
};
struct KnnUniform {   // the storage of a stride-0 view
  int32_t k, mask;
  float boost, min_score;
  KnnAsk ask() const { return {&k, &boost, &mask, &min_score, 0}; }
};
// One vector search: the leaves, the queries, what is asked and where the answer goes.  knn_search (vectors.cpp) and
// knn_bytes_search (vectors_bytes.cpp) take it, as do the gather route and the passes of the requests entries.
struct KnnCall {
  const nrtgpu_seg* const* segs;
  const int32_t* doc_bases;   // NULL: zeros
  int32_t n_segs, field_id;
  bool bytes;            // int8 rows and queries; else fp32
  const void* queries;   // n_queries x dim elements, row-major
  int32_t n_queries, dim, sim;
  // false: ExactVectorQuery -- every doc with a vector matches, the boost is inside the score.  true: `knn` requests -- pre-filter,
  // threshold on the unboosted score (MinThresholdQuery's MinScoreWrapper), boost applied afterwards, totalHits = the docs returned.
  bool knn_request;
  KnnAsk ask;
  nrtgpu_topdocs* out;   // one per query; or NULL and the device-resident triple of the multi-GPU path (float rows only): per query
                         // k_stride sorted keys, its count, and the live vectors of these leaves as the hit total
  char *ext_keys = nullptr, *ext_cnts = nullptr, *ext_hits = nullptr;
  int32_t k_max() const {   // a pass is searched with the largest k of its members; every member takes the first k of its own
    int32_t k = ask.ks[0];
    for (int32_t q = 1; q < n_queries && ask.stride; ++q) k = std::max(k, ask.k(q));
    return k;
  }
  // All members share one filter and one threshold: the leaf's one accept set and the launch's one threshold serve them (and the
  // gather route may); else the pass carries an accept table per (leaf, member) and a threshold per member.
  bool one_filter() const { return ask.stride == 0; }
  int32_t shared_mask() const { return one_filter() ? ask.masks[0] : 0; }   // != 0: the selective filter of a uniform request
  float score_boost() const { return knn_request ? 1.0f : ask.boosts[0]; }
};

// The leaves of a call that hold rows of its element type, in order: fn(const KnnLeaf&) -> int for each, until one fails.
//   mask < 0: no accept set is looked up (accept = nullptr);  0: liveDocs;  > 0: liveDocs & the mask, ONE accept_set_of per leaf
// and walk -- the walks of a search look a set up as often, and in the order, the loops they replace did.
struct KnnLeaf {
  const nrtgpu_seg* seg;
  const FieldData* f;
  int32_t si, index;              // the call's leaf; the leaves with rows before it
  int32_t doc_base;
  int64_t tile_begin, row_begin;  // tiles of 16 rows / rows of the leaves before it
  int64_t live;                   // vectors whose doc is live (deleted docs are masked inside the kernels and are no hits)
  const uint64_t* accept;         // (vectors are not re-coded for liveDocs: always the mask)
  int64_t accept_docs;            // mask > 0: the docs of the set
};
template <class Fn>
int knn_walk_leaves(const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs, int32_t field_id, bool bytes, int32_t mask, Fn&& fn) {
  KnnLeaf l{};
  for (int si = 0; si < n_segs; ++si) {
    auto fit = segs[si]->fields.find(field_id);
    if (fit == segs[si]->fields.end() || fit->second.n_vec == 0) continue;
    const FieldData& f = fit->second;
    if (!(bytes ? f.d_btiles != nullptr : f.d_vectors != nullptr)) continue;
    l.seg = segs[si];
    l.f = &f;
    l.si = si;
    l.doc_base = doc_bases ? doc_bases[si] : 0;
    l.live = live_vector_count(segs[si], f);
    l.accept = mask < 0 ? nullptr : segs[si]->d_live;
    if (mask > 0)
      if (int rc = accept_set_of(segs[si], mask, 0, &l.accept, &l.accept_docs)) return rc;
    if (int rc = fn((const KnnLeaf&)l)) return rc;
    ++l.index;
    l.tile_begin += ((int64_t)f.n_vec + 15) >> 4;
    l.row_begin += f.n_vec;
  }
  return NRTGPU_OK;
}
template <class Fn>
int knn_walk_leaves(const KnnCall& c, int32_t mask, Fn&& fn) {
  return knn_walk_leaves(c.segs, c.doc_bases, c.n_segs, c.field_id, c.bytes, mask, fn);
}
// liveDocs & the member's filter per (leaf, member) of a pass that carries an accept table (plan.h: kKnnAcceptCols pointers per
// leaf with rows) into `table`: each distinct mask of the pass is looked up once per leaf.
int knn_stage_accept_table(const KnnCall& c, int q0, int nq, const uint64_t** table);
// What a vector entry asks of the field `f` in leaf si: rows of its own element type -- the other type is refused with the
// caller's hint of where to take it -- and of the queries' dimension (dim 0: the caller checks the dimension itself).  *has_rows:
// the leaf holds rows a search of the kind reads.  knn_check_leaves: the same of every leaf that has the field.
int knn_check_field(bool bytes, int si, int32_t field_id, const FieldData& f, int32_t dim, const char* hint, bool* has_rows = nullptr);
int knn_check_leaves(const nrtgpu_seg* const* segs, int32_t n_segs, int32_t field_id, bool bytes, int32_t dim, const char* hint);
constexpr const char* kHintSearchBytes = "search it with nrtgpu_knn_exact_bytes / nrtgpu_knn_search_bytes";
constexpr const char* kHintSearchFloat = "search it with nrtgpu_knn_exact / nrtgpu_knn_search";
constexpr const char* kHintRescoreFloat = "rescore it with nrtgpu_rescore_vectors / nrtgpu_search_hybrid_batch";
constexpr const char* kHintHybridFloatOnly = "the hybrid tail rescores float vector fields only";
// What the searches ask of their scalars; bad_count: the caller's own count (queries, leaves) is out of range -- the same refusal.
// knn_check_byte_boost: hits are kept as keys whose order is the order of NON-NEGATIVE float bits: a negative boost would rank
// them backwards.  byte_boost: knn_bytes_search tests its boost BEFORE k and the dimension are held against the device's limits
// (the coalesced byte entries test theirs after knn_check_scalars: the entries' refusals keep their order).
int knn_check_scalars(bool bad_count, int32_t k, int32_t dim, int32_t sim, const float* byte_boost = nullptr);
int knn_check_byte_boost(float boost);
// |q|^2 (fp32, in element order, every product rounded before it is added: float_qnorm2's chain), the largest |element| and the
// 1-norm of nq queries of `dim` floats; max_abs / l1 may be NULL.  Each sum is a chain of dependent additions, so eight queries are
// walked side by side -- eight independent chains, every query's own order untouched.
void knn_query_stats(const float* queries, int nq, int dim, float* norm2, float* max_abs, double* l1);

// The turns on the device, the timed scoring launches, the rounds over the leaves' tiles, a panel's statistics.
struct KnnRun {
  nrtgpu_ctx* ctx;
  Slot* slot;
  size_t n_ev = 0;   // timing events recorded for the panel under way (two per scoring launch)
  // Ordering on the device (search.cpp: enqueue_search has the BM25 side): a stage of a vector search -- nomination launches,
  // selections, rescoring -- starts behind the BM25 scorers enqueued last (they want every CU's LDS) and they start behind it;
  // but two vector searches do NOT queue behind each other: the nomination kernel streams, its workgroups are handed out as
  // CUs come free, so a second call's launches fill the tail of this call's and run under its small selection / rescoring
  // kernels (34 KB of LDS beside a nomination workgroup's 112).  Measured with two callers at 10 M x 768: 32 queries per call
  // 3.21 -> 2.90 ms per step, 64: 3.61 -> 3.20.  The host lock is held for the two event operations only.
  int take_turn();
  int end_turn();
  // One scoring launch: between two events when the context collects timing; a launch status != 0 fails as "<kernel> launch: ...".
  template <class Launch>
  int timed_launch(const char* kernel, Launch&& launch) {
    const bool timing = ctx->cfg.collect_timing != 0;
    if (timing) {
      while (slot->round_ev.size() < n_ev + 2) {
        hipEvent_t ev = nullptr;
        HIP_TRY(hipEventCreate(&ev));
        slot->round_ev.push_back(ev);
      }
      HIP_TRY(hipEventRecord(slot->round_ev[n_ev], slot->stream));
    }
    const int e = launch();
    if (e) return fail(NRTGPU_ERR_HIP, "%s launch: %s", kernel, hipGetErrorString((hipError_t)e));
    if (timing) {
      HIP_TRY(hipEventRecord(slot->round_ev[n_ev + 1], slot->stream));
      n_ev += 2;
    }
    return NRTGPU_OK;
  }
  // One pass over `total_tiles` tiles of 16 rows in rounds: launch(tile_begin, tile_end, blocks, append_only) scores a round,
  // select() follows it.  Nominating, the first round is `first_round` tiles and at most the candidate list (cap rows: every row
  // takes a slot); a later round is 15 x the tiles seen so far (later rounds only append rows that beat theta), and after two
  // selections the remaining launches run back to back (append_only) with ONE selection behind them.  safe: rounds no longer than
  // the list, growing x 4, a selection after each (a panel whose list overflowed is redone so).  Neither: theta is fixed and
  // tight -- everything at once.  A launch takes at most 2^22 tiles.
  template <class Launch, class Select>
  int tile_rounds(int64_t total_tiles, int64_t first_round, uint32_t cap, bool nominate, int safe, Launch&& launch, Select&& select) {
    int64_t seen = 0, round = first_round;
    int selections = 0;
    bool pending = false;
    for (int64_t t = 0; t < total_tiles;) {
      int64_t len = (safe || (nominate && seen == 0)) ? std::min<int64_t>(round, cap >> 4) : round;
      if (!nominate && !safe) len = total_tiles;
      len = std::min<int64_t>(len, (int64_t)1 << 22);   // (a queue entry carries the padded row inside the launch in 26 bits)
      const int64_t te = std::min<int64_t>(total_tiles, t + len);
      const uint32_t blocks = (uint32_t)std::min<int64_t>(((te - t) * 16 + 255) / 256, (int64_t)std::max(ctx->n_cus, 1));
      const bool defer = nominate && !safe && selections >= 2;
      if (int rc = launch(t, te, blocks, defer ? 1 : 0)) return rc;
      if (defer) {
        pending = true;
      } else {
        select();
        ++selections;
      }
      seen += te - t;
      t = te;
      round = safe ? std::min<int64_t>(round * 4, cap >> 4) : std::min<int64_t>(seen * 15, (int64_t)1 << 36);
    }
    if (pending) select();
    return NRTGPU_OK;
  }
  // A pass whose candidate list can overflow (rows in rising order of similarity: every row beats theta): pass(safe) runs it and
  // leaves *overflow -- the flag it fetched -- behind; raised, the pass is redone once in rounds no longer than the list (safe = 1),
  // and a flag still up fails with the caller's text.
  template <class Pass>
  int redo_on_overflow(const uint32_t* overflow, const char* text, Pass&& pass) {
    for (int safe = 0; safe < 2; ++safe) {
      if (int rc = pass(safe)) return rc;
      if (*overflow == 0u) return NRTGPU_OK;
    }
    return fail(NRTGPU_ERR_HIP, "%s", text);
  }
  // the panel is answered: its launches, their time and its rows into the context's statistics; n_ev starts over
  void add_stats(int64_t rows, int64_t sketch_launches, bool second_pass);
};
// A panel's sorted keys -> the callers' nrtgpu_topdocs.  clamp_to_k: counts[q] may exceed k (the byte search's running list).
// knn_request: totalHits = the docs returned, the boost applied afterwards; else `total`.  ask: the members' k and boost -- member
// q of a panel that was searched with the largest k takes the first k(q) keys of its list.
void knn_unpack_topdocs(const uint64_t* keys, const uint32_t* counts, uint32_t k_stride, int nq, bool clamp_to_k, int64_t total,
                        bool knn_request, const KnnAsk& ask, nrtgpu_topdocs* out);
// The searches: over float rows (vectors.cpp) and over byte rows (vectors_bytes.cpp).
int knn_search(nrtgpu_ctx* ctx, const KnnCall& call);
int knn_bytes_search(nrtgpu_ctx* ctx, const KnnCall& call);

// ---- the gather route of the filtered knn entries (vectors_gather.cpp) -------------------------------------------
// A uniform knn request with a filter (KnnCall::shared_mask() != 0) whose filter accepts few enough rows reads only those: the
// accepted rows are listed on the device, scored with final score bits and selected (knn_select_kernel<false>).  Called by
// knn_search / knn_bytes_search behind their argument checks, refusals and SegReadLocks; the call's float queries are padded to
// the RESIDENT dimension.  byte_qnorm2: a byte field's |q|^2 per query (byte_queries_stage), all the route adds to the call.
// The route decision: *gather iff the context's knob (nrtgpu_set_knn_gather) is > 0, the filter accepts at most that share of the
// field's rows over these leaves and the accepted rows fit one candidate list.  *estimate = sum over the leaves that hold the
// field of min(docs of the accept set, rows): an upper bound of the accepted rows (a sparse ord -> doc map accepts fewer).
int knn_gather_route(nrtgpu_ctx* ctx, const KnnCall& call, bool* gather, int64_t* estimate);
int knn_gather_run(nrtgpu_ctx* ctx, const KnnCall& call, const int32_t* byte_qnorm2, int64_t estimate);

// ---- the vector rescorers (vectors.cpp; what is specific to byte fields: vectors_bytes.cpp) ----------------------------------
// |q|^2 of a float query as the rescoring kernels' results depend on it: fp32, in element order, every product rounded before it is
// added.  The one chain the rescoring kernels' inputs use (the searches stage their panels' |q|^2 with knn_query_stats above: eight
// queries side by side in the same element order).
float float_qnorm2(const float* q, int dim);
// The inputs of the rescoring kernels (hybrid_rescore_kernel, hybrid_rescore_bytes_kernel, knn_refine_select_kernel) into host
// memory of the caller, each part optional (NULL):
//   leaves  n_segs slots of 40 bytes: DVecSeg, or DByteVecSeg for a byte field -- one layout (doc_bases may be NULL: zeros)
//   staged  the n queries as the kernel reads them: floats of `dim` elements (the RESIDENT dimension: pad_query_vectors), or int8
//           in piece order, byte_query_stride(dim) bytes each
//   qnorm2  |q|^2 per query: float_qnorm2, or int32 for a byte field (cosine refuses a zero query there)
int stage_rescore_inputs(const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs, int32_t field_id, bool bytes, int32_t sim,
                         const void* queries, int32_t n, int32_t dim, void* leaves, void* staged, void* qnorm2);
// The two-call rescorer (QueryRescorer over a first pass's hits) for either element type: hits -> (segment, row), one gather
// launch per leaf, sort by (combined score desc, doc asc), the window.  What differs comes in as a RescoreKind.
struct RescoreKind {
  const void* (*rows)(const FieldData&);   // the field's resident rows of this element type; NULL: the leaf has none
  const void* query;                       // one staged query (stage_rescore_inputs)
  size_t query_bytes;
  // the leaf's launch: n hits of the leaf, their rows and first-pass scores on the device -> combined scores
  std::function<void(hipStream_t, const FieldData&, const void* d_query, const int64_t* d_rows, const float* d_first, int32_t n, float* d_out)> launch;
};
int rescore_hits_impl(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs, int32_t field_id,
                      const RescoreKind& kind, const int32_t* docs, const float* first_scores, int32_t n, double query_weight, int32_t window,
                      nrtgpu_topdocs* out);
// What the byte entries (vectors_bytes.cpp; the byte tail of search_hybrid_impl, search.cpp) ask before anything is staged: of their
// scalars (the field in every leaf -- byte rows of the query's dimension, or absent: knn_check_leaves).
int byte_rescore_check_args(int32_t sim, int32_t dim, float boost, int32_t window);
size_t byte_query_stride(int32_t dim);
// n queries of `dim` int8 -> piece order and |q|^2 as int32 (padded / qnorm2 may be NULL: check only)
int byte_queries_stage(const int8_t* queries, int32_t n, int32_t dim, int32_t sim, int8_t* padded, int32_t* qnorm2);

// ---- search (search.cpp): pieces the multi-GPU entry (dist.cpp) reuses ------------------------------
// one shard's BM25 search with device-resident results and speculative thresholds guessed against the WHOLE search (search.cpp)
int search_bm25_shard_device(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                             const nrtgpu_bm25_query* queries, int32_t n_queries, int32_t k_stride, void* d_keys, void* d_counts, void* d_hits,
                             int32_t spec_world, void* d_guess, bool* speculated);
// nrtgpu_merge_topk_device + per query the packed key of rank k of the merged list (0: shorter), read from the merged keys
int merge_topk_device_kth(nrtgpu_ctx* ctx, int32_t n_lists, int32_t n_queries, int32_t k_stride, const void* d_keys_in, const void* d_counts_in,
                          const void* d_hits_in, const int32_t* ks, const int32_t* total_hits_thresholds, nrtgpu_topdocs* out, uint64_t* kth);
// a call that ran under speculation has come back: count it for its leaf set (the verdict: search.cpp)
void note_shard_speculation(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs, int64_t n_queries, int64_t n_failed);
// TopDocs.merge of n_lists gathered lists per query (layout [list][query]) into DEVICE arrays (keys n_queries x k_stride, counts,
// hit totals), enqueued on `slot`'s stream; the caller synchronises.
int merge_lists_on_device(nrtgpu_ctx* ctx, Slot* slot, int32_t n_lists, int32_t n_queries, int32_t k_stride, const void* g_keys,
                          const void* g_counts, const void* g_hits, const int32_t* ks, void* d_keys, void* d_counts, void* d_hits);
// Query vectors of `dim_user` elements as the resident rows want them: padded with zeros to the field's resident dimension
// (FieldData.dim).  p == the caller's array when nothing had to be padded.
struct PaddedQueries {
  std::vector<float> buf;
  const float* p = nullptr;
  int32_t dim = 0;
};
int pad_query_vectors(const nrtgpu_seg* const* segs, int32_t n_segs, int32_t field_id, const float* queries, int32_t n, int32_t dim_user,
                      PaddedQueries* out);
// The vector rescorer over device-resident first-pass lists (hybrid_rescore_kernel), enqueued on `slot`'s stream: uploads the leaf
// table and the query vectors into the slot's aux buffers; windows -> d_win_keys (n_queries x w_stride), d_win_counts.
int hybrid_tail_on_device(nrtgpu_ctx* ctx, Slot* slot, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                          int32_t field_id, int32_t sim, const float* query_vectors, int32_t dim, float boost, double qw, double rw,
                          int32_t window, int32_t n_queries, const void* d_first_keys, const void* d_first_counts, int32_t k_stride,
                          int32_t drop_foreign, void* d_win_keys, void* d_win_counts, uint32_t w_stride);

// ---- planner (planner.cpp) ---------------------------------------------------------------------
struct HostPlan {
  std::vector<DQuery> queries;
  std::vector<DItem> items;
  std::vector<DPart> parts;
  std::vector<DQTerm> qterms;       // compact plan: per query clause (expand_terms_kernel writes the DTerms on the device)
  std::vector<DQExpand> qexpand;    // per query
  std::vector<uint32_t> qs_begin;   // per (query, leaf): first DTerm of the pair, ~0 = none
  uint32_t n_dterms = 0;            // DTerm records the expansion writes
  uint32_t n_leaves = 0;
  std::shared_ptr<LeafSetCache> lsc;  // keeps the terms' resident tables alive until the call is over
  std::vector<float> caches;
  std::vector<uint32_t> list_idx;   // per query: item indices (merge input lists)
  std::vector<uint32_t> q_base, q_nlists, q_k;
  std::vector<uint64_t> theta_init;  // per query: key below which nothing is collected (min_competitive_score)
  uint32_t k_stride = 0;
  int64_t postings = 0;             // postings in the scanned term ranges (algorithmic work)
  bool fixed_point = false;         // every query of the batch passed the fixed-point range analysis
  bool clause_counting = false;     // exhaustive scan: some query has minimumNumberShouldMatch > 1 / is a DisjunctionMaxQuery: count-carrying variant
  bool masked = false;              // exhaustive scan: some part reads a doc-set mask (liveDocs / FILTER / MUST_NOT)
  bool ms_shapes = false;           // MaxScore route: some query has a FILTER / MUST_NOT mask, minimumNumberShouldMatch > 1 or is a DisjunctionMaxQuery
  bool ms_two = false;              // MaxScore route: some query's score needs the second accumulator (plan.h: kMsSec*)
  uint32_t n_slices = 1;            // searcher slices over the call's leaves (MyIndexSearcher.slices): per query that many hit sums
  // MaxScore route (maxscore.hip): items [0, n_ms_items) run it, the others the exhaustive scan
  uint32_t n_ms_items = 0;
  std::vector<uint32_t> q_wins;     // per query: doc windows of its MaxScore items (plan.h: MsArgs.q_wins)
  std::vector<int64_t> q_lower;     // per query on that route in kMsModePrune: live docs certain to match (> totalHitsThreshold), else 0
  std::vector<uint8_t> q_route;     // per query: kRouteScan (exhaustive scan) or kRouteMs + its kMsMode* (plan.h)
  int64_t ms_postings = 0;          // postings of the queries on that route (algorithmic work, as `postings`)
  std::vector<int32_t> part_leaf;   // plans built with kept leaves (build_plan: keep) only: per part its leaf's index in the call
};
// A leaf the caller wants planned for a query even though it holds none of the query's terms (knnclauses.cpp: a listed doc
// there is still a hit): the tile range to walk, as a part with n_terms == 0.  tile_end <= tile_begin: not kept.
struct PlanKeepLeaf {
  uint32_t tile_begin, tile_end;
};

const uint8_t kRouteScan = 0, kRouteMs = 1;   // HostPlan.q_route: kRouteMs + kMsMode*
inline uint32_t round_up(uint32_t v, uint32_t m) { return (v + m - 1) / m * m; }
int validate_query(const nrtgpu_bm25_query& q, int qi);
// fixed-point eligibility of one query term: the scale 2^E at which all its scores are integers < 2^32
bool fixed_scale_of_term(float weight, const float* cache256, uint32_t max_norm, int32_t* scale);
// prune: 0 = every query is scanned exhaustively; 1 = queries that qualify take the MaxScore route (total_hits then a
// lower bound, relation GTE); 2 = the same for device-resident results: no searchAfter there (a page may hold fewer
// than numHits hits, and then the relation needs the exact count)
int build_plan(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
               const nrtgpu_bm25_query* queries, int32_t n_queries, HostPlan& hp, int prune = 0, const PlanKeepLeaf* keep = nullptr);
// keep: nullptr, or n_queries x n_segs records (prune == 0 only): the (query, leaf) pairs to plan although the leaf holds none of
// the query's terms; a query none of whose terms any leaf holds is then planned over its kept leaves.  Plans built without it
// are what they were.

// The plan of a doc-set call (docset.cpp): parts without clauses over every tile of every leaf, DPart.live_bits = the query's
// combined accept set with liveDocs.  Of queries[i] only k, total_hits_threshold and the mask fields are read (the masks must be
// resident).  Fills what final_score_run reads of a HostPlan, part_leaf included.
int docset_plan(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs, const nrtgpu_bm25_query* queries,
                int32_t n_queries, HostPlan& hp);

// ---- the text routes' plan blob and workspace (search.cpp: enqueue_search; finalscore.cpp: enqueue_final_score) -----------------
// One layout for every route: the twelve plan arrays of a HostPlan in upload order, and the seven workspace regions every route
// has (per-slot outputs of the scorers, the merge's outputs, the expanded DTerm records).  A route appends what is its own with
// plan.take() / work.take() behind them.  n_slots: output slots of the scorers (the items, and whatever the route puts behind them).
struct PlanLayout {
  Carver plan, work;
  size_t queries, items, parts, qterms, qexpand, qs_begin, caches, list_idx, q_base, q_nlists, q_k, theta;
  size_t item_keys, item_counts, item_hits, out_keys, out_counts, out_hits, terms;
  PlanLayout(const HostPlan& hp, size_t n_slots, size_t n_queries, uint32_t k_stride_out) {
    queries = plan.take(hp.queries.size() * sizeof(DQuery));
    items = plan.take(hp.items.size() * sizeof(DItem));
    parts = plan.take(hp.parts.size() * sizeof(DPart));
    qterms = plan.take(hp.qterms.size() * sizeof(DQTerm));
    qexpand = plan.take(sizeof(DExpandHead) + hp.qexpand.size() * sizeof(DQExpand)) + sizeof(DExpandHead);   // (the head in front: put_expand_head)
    qs_begin = plan.take(hp.qs_begin.size() * 4);
    caches = plan.take(hp.caches.size() * sizeof(float));
    list_idx = plan.take(hp.list_idx.size() * 4);
    q_base = plan.take(hp.q_base.size() * 4);
    q_nlists = plan.take(hp.q_nlists.size() * 4);
    q_k = plan.take(hp.q_k.size() * 4);
    theta = plan.take(hp.theta_init.size() * 8);   // uploaded with the plan, then updated by the kernel
    item_keys = work.take(n_slots * (size_t)hp.k_stride * 8);
    item_counts = work.take(n_slots * 4);
    item_hits = work.take(n_slots * 8);
    out_keys = work.take(n_queries * k_stride_out * 8);
    out_counts = work.take(n_queries * 4);
    out_hits = work.take(n_queries * 8);
    terms = work.take((size_t)hp.n_dterms * sizeof(DTerm));   // written by expand_terms_kernel
  }
  static void put(char* hb, size_t off, const void* src, size_t bytes) {
    if (bytes) memcpy(hb + off, src, bytes);
  }
  void fill(char* hb, const HostPlan& hp) const {   // the twelve arrays into the host blob
    put(hb, queries, hp.queries.data(), hp.queries.size() * sizeof(DQuery));
    put(hb, items, hp.items.data(), hp.items.size() * sizeof(DItem));
    put(hb, parts, hp.parts.data(), hp.parts.size() * sizeof(DPart));
    put(hb, qterms, hp.qterms.data(), hp.qterms.size() * sizeof(DQTerm));
    put(hb, qexpand, hp.qexpand.data(), hp.qexpand.size() * sizeof(DQExpand));
    put(hb, qs_begin, hp.qs_begin.data(), hp.qs_begin.size() * 4);
    put(hb, caches, hp.caches.data(), hp.caches.size() * sizeof(float));
    put(hb, list_idx, hp.list_idx.data(), hp.list_idx.size() * 4);
    put(hb, q_base, hp.q_base.data(), hp.q_base.size() * 4);
    put(hb, q_nlists, hp.q_nlists.data(), hp.q_nlists.size() * 4);
    put(hb, q_k, hp.q_k.data(), hp.q_k.size() * 4);
    put(hb, theta, hp.theta_init.data(), hp.theta_init.size() * 8);
  }
  // what the plan expansion reads in front of the DQExpand array (plan.h: DExpandHead); rows: where it writes the MaxScore
  // route's walk rows, nullptr: none
  void put_expand_head(char* hb, const char* db, DWalkRow* rows) const {
    DExpandHead xh{};
    xh.caches = (const float*)(db + caches);
    xh.queries = (const DQuery*)(db + queries);
    xh.rows = rows;
    memcpy(hb + qexpand - sizeof(DExpandHead), &xh, sizeof(xh));
  }
};
// what every batch entry says of its sizes
int check_batch_size(const nrtgpu_ctx* ctx, int32_t n_queries, int32_t n_segs);
// `hits` as the device leaves it -> out (search.cpp): lower: the MaxScore route's certain bound (0: none); n_first: the length the
// relation is judged by
void unpack_topdocs(const uint64_t* keys, uint32_t n, uint64_t hits, const int32_t k, int64_t lower, uint32_t n_first, nrtgpu_topdocs* out);
// a call's diagnostics and statistics (search.cpp); reads the slot's timing events the call recorded
void account(nrtgpu_ctx* ctx, Slot* slot, const HostPlan& hp, int32_t n_queries, double plan_ms, double t_entry_ms = 0.0, double queue_ms = 0.0);

// ---- the final-score routes (finalscore.cpp): what funcscore.cpp and multimatch.cpp share --------------------------------
// The head of an entry point: the argument checks (null_argument: one of the route's own pointers is NULL; n_queries: the
// batch entries', nullptr for the _supported predicates), the batch entries' first deadline check, hipSetDevice.
int final_score_enter(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs, bool null_argument, const int32_t* n_queries);
// the context's flags neither route runs under; route: "function-score" / "multi-match", for the message
int final_score_check_flags(const nrtgpu_ctx* ctx, const char* route);
// the exhaustive plan (build_plan, prune = 0: nothing may be skipped), refused unless it is a fixed-point one
int final_score_plan(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs, const nrtgpu_bm25_query* queries,
                     int32_t n_queries, const char* route, HostPlan& hp);
struct PlanBytes {   // an array of the route's own, appended to the plan buffer
  const void* p;
  size_t bytes;
};
const int kFinalScoreExtras = 4;   // at most: two per-query record arrays and two per-part arrays (docset.cpp)
// the route's scorer: d_extra[i] = the device address of extras[i]
typedef void (*FinalScoreLaunch)(hipStream_t, const FinalScoreArgs&, const void* const* d_extra);
// From "the plan and the route's records exist" to "out[], the diagnostics and the statistics are filled": workspace, plan upload,
// expansion, the scorer in its turn on the device, merge, per-slice relation, the wait, unpacking.  queries: the CALLER's (k,
// capacity); t0: now_ms() when planning began.  The caller holds its SegReadLocks until this returns.
// own: nullptr, or a route's own device output -- work_bytes of the workspace behind the shared regions, zeroed per call by the
// memset that zeroes the per-slice sums (their address reaches the scorer as FinalScoreArgs.own), and collect(), called behind the
// wait and the unpacking, before the call is accounted: it copies what the route wants of them on the slot's stream.  What the
// routes without one enqueue and copy is what it was.
// counts_past: the route's kernel hands final_epilogue a slice_past (plan.h: FinalScoreArgs) -- the relation then asks of a query with
// a cursor that one slice holds numHits hits BEHIND it, as that slice's collector would before it publishes anything.
struct FinalScoreOwn {
  size_t work_bytes;
  int (*collect)(nrtgpu_ctx* ctx, Slot* slot, const char* d_own, void* user);
  void* user;
};
int final_score_run(nrtgpu_ctx* ctx, const HostPlan& hp, const nrtgpu_bm25_query* queries, int32_t n_queries, nrtgpu_topdocs* out, double t0,
                    const PlanBytes* extras, int n_extras, FinalScoreLaunch launch, const FinalScoreOwn* own = nullptr, bool counts_past = false);

// ---- what the routes lend each other (multimatch.cpp and funcscore.cpp define them; funcscore_multimatch.cpp uses both halves) ----
// multimatch.cpp: the record the kernel and nrtgpu_multi_match_value read, from the caller's struct; refusals by the header's
// table.  occur: the clauses' nrtgpu_term.occur, or nullptr = all SHOULD
int group_record(const nrtgpu_clause_groups& g, int qi, int32_t n_terms, const int32_t* occur, int32_t min_should_match, DGroupQuery* out);
// multimatch.cpp: what the multi-match route refuses of (queries[i], groups[i]) before anything is planned, the context's flags
// aside; the records (optional) and the reduced copies of the queries (plain SHOULD disjunctions: what is planned) on the way
int multi_match_check_queries(const nrtgpu_bm25_query* queries, const nrtgpu_clause_groups* groups, int32_t n_queries, std::vector<DGroupQuery>* records,
                              std::vector<nrtgpu_bm25_query>* flat, std::vector<std::vector<nrtgpu_term>>* flat_terms);
// multimatch.cpp: the plan of the reduced queries (final_score_plan), and every clause's group into its DQTerm
int multi_match_plan(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs, const nrtgpu_bm25_query* flat,
                     const nrtgpu_clause_groups* groups, int32_t n_queries, const char* route, HostPlan& hp);
// funcscore.cpp: the record the kernels and nrtgpu_function_score_value read, from the caller's struct; refusals by the header's table
int function_record(const nrtgpu_function_score& fs, int qi, DFuncQuery* out);
// funcscore.cpp: refuses a function mask that is not resident on a leaf of the call
int function_masks_resident(const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_function_score& fs, int qi);
// funcscore.cpp: the doc sets of every function on every part's leaf, for any plan over these leaves (a part names its leaf via qs_begin)
int function_masks(const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_function_score* functions, const HostPlan& hp,
                   std::vector<DFuncMasks>* out);

// fieldsort.cpp: what the routes over a doc value column (sorted searches, the terms aggregation of termscount.cpp) share.
// What is planned for the queries of such a call: plain SHOULD disjunctions (the vectors own the copies' clauses; the caller
// points queries[i].terms at terms[i] once every query has been pushed).
struct FlatQueries {
  std::vector<nrtgpu_bm25_query> queries;
  std::vector<std::vector<nrtgpu_term>> terms;
};
// the kind of the field's column over the leaves of the call (-1: on no leaf) and whether it is multi-valued; refuses leaves
// that disagree in either
int doc_values_kind(const nrtgpu_seg* const* segs, int32_t n_segs, int32_t field_id, int qi, int* kind, bool* multi);
// the field's column on one leaf as the kernels read it (plan.h: DSortPart, either arity); {nullptr, nullptr}: no doc of the leaf has a value
DSortPart doc_values_column(const nrtgpu_seg* seg, int32_t field_id);
// what both routes refuse of one query as unsupported, in the header's order (under: "a sort" / "a terms count"); *need: the
// clauses a hit matches at least; the query's flat copy is pushed
int doc_values_query(const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_bm25_query& q, int qi, int kind, int32_t field_id, const char* under,
                     uint32_t* need, FlatQueries* flat);
// what the sorted routes (this one, fieldsort64.cpp, docset.cpp) refuse of a nrtgpu_field_sort / nrtgpu_field_sort64 as an invalid argument
template <class SORT>
int field_sort_check(const SORT& s, int qi) {
  if (s.reverse != 0 && s.reverse != 1) return fail(NRTGPU_ERR_INVALID_ARG, "query %d: reverse %d outside 0..1", qi, s.reverse);
  if (s.has_after != 0 && s.has_after != 1) return fail(NRTGPU_ERR_INVALID_ARG, "query %d: the sort's has_after %d outside 0..1", qi, s.has_after);
  if (s.has_after != 0 && s.after_doc < 0) return fail(NRTGPU_ERR_INVALID_ARG, "query %d: after_doc %d", qi, s.after_doc);
  return NRTGPU_OK;
}
// a nrtgpu_field_sort's side of the query's record
void field_sort_record(const nrtgpu_field_sort& s, int kind, DSortQuery* r);
// the pages' key high words -> the value bits the hits sorted as (both sorted routes over a 32-bit column, behind final_score_run)
void field_sort_values(const std::vector<DSortQuery>& records, const std::vector<int>& kinds, int32_t n_queries, nrtgpu_fielddocs* out);
// NRTGPU_ERR_UNSUPPORTED with the reason: the sort's column is multi-valued (both sorted routes, where they refuse "on no leaf")
int field_sort_multi(int qi, int32_t field_id);
// the FILTER / MUST_NOT masks of q are resident on every leaf of the call, else NRTGPU_ERR_UNSUPPORTED naming the query (what
// doc_values_query refuses of them; docset.cpp asks the same of a doc-set query's masks)
int doc_values_masks_resident(const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_bm25_query& q, int qi);
// NRTGPU_ERR_UNSUPPORTED with the reason: a 32-bit entry named a field that holds a 64-bit column (kind >= kDocValuesInt64);
// instead: what serves such a column, or that nothing does
int doc_values_wide(int qi, int32_t field_id, const char* instead);
constexpr const char* kTermsCountWide = "terms counts read 32-bit columns, 64-bit buckets are not built by this entry: count it with "
                                        "nrtgpu_count_terms64_batch / nrtgpu_count_docset_terms64_batch";
// the leaf (index into segs) of every part of a plan of the flat copies: a part names its (query, leaf) pair by its first DTerm
int doc_values_part_leaves(const nrtgpu_seg* const* segs, int32_t n_segs, const HostPlan& hp, const char* route, std::vector<int32_t>* out);
// the column of every part's leaf, for a plan of the flat copies (field_ids: per query)
int doc_values_parts(const nrtgpu_seg* const* segs, int32_t n_segs, const int32_t* field_ids, const HostPlan& hp, const char* route,
                     std::vector<DSortPart>* out);

// fieldsort64.cpp: what the sorted routes over a 64-bit column share (the text route there; the doc-set form in docset.cpp).
// NRTGPU_ERR_UNSUPPORTED with the reason: the sort's column is a 32-bit one (multi: multi-valued); entry32: the entry that serves it
int field_sort64_narrow(int qi, int32_t field_id, bool multi, const char* entry32);
// the bits the call's global docids need: max(1, bit_length(D - 1)), D = max over the leaves of base + max_doc; doc_bases NULL:
// in_order ? the leaves in order, base 0 for the first (the predicates) : every leaf at base 0 (what the plans do).
// NRTGPU_ERR_UNSUPPORTED: D beyond 2^31
int sort64_doc_bits(const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs, bool in_order, uint32_t* db);
// the sort's side of the query's record (`need` is the caller's): the window of the column's codes over the leaves that hold a
// value, the cursor as a code; NRTGPU_ERR_UNSUPPORTED naming the bits when the window does not fit beside db docid bits
int field_sort64_record(const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_field_sort64& s, int kind, uint32_t db, int qi, DSort64Query* r);
// the field's 64-bit column on one leaf ({nullptr, nullptr}: the leaf lacks it -- or holds a 32-bit one, which the checks refused)
DSort64Part doc_values_column64(const nrtgpu_seg* seg, int32_t field_id);
// The internal pages final_score_run fills for such a call (ks: the queries' numHits; capacities: the caller's) and their decode
// into the caller's pages: key = high << 32 | (0xFFFFFFFF - doc), then plan.h: sort_key64_decode; a sentinel ordinal is the
// sort's missing value, reported like every value through doc_value_bits64 (a NaN comes back canonical).
struct Sort64Pages {
  std::vector<nrtgpu_topdocs> pages;
  std::vector<int32_t> docs;
  std::vector<float> highs;
  Sort64Pages(const int32_t* ks, const nrtgpu_fielddocs64* out, int32_t n_queries);
  void decode(const std::vector<DSort64Query>& records, const std::vector<int>& kinds, nrtgpu_fielddocs64* out) const;
};

// termscount.cpp: what the routes that fill count tables share (a text query's hits there; a doc set's in docset.cpp).
// Where the route's own workspace bytes lie (offsets from FinalScoreArgs.own), and what comes back from them.
struct TermsWork {
  int32_t n_queries = 0;
  size_t o_states = 0, o_tables = 0, o_out = 0, bytes = 0;
  uint32_t out_cap = 0;    // entries `out` holds: sum of max_buckets
  std::vector<DTermsState> states;     // terms_collect(): n_queries + 1
  std::vector<uint64_t> entries;       // terms_collect(): states[n_queries].claimed
  void layout(int32_t n_queries, uint64_t slots, uint64_t cap);
};
// what both refuse of (terms[qi], out[qi]) as an invalid argument (out: nullptr for the predicates), the column's kind over the
// leaves, the query's record with its table behind the earlier queries' (*slots, *cap: the call's running sums)
int terms_count_record(const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_terms_count& t, const nrtgpu_term_counts* out, int qi, uint64_t* slots,
                       uint64_t* cap, DTermsQuery* record, int* kind, bool* multi, uint64_t max_call_slots = kTermsMaxCallSlots);
// FinalScoreOwn.collect of both (user: the call's TermsWork): the states, then the entries that exist
int terms_collect(nrtgpu_ctx* ctx, Slot* slot, const char* d_own, void* user);
// the call's answers from what terms_collect brought back and the merge's (empty) lists
int terms_unpack(const TermsWork& work, const std::vector<int>& kinds, const nrtgpu_topdocs* pages, int32_t n_queries, nrtgpu_term_counts* out);

// termscount64.cpp: the same of the routes that fill 64-bit count tables (plan.h: DTermsState64; a slot is a key in one array and
// a count in another, so the compacted entries come back as two lists).
struct TermsWork64 {
  int32_t n_queries = 0;
  size_t o_states = 0, o_keys = 0, o_counts = 0, o_out_codes = 0, o_out_counts = 0, bytes = 0;
  uint32_t out_cap = 0;    // entries the out lists hold: sum of max_buckets
  std::vector<DTermsState64> states;   // terms64_collect(): n_queries + 1
  std::vector<uint64_t> codes;         // terms64_collect(): states[n_queries].claimed entries ...
  std::vector<uint32_t> counts;        // ... and their counts
  void layout(int32_t n_queries, uint64_t slots, uint64_t cap);
};
// terms_count_record over an output of the 64-bit entries, against the bound of kTerms64MaxCallSlots
int terms_count64_record(const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_terms_count& t, const nrtgpu_term_counts64* out, int qi, uint64_t* slots,
                         uint64_t* cap, DTermsQuery* record, int* kind, bool* multi);
// NRTGPU_ERR_UNSUPPORTED with the reason: the count column is a 32-bit one (multi: multi-valued); entry32: the entry that serves it
int terms_count64_narrow(int qi, int32_t field_id, bool multi, const char* entry32);
int terms64_collect(nrtgpu_ctx* ctx, Slot* slot, const char* d_own, void* user);
int terms64_unpack(const TermsWork64& work, const std::vector<int>& kinds, const nrtgpu_topdocs* pages, int32_t n_queries, nrtgpu_term_counts64* out);
// the regions of the route's workspace (d_own: FinalScoreArgs.own) as the launches take them
void terms64_regions(const TermsWork64& w, char* d_own, DTermsState64** states, unsigned long long** keys, uint32_t** counts, unsigned long long** out_codes,
                     uint32_t** out_counts);

// rangecount.cpp: what the routes that count value ranges share (a text query's hits there; a doc set's in docset.cpp).
// The call's records, cut array and interval counters: what goes into the plan buffer (the DRangeCountQuery records, then the
// queries' cuts at the call's column width), the route's own workspace bytes (the uint32 counters), and what comes back from them.
struct RangeWork {
  int32_t n_queries = 0;
  bool wide = false;                        // the call's columns hold 64-bit codes
  size_t bytes = 0;                         // FinalScoreOwn.work_bytes: 4 per counter
  std::vector<int> kinds;                   // per query: range_count_begin()
  std::vector<char> multi;
  std::vector<DRangeCountQuery> records;    // layout(); the caller fills `need`, then seal() copies them into plan_bytes
  std::vector<char> plan_bytes;
  std::vector<uint32_t> counters;           // range_collect()
  void layout(const nrtgpu_range_count* ranges, int32_t n_queries);
  void seal();
  uint32_t interval_of(const DRangeCountQuery& r, uint64_t code) const;   // among r's cuts, at the call's width
};
// what both refuse of (ranges[qi], out[qi]) as an invalid argument (out: nullptr for the predicates); the column's kind and arity
// over the leaves are pushed
int range_count_begin(const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_range_count& r, const nrtgpu_range_counts* out, int qi, RangeWork* work);
// what both refuse of query qi's count column as unsupported, where it is on some leaf: a multi-valued one, a width other than
// an earlier query's
int range_count_column(const RangeWork& work, const nrtgpu_range_count* ranges, int qi);
// the count column on one leaf as the kernels read it (DSortPart.code: the column at the call's width)
DSortPart range_count_column_of(const nrtgpu_seg* seg, int32_t field_id, bool wide);
// FinalScoreOwn.collect of both (user: the call's RangeWork): exactly the counters that exist
int range_collect(nrtgpu_ctx* ctx, Slot* slot, const char* d_own, void* user);
// the roll-up of the interval counters into the ranges, total_hits from the merge's (empty) lists
int range_unpack(const RangeWork& work, const nrtgpu_range_count* ranges, const nrtgpu_topdocs* pages, int32_t n_queries, nrtgpu_range_counts* out);

}  // namespace rt
}  // namespace nrtgpu
