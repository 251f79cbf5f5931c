// knnclauses.cpp -- a text query beside knn clauses (include/nrtgpu.h: nrtgpu_search_text_knn_batch): a request's `query` and its
// resolved `knn` lists scored as ONE BooleanQuery.  The text queries are planned as the exhaustive route plans them (build_plan,
// prune = 0) with the leaves a query lists docs in KEPT (PlanKeepLeaf: a listed doc is a hit also where the leaf holds none of the
// query's terms); beside the plan go the listed docs per (query, leaf) -- sorted leaf-local docids and their knn_sum doubles,
// duplicates across lists merged in list order -- and one DKnnPart per part (plan.h), which bm25_text_knn_kernel
// (knnclauses.hip) reads.  The path from the plan to the caller's pages is finalscore.cpp's.
#include "runtime_internal.h"

namespace nrtgpu {
namespace rt {

namespace {

inline float clause_value(float score, float boost) { return score * boost; }   // DocAndScoreQuery under a BoostQuery: one float multiply

bool has_masks(const nrtgpu_bm25_query& q) { return q.filter_mask != 0 || q.must_not_mask != 0 || q.n_more_filters != 0 || q.n_more_must_not != 0; }

// What the lists themselves say, no leaves and no device needed: the header's INVALID_ARG rows (docids in no leaf aside), then
// the clause values the accumulators cannot hold.
int check_lists(const nrtgpu_bm25_query& q, const nrtgpu_knn_clauses& kc, int qi) {
  if (kc.n_lists < 0 || kc.n_lists > NRTGPU_MAX_KNN_LISTS)
    return fail(NRTGPU_ERR_INVALID_ARG, "query %d: n_lists %d outside 0..%d", qi, kc.n_lists, NRTGPU_MAX_KNN_LISTS);
  if (kc.n_lists > 0 && !kc.lists) return fail(NRTGPU_ERR_INVALID_ARG, "query %d: lists is NULL", qi);
  if (kc.text_nested != 0 && kc.text_nested != 1) return fail(NRTGPU_ERR_INVALID_ARG, "query %d: text_nested must be 0 or 1", qi);
  if (kc.text_nested == 0 && has_masks(q))
    return fail(NRTGPU_ERR_INVALID_ARG, "query %d: a text query with FILTER / MUST_NOT clauses is no pure disjunction: text_nested must be 1", qi);
  std::vector<int32_t> sorted;
  for (int li = 0; li < kc.n_lists; ++li) {
    const nrtgpu_doc_scores& l = kc.lists[li];
    if (l.n < 0 || l.n > NRTGPU_MAX_K) return fail(NRTGPU_ERR_INVALID_ARG, "query %d list %d: n %d outside 0..%d", qi, li, l.n, NRTGPU_MAX_K);
    if (l.n > 0 && (!l.docs || !l.scores)) return fail(NRTGPU_ERR_INVALID_ARG, "query %d list %d: docs / scores is NULL", qi, li);
    if (!std::isfinite(l.boost) || !(l.boost > 0.0f)) return fail(NRTGPU_ERR_INVALID_ARG, "query %d list %d: the boost must be finite and > 0", qi, li);
    for (int i = 0; i < l.n; ++i)
      if (!std::isfinite(l.scores[i])) return fail(NRTGPU_ERR_INVALID_ARG, "query %d list %d: score %d is NaN or infinite", qi, li, i);
    sorted.assign(l.docs, l.docs + l.n);
    std::sort(sorted.begin(), sorted.end());
    for (int i = 1; i < l.n; ++i)
      if (sorted[(size_t)i] == sorted[(size_t)i - 1]) return fail(NRTGPU_ERR_INVALID_ARG, "query %d list %d: doc %d twice", qi, li, sorted[(size_t)i]);
  }
  for (int li = 0; li < kc.n_lists; ++li) {
    const nrtgpu_doc_scores& l = kc.lists[li];
    for (int i = 0; i < l.n; ++i) {
      const float v = clause_value(l.scores[i], l.boost);
      if (!(v > 0.0f) || !std::isfinite(v))   // (the accumulators' 0 means "no match"; Lucene scores are >= 0)
        return fail(NRTGPU_ERR_UNSUPPORTED, "query %d list %d: the clause value of entry %d is <= 0 or overflows", qi, li, i);
    }
  }
  return NRTGPU_OK;
}

// The exactness test (nrtgpu.h): every partial sum of the text clauses' fixed-point values and the lists' values, in any order,
// is a double.  has_text: some text clause matches something (else only the lists count).  1 exact, 0 not.
int sums_exact(const nrtgpu_bm25_query& q, const nrtgpu_knn_clauses& kc, bool has_text, int32_t fx_E) {
  bool any = false;
  int lo = 0;
  double top = 0.0;
  for (int li = 0; li < kc.n_lists; ++li) {
    const nrtgpu_doc_scores& l = kc.lists[li];
    float largest = 0.0f;
    for (int i = 0; i < l.n; ++i) {
      const float v = clause_value(l.scores[i], l.boost);
      const int e = ilogbf(v) - 23;   // the value is a multiple of 2^e
      lo = any ? std::min(lo, e) : e;
      any = true;
      largest = std::max(largest, v);
    }
    top += (double)largest;
  }
  if (!any) return 1;   // the text query alone
  if (has_text) {
    lo = std::min(lo, -(int)fx_E);
    for (int t = 0; t < q.n_terms; ++t) top += (double)q.terms[t].weight;
  }
  int e = 0;
  const double m = frexp(top, &e);   // top = m 2^e, 0.5 <= m < 1
  const int hi = m == 0.5 ? e - 1 : e;   // ceil(log2 top)
  return hi - lo <= 53 ? 1 : 0;
}

// What the route refuses of a call before anything is planned (the segments' content is held).
int check_call(nrtgpu_ctx* ctx, const nrtgpu_bm25_query* queries, const nrtgpu_knn_clauses* knn, int32_t n_queries) {
  for (int qi = 0; qi < n_queries; ++qi) {
    if (int rc = validate_query(queries[qi], qi)) return rc;
    if (int rc = check_lists(queries[qi], knn[qi], qi)) return rc;
  }
  if (int rc = final_score_check_flags(ctx, "text + knn")) return rc;
  for (int qi = 0; qi < n_queries; ++qi) {
    const nrtgpu_bm25_query& q = queries[qi];
    if (q.disjunction_max != 0) return fail(NRTGPU_ERR_UNSUPPORTED, "query %d: knn clauses beside a DisjunctionMaxQuery", qi);
    for (int t = 0; t < q.n_terms; ++t)
      if (q.terms[t].occur != 0) return fail(NRTGPU_ERR_UNSUPPORTED, "query %d: knn clauses beside MUST clauses", qi);
    if (q.min_should_match > 1) return fail(NRTGPU_ERR_UNSUPPORTED, "query %d: knn clauses beside minimumNumberShouldMatch %d", qi, q.min_should_match);
    if (q.min_competitive_score != 0.0f) return fail(NRTGPU_ERR_UNSUPPORTED, "query %d: knn clauses with a min_competitive_score", qi);
  }
  return NRTGPU_OK;
}

// The listed docs of the call, per (query, leaf): leaf-local docids ascending with their knn_sum, the pairs in (query, leaf) order.
struct Staged {
  std::vector<uint32_t> docs;
  std::vector<double> sums;
  std::vector<uint32_t> pair_begin;   // n_queries x n_segs + 1: the pair's entries are [pair_begin[i], pair_begin[i + 1])
  std::vector<PlanKeepLeaf> keep;     // n_queries x n_segs: the tiles that hold the pair's entries
};

int stage_lists(const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs, const nrtgpu_knn_clauses* knn, int32_t n_queries, Staged* out) {
  const size_t n_pairs = (size_t)n_queries * (size_t)std::max(n_segs, 1);
  out->pair_begin.assign(n_pairs + 1, 0u);
  out->keep.assign(n_pairs, PlanKeepLeaf{0u, 0u});
  // the leaves in docBase order: a global docid's leaf is the last one that starts at or below it
  std::vector<int32_t> by_base((size_t)n_segs);
  for (int32_t si = 0; si < n_segs; ++si) by_base[(size_t)si] = si;
  if (doc_bases) std::sort(by_base.begin(), by_base.end(), [&](int32_t a, int32_t b) { return doc_bases[a] < doc_bases[b]; });
  struct Entry { int32_t leaf; uint32_t doc; int32_t list; float value; };
  std::vector<Entry> ents;
  for (int qi = 0; qi < n_queries; ++qi) {
    const nrtgpu_knn_clauses& kc = knn[qi];
    ents.clear();
    for (int li = 0; li < kc.n_lists; ++li) {
      const nrtgpu_doc_scores& l = kc.lists[li];
      for (int i = 0; i < l.n; ++i) {
        if (!doc_bases) return fail(NRTGPU_ERR_INVALID_ARG, "query %d list %d: global docids need doc_bases", qi, li);
        const int32_t doc = l.docs[i];
        auto it = std::upper_bound(by_base.begin(), by_base.end(), doc, [&](int32_t d, int32_t leaf) { return d < doc_bases[leaf]; });
        const int32_t leaf = it == by_base.begin() ? -1 : *(it - 1);
        if (leaf < 0 || (int64_t)doc - (int64_t)doc_bases[leaf] >= (int64_t)segs[leaf]->max_doc)
          return fail(NRTGPU_ERR_INVALID_ARG, "query %d list %d: doc %d lies in no leaf of the call", qi, li, doc);
        ents.push_back(Entry{leaf, (uint32_t)(doc - doc_bases[leaf]), li, clause_value(l.scores[i], l.boost)});
      }
    }
    std::sort(ents.begin(), ents.end(), [](const Entry& a, const Entry& b) {
      return a.leaf != b.leaf ? a.leaf < b.leaf : (a.doc != b.doc ? a.doc < b.doc : a.list < b.list);
    });
    size_t at = 0;
    for (int32_t si = 0; si < std::max(n_segs, 1); ++si) {
      const size_t pair = (size_t)qi * (size_t)std::max(n_segs, 1) + (size_t)si;
      out->pair_begin[pair] = (uint32_t)out->docs.size();
      while (at < ents.size() && ents[at].leaf == si) {
        const uint32_t doc = ents[at].doc;
        double sum = 0.0;   // the doc's lists in list order
        for (; at < ents.size() && ents[at].leaf == si && ents[at].doc == doc; ++at) sum += (double)ents[at].value;
        out->docs.push_back(doc);
        out->sums.push_back(sum);
      }
      const uint32_t b = out->pair_begin[pair], e = (uint32_t)out->docs.size();
      if (e > b) out->keep[pair] = PlanKeepLeaf{out->docs[b] / (uint32_t)kTileDocs, out->docs[e - 1u] / (uint32_t)kTileDocs + 1u};
    }
  }
  out->pair_begin[n_pairs] = (uint32_t)out->docs.size();
  return NRTGPU_OK;
}

// One DKnnPart per part of the plan: the entries of the part's (query, leaf) inside its tile range.
void knn_parts(const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_knn_clauses* knn, const HostPlan& hp, const Staged& st,
               std::vector<DKnnPart>* out) {
  out->assign(hp.parts.size(), DKnnPart{});
  for (const DItem& it : hp.items)
    for (uint32_t pi = 0; pi < it.n_parts; ++pi) {
      const size_t p_at = (size_t)it.part_begin + pi;
      const DPart& p = hp.parts[p_at];
      const int32_t leaf = hp.part_leaf[p_at];
      const size_t pair = (size_t)it.query * (size_t)n_segs + (size_t)leaf;
      const uint32_t* const d0 = st.docs.data();
      const uint32_t b = st.pair_begin[pair], e = st.pair_begin[pair + 1];
      DKnnPart& kp = (*out)[p_at];
      kp.live_bits = segs[leaf]->d_live;
      kp.entry_begin = (uint32_t)(std::lower_bound(d0 + b, d0 + e, p.tile_begin * (uint32_t)kTileDocs) - d0);
      kp.entry_end = (uint32_t)(std::lower_bound(d0 + b, d0 + e, (uint32_t)std::min<uint64_t>((uint64_t)p.tile_end * (uint64_t)kTileDocs, 0xFFFFFFFFull)) - d0);
      kp.nested = (uint32_t)knn[it.query].text_nested;
    }
}

// the scale of query qi's accumulators in the plan; false: the query has no item
bool query_scale(const HostPlan& hp, uint32_t qi, int32_t* fx_E) {
  if (hp.q_nlists[qi] == 0) return false;
  *fx_E = hp.items[hp.list_idx[hp.q_base[qi]]].fx_E;
  return true;
}

int plan_call(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs, const nrtgpu_bm25_query* queries,
              const nrtgpu_knn_clauses* knn, int32_t n_queries, const Staged& st, HostPlan& hp) {
  if (int rc = build_plan(ctx, segs, doc_bases, n_segs, queries, n_queries, hp, 0, st.keep.data())) return rc;
  if (!hp.fixed_point)
    return fail(NRTGPU_ERR_UNSUPPORTED, "text + knn queries need the fixed-point accumulators (the weights of a query in this batch span too many binades)");
  for (int qi = 0; qi < n_queries; ++qi) {
    int32_t fx_E = 0;
    if (!query_scale(hp, (uint32_t)qi, &fx_E)) continue;
    if (!sums_exact(queries[qi], knn[qi], hp.qexpand[(size_t)qi].n_terms != 0, fx_E))
      return fail(NRTGPU_ERR_UNSUPPORTED, "query %d: the lists' values beside the text clauses' span more than 53 bits: the sums are not exact in any order", qi);
  }
  return NRTGPU_OK;
}

}  // namespace
}  // namespace rt
}  // namespace nrtgpu

extern "C" int nrtgpu_text_knn_value(int32_t text_nested, int32_t text_matched, uint64_t fixed_sum, int32_t fx_E, double knn_sum, float* out) {
  if (!out) return fail(NRTGPU_ERR_INVALID_ARG, "NULL argument");
  if (text_nested != 0 && text_nested != 1) return fail(NRTGPU_ERR_INVALID_ARG, "text_nested must be 0 or 1");
  if (text_matched != 0 && (fixed_sum == 0 || fixed_sum >= (1ull << 53))) return fail(NRTGPU_ERR_INVALID_ARG, "a matched doc's fixed-point sum lies in 1..2^53-1");
  if (!(knn_sum >= 0.0) || !std::isfinite(knn_sum)) return fail(NRTGPU_ERR_INVALID_ARG, "knn_sum must be finite and >= 0 (0: no list holds the doc)");
  if (text_matched == 0 && knn_sum == 0.0) return fail(NRTGPU_ERR_INVALID_ARG, "a doc that neither matches the text nor lies in a list has no score");
  *out = text_knn_value((uint32_t)text_nested, text_matched != 0, fixed_sum, fx_E, knn_sum);
  return NRTGPU_OK;
}

extern "C" int nrtgpu_text_knn_exact(const nrtgpu_bm25_query* q, const nrtgpu_knn_clauses* kc, int32_t fx_E) {
  if (!q || !kc) return fail(NRTGPU_ERR_INVALID_ARG, "NULL argument");
  if (q->n_terms < 0 || (q->n_terms > 0 && !q->terms)) return fail(NRTGPU_ERR_INVALID_ARG, "query 0: terms");
  if (int rc = check_lists(*q, *kc, 0)) return rc;
  return sums_exact(*q, *kc, q->n_terms > 0, fx_E);
}

extern "C" int nrtgpu_text_knn_supported(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, int32_t n_segs, const nrtgpu_bm25_query* q,
                                         const nrtgpu_knn_clauses* kc) {
  if (int rc = final_score_enter(ctx, segs, n_segs, !q || !kc, nullptr)) return rc;
  SegReadLocks content(segs, n_segs);
  if (int rc = check_call(ctx, q, kc, 1)) return rc;
  // (without doc_bases the lists' docs name no leaves: the plan is the text query's alone, which answers everything but "a doc
  //  lies in no leaf of the call"; the exactness test runs on the scale that plan gives)
  HostPlan hp;
  Staged none;
  none.keep.assign((size_t)std::max(n_segs, 1), PlanKeepLeaf{0u, 0u});
  return plan_call(ctx, segs, nullptr, n_segs, q, kc, 1, none, hp);
}

extern "C" int nrtgpu_search_text_knn_batch(nrtgpu_ctx* ctx, const nrtgpu_seg* const* segs, const int32_t* doc_bases, int32_t n_segs,
                                            const nrtgpu_bm25_query* queries, const nrtgpu_knn_clauses* knn, int32_t n_queries,
                                            nrtgpu_topdocs* out) {
  if (int rc = final_score_enter(ctx, segs, n_segs, !queries || !knn || !out, &n_queries)) return rc;
  const double t0 = now_ms();
  SegReadLocks content(segs, n_segs);   // until this call's kernels have finished
  if (int rc = check_call(ctx, queries, knn, n_queries)) return rc;
  Staged st;
  if (int rc = stage_lists(segs, doc_bases, n_segs, knn, n_queries, &st)) return rc;
  HostPlan hp;
  if (int rc = plan_call(ctx, segs, doc_bases, n_segs, queries, knn, n_queries, st, hp)) return rc;
  std::vector<DKnnPart> kparts;
  knn_parts(segs, n_segs, knn, hp, st, &kparts);
  const PlanBytes extras[3] = {{kparts.data(), kparts.size() * sizeof(DKnnPart)}, {st.docs.data(), st.docs.size() * 4}, {st.sums.data(), st.sums.size() * 8}};
  return final_score_run(ctx, hp, queries, n_queries, out, t0, extras, 3, [](hipStream_t s, const FinalScoreArgs& a, const void* const* d_extra) {
    launch_bm25_text_knn(s, a, (const DKnnPart*)d_extra[0], (const uint32_t*)d_extra[1], (const double*)d_extra[2]);
  }, nullptr, true);   // (counts the hits behind a cursor per slice: slice_relation_past_kernel)
}
