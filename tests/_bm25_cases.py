"""The cases of tests/test_bm25_edges_gpu.py (a layout sweep) and tests/test_fuzz_bm25_gpu.py (a seeded differential fuzz) over the
two routes of nrtgpu_search_bm25_batch -- the exhaustive scan (csrc/kernels.hip) and the MaxScore walk (csrc/maxscore.hip) -- built
from an explicit layout or a seed.  Pure NumPy plus the oracle, no device: the index (build_index over tests/test_walk_rows_gpu's
segment()), the masks, the requests, and what each request must return -- from oracle.search_bm25 alone, with the accept words of
tests/test_filters_gpu.accept_of.  The layouts, the edge docs and the fuzz sizes are tests/_final_score_cases.py's, imported, not
restated.  tests/test_bm25_cases_host.py checks, without a device, that the cases reach what they are meant for and that the
library takes every one of them.

  clause   (term id, boost) over field 0
  request  Req: the clauses, the page (k, threshold, cursor), the shape (minimumNumberShouldMatch, a DisjunctionMaxQuery's tie
           breaker, MUST flags), one FILTER and one MUST_NOT mask id, a min competitive score from outside
  Model    an index as the oracle sees it; Model.expected(req) the answer; query_of / manager_of: the request as the binding's objects

The terms.  POOL terms 1 - 8 occur in one doc of 2 ... 500, anywhere.  EDGE_TERM occurs in exactly the edge docs of every leaf
(_final_score_cases.EDGE_DOCS: on and next to the 64-doc mask word, the 1024-doc sub-tile and the leaf's end), with a freq of 12 or 17
(the second an escape code) in a doc of 4 tokens: rare, frequent in its doc and the doc short -- whatever else matches, an edge doc
heads the page.  RUN_TERM occurs once in every 7th doc, all of them 30 tokens long: a run of equal scores for a cursor to sit in.
FILLER_TERM is in no query (a leaf of the `gaps` layout keeps it alone), TERM_NOWHERE in no doc.

The relation behind a cursor over several slices.  The reference's collector counts every hit but queues only those behind the
cursor, and its count becomes a lower bound only once ITS queue is full; nrtgpu_search_bm25_batch states another rule
(include/nrtgpu.h: nrtgpu_topdocs.total_hits_is_lower_bound): some slice counted more than
max(totalHitsThreshold, numHits) hits and numHits hits were returned.  The two differ exactly in the set D (Model.in_d), computed
from the oracle alone: a cursor, more than one slice, the oracle returned numHits hits with EQUAL_TO, and some slice's exact count
is above max(threshold, numHits).  In D the expected relation is GREATER_THAN_OR_EQUAL_TO with a count in (max(threshold, numHits),
exact total]; everywhere else the oracle's relation holds and tests/test_parity_gpu.total_ok.

What the generators leave out, because the planner refuses it (planner.cpp): minimumNumberShouldMatch > 1, DisjunctionMax and MUST
clauses without the fixed-point sums; the second-accumulator shapes (a tie breaker > 0, MUST next to SHOULD clauses) with more than
8 clauses, with ScoreMode.COMPLETE, with a min competitive score or under NRTGPU_FLAG_NO_PRUNE (second_accumulator / taken_by)."""
from __future__ import annotations

import dataclasses
import functools
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from nrtsearch_amd import _lib, api, synth
from oracle import oracle

from tests import _final_score_cases as fc
from tests._multi_match_ref import words_of
from tests.test_filters_gpu import accept_of
from tests.test_walk_rows_gpu import segment

f32 = np.float32
INT_MAX = fc.INT_MAX
DEFAULT_SLICING = fc.DEFAULT_SLICING
EDGE_DOCS = fc.EDGE_DOCS
EDGE, SPARSE, DENSE = fc.EDGE, fc.SPARSE, fc.DENSE           # mask ids
MS_MAX_TERMS, MS_WIN_DOCS = 8, 64 * 1024                     # csrc/plan.h: kMsMaxTerms, kMsWinDocs
POOL_EVERY = {1: 2, 2: 3, 3: 5, 4: 9, 5: 20, 6: 50, 7: 150, 8: 500}
EDGE_TERM, RUN_TERM, FILLER_TERM, TERM_NOWHERE = 9, 10, 20, 999_983
QUERY_TERMS = tuple(POOL_EVERY) + (EDGE_TERM, RUN_TERM)
RUN_EVERY, RUN_LENGTH, EDGE_LENGTH = 7, 30, 4
BOOSTS = (1.0, 1.0, 0.5, 2.0, 3.25)
Clause = Tuple[int, float]

NO_PRUNE, NO_MASK_VARIANT, NO_PREFETCH = _lib.NRTGPU_FLAG_NO_PRUNE, _lib.NRTGPU_FLAG_NO_MASK_VARIANT, _lib.NRTGPU_FLAG_NO_PREFETCH
NO_LIVE_FOLD, NO_FIXED_POINT = _lib.NRTGPU_FLAG_NO_LIVE_FOLD, _lib.NRTGPU_FLAG_NO_FIXED_POINT


@dataclasses.dataclass(frozen=True)
class Req:
    clauses: Tuple[Clause, ...]
    k: int = 10
    threshold: int = 1000
    after: Optional[Tuple[int, float]] = None               # (global doc, score)
    min_should_match: int = 0
    dismax: Optional[float] = None                          # the tie breaker of a DisjunctionMaxQuery over the clauses
    must: Tuple[bool, ...] = ()                             # per clause; MUST clauses come first (the order the binding hands over)
    filter: int = 0                                         # mask ids, 0: none
    must_not: int = 0
    min_competitive_score: float = 0.0

    @property
    def terms(self) -> List[int]:
        return [t for t, _ in self.clauses]

    @property
    def mixed_must(self) -> bool:
        return any(self.must) and not all(self.must)

    @property
    def second_accumulator(self) -> bool:
        """planner.cpp: sec_mode_of -- the shapes only the MaxScore kernel carries"""
        return (self.dismax is not None and self.dismax > 0.0) or self.mixed_must

    @property
    def shaped(self) -> bool:
        """what the scan's count-carrying variant and MaxScore's count mode are for"""
        return bool(self.filter or self.must_not or self.min_should_match > 1 or self.dismax is not None or any(self.must))


def describe(r: Req) -> str:
    return ", ".join(f"{f.name}={getattr(r, f.name)!r}" for f in dataclasses.fields(r) if getattr(r, f.name) != f.default)


REFUSED_SECOND_ACCUMULATOR = "run on the MaxScore route only"          # planner.cpp's two messages, as far as they are quoted here
REFUSED_FIXED_POINT = "need the fixed-point accumulators"


def refusal(r: Req, flags: int) -> Optional[str]:
    """The planner's refusals restated (planner.cpp: "... run on the MaxScore route only (<= 8 clauses, fixed-point sums, no
    min_competitive_score, not ScoreMode.COMPLETE ...)", checked first; "minimumNumberShouldMatch > 1 / DisjunctionMaxQuery need the
    fixed-point accumulators ..."): None if a context with these flags takes the request on an index of this module's, else the
    message it refuses it with.  (COMPLETE over few postings would run; the generators never ask.  A conjunction counts as
    minimumNumberShouldMatch = its clauses.)"""
    assert 1 <= len(r.clauses) <= 10 and 1 <= r.k <= 1024 and r.threshold >= 0
    if r.second_accumulator and (flags & (NO_PRUNE | NO_FIXED_POINT) or len(r.clauses) > MS_MAX_TERMS or r.threshold == INT_MAX or r.min_competitive_score != 0.0):
        return REFUSED_SECOND_ACCUMULATOR
    counts_clauses = r.min_should_match > 1 or r.dismax is not None or (bool(r.must) and all(r.must) and len(r.must) > 1)
    if counts_clauses and flags & NO_FIXED_POINT:
        return REFUSED_FIXED_POINT
    return None


def taken_by(r: Req, flags: int) -> bool:
    return refusal(r, flags) is None


def on_maxscore(r: Req, flags: int) -> bool:
    """the requests the planner certainly routes to the MaxScore kernel (planner.cpp: resolve_queries), given one clause matches"""
    return not (flags & (NO_PRUNE | NO_FIXED_POINT)) and len(r.clauses) <= MS_MAX_TERMS and r.min_competitive_score == 0.0 and r.threshold != INT_MAX


# ---- the index ---------------------------------------------------------------------------------------------------------------------------
def edge_flags(sizes) -> np.ndarray:
    flags = np.zeros(int(sum(sizes)), dtype=bool)
    base = 0
    for n in sizes:
        flags[[base + d for d in EDGE_DOCS(n)]] = True
        base += n
    return flags


def build_index(leaf_docs: Sequence[int], seed: int, deletes=0.05, live_none: Sequence[int] = (), without: Sequence[Tuple[int, int]] = ()) -> synth.Corpus:
    """A synth.Corpus over field 0 from explicit leaf sizes.  deletes: the deleted share, one number or one per leaf (edge docs are
    never deleted here: Model.edges_deleted is the copy that deletes exactly them); leaves in live_none carry live_bits=None (their
    share must be 0); without: (leaf, term) pairs whose posting list is left out."""
    leaf_docs = tuple(int(n) for n in leaf_docs)
    n_docs, n_leaves = sum(leaf_docs), len(leaf_docs)
    bases = np.concatenate([[0], np.cumsum(leaf_docs)]).astype(np.int64)
    share = np.asarray(deletes if isinstance(deletes, (tuple, list)) else (deletes,) * n_leaves, dtype=np.float64)
    assert len(share) == n_leaves and all(share[si] == 0.0 for si in live_none)
    rng = np.random.default_rng(seed)
    local = np.concatenate([np.arange(n) for n in leaf_docs])
    edge = edge_flags(leaf_docs)
    run = (local % RUN_EVERY == 3) & ~edge
    deleted = (rng.random(n_docs) < np.repeat(share, leaf_docs)) & ~edge
    # (a mean of 400 tokens beside the few docs of 33 000+: a clause's scores then span less than the 8 binades a fixed-point table holds)
    lengths = np.clip(np.rint(np.exp(rng.normal(np.log(fc.MEAN_LENGTH[0]), 0.5, size=n_docs))), 4, 4000).astype(np.int64)
    n_long = min(9, n_docs)
    lengths[rng.choice(n_docs, n_long, replace=False)] = rng.integers(33_000, 36_000, n_long)     # norm bytes >= 128: escape codes
    lengths[run], lengths[edge] = RUN_LENGTH, EDGE_LENGTH
    norms = synth.int_to_byte4(lengths)
    postings: Dict[int, Tuple[np.ndarray, np.ndarray]] = {}
    for t, every in list(POOL_EVERY.items()) + [(FILLER_TERM, 3)]:
        d = np.nonzero(rng.random(n_docs) < 1.0 / every)[0]
        fr = np.minimum(rng.geometric(0.45, size=len(d)), 20)
        high = rng.random(len(d)) < 0.03
        fr[high] = rng.integers(13, 21, int(high.sum()))                                          # a few certain escapes
        postings[t] = (d, fr.astype(np.int32))
    d = np.nonzero(edge)[0]
    postings[EDGE_TERM] = (d, np.where(np.arange(len(d)) % 2 == 0, 12, 17).astype(np.int32))
    d = np.nonzero(run)[0]
    postings[RUN_TERM] = (d, np.ones(len(d), np.int32))
    without = {(int(a), int(b)) for a, b in without}
    segs, doc_freq = [], {}
    for si, n in enumerate(leaf_docs):
        base, post = int(bases[si]), {}
        for t, (d, fr) in postings.items():
            lo, hi = np.searchsorted(d, [base, base + n])
            if hi > lo and (si, t) not in without:
                post[t] = (d[lo:hi] - base, fr[lo:hi])
                doc_freq[t] = doc_freq.get(t, 0) + int(hi - lo)
        live = None if si in live_none else words_of(~deleted[base: base + n])
        segs.append(segment(n, base, norms[base: base + n].copy(), post, live))
    return synth.Corpus(n_docs=n_docs, doc_count=n_docs, sum_total_term_freq=int(lengths.sum()), segments=segs, doc_freq=doc_freq)


def sweep_masks(sizes, seed: int) -> Dict[int, List[np.ndarray]]:
    """EDGE: exactly the edge docs of every leaf (as a FILTER it accepts only them, as a MUST_NOT it rejects only them); SPARSE 2 %,
    DENSE 97 %"""
    return {EDGE: fc.edge_mask(sizes),
            SPARSE: [synth.random_mask(n, 0.02, seed + 2 * si) for si, n in enumerate(sizes)],
            DENSE: [synth.random_mask(n, 0.97, seed + 2 * si + 1) for si, n in enumerate(sizes)]}


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
class Model:
    """An index as the oracle sees it.  masks: id -> words per leaf."""

    def __init__(self, corpus: synth.Corpus, masks: Dict[int, List[np.ndarray]], slicing=DEFAULT_SLICING, target_items: int = 0):
        self.corpus, self.masks, self.slicing, self.target_items = corpus, masks, tuple(slicing), int(target_items)
        self.segments = corpus.segments
        self.sizes = [seg.max_doc for seg in self.segments]
        self.n_docs = int(sum(self.sizes))
        self.slices = oracle.corpus_slices(corpus, self.slicing)
        self._memo: dict = {}

    def edges_deleted(self) -> "Model":
        """the second copy of the index: the same postings, liveDocs that lose exactly the edge docs of every leaf (a later reader
        version of the same leaves: GpuSegment.fork)"""
        segs = [dataclasses.replace(seg, live_bits=accept_of(seg, None, fc.edge_mask([seg.max_doc])[0]) & words_of(np.ones(seg.max_doc, dtype=bool)))
                for seg in self.segments]
        return Model(dataclasses.replace(self.corpus, segments=segs), self.masks, self.slicing, self.target_items)

    def accept(self, r: Req):
        """liveDocs & FILTER & ~MUST_NOT per leaf as words, or None: the leaves' own liveDocs"""
        if not r.filter and not r.must_not:
            return None
        return [accept_of(seg, self.masks[r.filter][si] if r.filter else None, self.masks[r.must_not][si] if r.must_not else None)
                for si, seg in enumerate(self.segments)]

    def _oracle(self, r: Req, k: Optional[int] = None, **over):
        kw = dict(boosts=[b for _, b in r.clauses], after=r.after, total_hits_threshold=r.threshold, accept=self.accept(r),
                  min_should_match=r.min_should_match, dismax=r.dismax, must=list(r.must) if r.must else None, slicing=self.slicing)
        kw.update(over)
        return oracle.search_bm25(self.corpus, r.terms, r.k if k is None else k, **kw)

    def oracle(self, r: Req):
        """oracle.search_bm25 of the request as it stands (a min competitive score aside) -> (docs, scores, total_hits, relation_gte)"""
        key = ("oracle", r)
        if key not in self._memo:
            self._memo[key] = self._oracle(r)
        return self._memo[key]

    def slice_counts(self, r: Req) -> List[int]:
        """per searcher slice the exact number of hits (a collector counts every hit, behind the cursor or not)"""
        key = ("slices", dataclasses.replace(r, k=1, threshold=INT_MAX, after=None, min_competitive_score=0.0))
        if key not in self._memo:
            self._memo[key] = [self._oracle(r, k=1, after=None, total_hits_threshold=INT_MAX, segments=list(g), slicing=None)[2] for g in self.slices]
        return self._memo[key]

    def in_d(self, r: Req) -> bool:
        """the requests on which the library's stated rule and the reference's differ (the module's docstring)"""
        if r.after is None or len(self.slices) < 2 or r.threshold == INT_MAX:
            return False
        docs, _, _, gte = self.oracle(r)
        return len(docs) == r.k and not gte and max(self.slice_counts(r)) > max(r.threshold, r.k)

    def expected(self, r: Req):
        """-> (docs, scores, exact total_hits, relation_gte); read-only, computed once per request"""
        key = ("expected", r)
        if key not in self._memo:
            docs, scores, total, gte = self.oracle(r)
            if r.min_competitive_score > 0.0:   # counted, not collected: the docs strictly below the bound (threshold INT_MAX: an exact count)
                assert r.threshold == INT_MAX and r.after is None
                keep = scores >= f32(r.min_competitive_score)
                docs, scores = docs[keep], scores[keep]
            self._memo[key] = (docs, scores, total, True if self.in_d(r) else gte)
        return self._memo[key]

    def matches_something(self, r: Req) -> bool:
        return any(self.corpus.doc_freq.get(t, 0) > 0 for t in r.terms)


# ---- the same request as the binding's objects -------------------------------------------------------------------------------------------
def query_of(r: Req):
    cl = tuple(api.TermQuery(0, t) if b == 1.0 else api.BoostQuery(api.TermQuery(0, t), float(b)) for t, b in r.clauses)
    f = (api.MaskFilter(r.filter),) if r.filter else ()
    mn = (api.MaskFilter(r.must_not),) if r.must_not else ()
    if r.dismax is not None:
        dq = api.DisjunctionMaxQuery(cl, float(r.dismax))
        return dq if not (f or mn) else api.BooleanQuery(must=(dq,), filter=f, must_not=mn)
    if any(r.must):
        return api.BooleanQuery(tuple(c for c, m_ in zip(cl, r.must) if not m_), 0, f, mn, tuple(c for c, m_ in zip(cl, r.must) if m_))
    if len(cl) == 1 and not f and not mn and r.min_should_match == 0:
        return cl[0]
    # (with a FILTER clause the SHOULD clauses are optional unless one must match: minimumNumberShouldMatch 1 is the plain disjunction)
    return api.BooleanQuery(cl, max(r.min_should_match, 1 if f else 0), f, mn)


def manager_of(r: Req):
    return api.TopScoreDocCollectorManager(r.k, None if r.after is None else api.ScoreDoc(int(r.after[0]), float(r.after[1])), r.threshold,
                                           float(r.min_competitive_score))


# ---- building blocks of requests ---------------------------------------------------------------------------------------------------------
def plain(terms, boosts=None, **kw) -> Req:
    return Req(tuple((int(t), float(1.0 if boosts is None else boosts[i])) for i, t in enumerate(terms)), **kw)


def with_must(terms, must, boosts=None, **kw) -> Req:
    """MUST clauses first, as the binding hands them over"""
    order = [i for i, m_ in enumerate(must) if m_] + [i for i, m_ in enumerate(must) if not m_]
    return plain([terms[i] for i in order], None if boosts is None else [boosts[i] for i in order], must=tuple(bool(must[i]) for i in order), **kw)


def next_page(m: Model, r: Req, at: Optional[int] = None) -> Optional[Req]:
    """the request again with `after` = a hit of its own first page (the last one unless `at` says which)"""
    docs, scores = m.expected(r)[:2]
    if len(docs) == 0:
        return None
    at = len(docs) - 1 if at is None else at
    return dataclasses.replace(r, after=(int(docs[at]), float(scores[at])))


def whole_list(m: Model, r: Req):
    """every hit of the request in rank order (at most 1024 of them, asserted)"""
    docs, scores, total, _ = m.expected(dataclasses.replace(r, k=1024, threshold=INT_MAX, after=None))
    assert total == len(docs), (total, describe(r))
    return docs, scores


# ---- the layout sweep --------------------------------------------------------------------------------------------------------------------
WINDOW_EDGES = (MS_WIN_DOCS - 1, MS_WIN_DOCS, MS_WIN_DOCS + 1)          # a MaxScore window's last doc, a full one, one doc in the next
SINGLE_LEAF = fc.SINGLE_LEAF + WINDOW_EDGES
MULTI_LEAF = fc.MULTI_LEAF
LAYOUTS = SINGLE_LEAF + MULTI_LEAF
SLICE_LAYOUTS = tuple(l for l in MULTI_LEAF if l.endswith("_slices"))
GAPS_ABSENT = fc.GAPS_ABSENT
T3 = (EDGE_TERM, 2, 5)
T8 = (EDGE_TERM, 1, 2, 3, 4, 5, 6, 2)
T10 = (EDGE_TERM, 1, 2, 3, 4, 5, 6, 7, 8, 2)
SLICE_TERM, SLICE_K, SLICE_THRESHOLD = 5, 30, 10                        # the *_slices cursors: about 51 hits per 1025-doc slice


def layout_of(layout) -> dict:
    """_final_score_cases.layout_of's sizes, deletes and slicing; `without` in this module's (leaf, term) pairs; target_items = 1
    for the *_slices layouts: the cost cuts no item, the slice slots do"""
    spec = fc.layout_of(layout)
    spec["without"] = [(si, t) for si in GAPS_ABSENT for t in QUERY_TERMS] if layout == "gaps" else []
    if layout in SLICE_LAYOUTS:
        spec["target_items"] = 1
    return spec


@functools.lru_cache(maxsize=2)
def sweep_case(layout):
    """-> (model, [Req], {mark: index of the request})"""
    li = LAYOUTS.index(layout)
    spec = layout_of(layout)
    corpus = build_index(spec["leaf_docs"], 7000 + li, spec["deletes"], spec["live_none"], spec["without"])
    m = Model(corpus, sweep_masks(spec["leaf_docs"], 8000 + 100 * li), spec["slicing"], spec["target_items"])
    return (m,) + sweep_requests(m)


def sweep_requests(m: Model):
    """the sweep's requests over one model (its masks: sweep_masks) -> ([Req], marks).  Marks: "edge" a page an edge doc heads,
    "edge_filter" / "edge_must_not" the EDGE mask both ways, "run" the cursor inside a run of equal scores, "in_d" / "not_in_d" the
    *_slices cursors."""
    reqs: List[Req] = []
    marks: Dict[str, int] = {}

    def add(r: Optional[Req], mark: Optional[str] = None):
        if r is None:
            return None
        if mark:
            marks[mark] = len(reqs)
        reqs.append(r)
        return r

    hits = m.expected(plain(T3, k=1, threshold=INT_MAX))[2]
    below, above = hits // 2, hits + 1                                   # thresholds on both sides of the layout's hit count
    # plain disjunctions of 3 and 8 clauses: every k, thresholds on both sides and COMPLETE
    for i, (k, thr) in enumerate(((64, below), (1, below), (64, above), (1000, INT_MAX), (1024, below), (64, INT_MAX), (1, above), (1000, 0))):
        add(plain(T3, k=k, threshold=thr), "edge" if i == 0 else None)
    for k, thr in ((64, below), (1000, above), (1024, INT_MAX), (1, 1000)):
        add(plain(T8, k=k, threshold=thr))
    add(plain(T3, (2.0, 0.5, 3.25), k=64, threshold=below))
    add(plain((2,), k=64, threshold=below))
    add(plain((TERM_NOWHERE,), k=64))
    add(plain((TERM_NOWHERE, 2), k=64, threshold=below))
    add(plain(T10, k=64, threshold=below))                               # 9 and 10 clauses: the scan whatever the flags
    add(plain(T10[:9], k=1000, threshold=INT_MAX, min_should_match=2))
    # minimumNumberShouldMatch 2
    add(plain(T3, k=64, threshold=below, min_should_match=2))
    add(plain(T8, k=1000, threshold=INT_MAX, min_should_match=2))
    add(plain(T8, k=1, threshold=above, min_should_match=3))
    # DisjunctionMax, tie breakers 0 and 0.3
    for terms, tie, k, thr in ((T3, 0.0, 64, below), (T3, 0.3, 64, below), (T3, 0.3, 1024, above), (T8, 0.0, 1000, INT_MAX), (T8, 0.3, 1, below)):
        add(plain(terms, k=k, threshold=thr, dismax=tie))
    # a MUST clause next to SHOULD clauses; the conjunction
    add(with_must(T3, (False, True, False), k=64, threshold=below))
    add(with_must(T3, (True, False, False), k=1000, threshold=above))    # MUST the edge term: the hits are edge docs
    add(with_must(T8, (False, True, True, False, False, False, False, False), k=64, threshold=below))
    add(with_must((2, 3), (True, True), k=64, threshold=INT_MAX))
    # masks: EDGE both ways, a dense and a sparse random one
    add(plain(T3, k=64, threshold=below, filter=EDGE), "edge_filter")
    add(plain(T3, k=64, threshold=below, must_not=EDGE), "edge_must_not")
    add(plain(T8, k=1024, threshold=INT_MAX, filter=EDGE))
    add(plain(T8, k=1000, threshold=above, must_not=EDGE))
    add(plain(T3, k=64, threshold=below, filter=DENSE))
    add(plain(T3, k=1000, threshold=0, filter=SPARSE))
    add(plain(T8, k=64, threshold=below, filter=DENSE, must_not=SPARSE))
    add(plain(T3, k=64, threshold=below, min_should_match=2, filter=EDGE))
    add(plain(T3, k=64, threshold=below, dismax=0.3, must_not=EDGE))
    add(plain(T3, k=64, threshold=below, dismax=0.0, filter=DENSE))
    add(with_must(T3, (False, True, False), k=64, threshold=below, must_not=SPARSE))
    # thresholds ON the boundary: the exact count of the request's largest slice (nothing is above it: EQUAL_TO) and one below it (a
    # lower bound) -- plain (the planner's certain bound), behind a mask and with a minimum (MaxScore's count mode)
    for i, r in enumerate((plain(T3, k=1), plain(T3, k=1, filter=DENSE), plain(T8, k=64, min_should_match=2))):
        top = max(m.slice_counts(r))
        add(dataclasses.replace(r, threshold=top), "at_count" if i == 1 else None)
        add(dataclasses.replace(r, threshold=max(top - 1, 0)), "below_count" if i == 1 else None)
    # a min competitive score from outside: a score of the request's own page
    whole = plain(T3, k=64, threshold=INT_MAX)
    top = m.expected(whole)[1]
    if len(top) >= 2:
        add(dataclasses.replace(whole, min_competitive_score=float(top[len(top) // 2])))
    # page 2 behind a cursor inside the planted run of equal scores: the first hit whose successor scores the same
    run = plain((RUN_TERM, 6), k=64, threshold=below)
    docs, scores = m.expected(dataclasses.replace(run, k=1024, threshold=INT_MAX))[:2]
    same = np.nonzero(scores[:-1].view(np.uint32) == scores[1:].view(np.uint32))[0]
    if len(same):
        at = int(same[min(2, len(same) - 1)])
        add(dataclasses.replace(run, after=(int(docs[at]), float(scores[at]))), "run")
    # the second page of every cursor-free request with k = 64 that fills its first
    for r in list(reqs):
        if r.after is None and r.k == 64 and r.min_competitive_score == 0.0 and len(m.expected(r)[0]) == 64:
            add(next_page(m, r))
    # *_slices: a cursor page inside D (about 10 hits per slice lie behind the cursor, 80 and more together) and one outside it
    if len(m.slices) >= 8:
        base = plain((SLICE_TERM,), k=SLICE_K, threshold=SLICE_THRESHOLD)
        docs, scores = whole_list(m, base)
        at = len(docs) - 10 * len(m.slices) - 1
        add(dataclasses.replace(base, after=(int(docs[at]), float(scores[at]))), "in_d")
        add(dataclasses.replace(base, after=(int(docs[2]), float(scores[2]))), "not_in_d")
        shaped = dataclasses.replace(base, filter=DENSE)                 # the same behind a mask: MaxScore's count mode
        docs, scores = whole_list(m, shaped)
        at = len(docs) - 10 * len(m.slices) - 1
        add(dataclasses.replace(shaped, after=(int(docs[at]), float(scores[at]))), "in_d_shaped")
    return reqs, marks


def edges_deleted_requests(m: Model) -> List[Req]:
    """what the copy without its edge docs is asked (no masks: a forked leaf carries liveDocs of its own, nothing else)"""
    hits = m.expected(plain(T3, k=1, threshold=INT_MAX))[2]
    return [plain(T3, k=64, threshold=hits // 2), plain(T3, k=1024, threshold=INT_MAX), plain(T8, k=64, threshold=hits // 2),
            plain(T8, k=1000, threshold=INT_MAX, min_should_match=2), plain(T3, k=64, threshold=hits // 2, dismax=0.0), plain(T10, k=64, threshold=hits // 2)]


# ---- the fuzz ----------------------------------------------------------------------------------------------------------------------------
FUZZ_SIZES = fc.FUZZ_SIZES + (40_000, 65_537)
FUZZ_MAX_DOCS = 150_000
FUZZ_SLICINGS = (DEFAULT_SLICING, (2000, 2), (500, 1), (20_000, 2))
FUZZ_TARGET_ITEMS = (0, 1, 64)
FUZZ_BUDGETS = (-1, 2, 0, 100000)
# (in this order: of the default rounds' two with (2000, 2) and two with (500, 1), one keeps the MaxScore route and two the scan)
FUZZ_FLAGS = (0, NO_LIVE_FOLD, NO_PRUNE, NO_PRUNE | NO_MASK_VARIANT, NO_PRUNE | NO_PREFETCH, NO_FIXED_POINT, NO_PRUNE | NO_LIVE_FOLD)
BIG_LEAVES = tuple(n for n in FUZZ_SIZES if n > 2000)                   # under (2000, 2) each a slice of its own
FUZZ_TERMS = tuple(POOL_EVERY) + tuple(POOL_EVERY)[:5] + (EDGE_TERM, RUN_TERM, TERM_NOWHERE)
FUZZ_MASKS = {SPARSE: 0.02, DENSE: 0.4, 7: 0.97}                       # and EDGE
CURSOR_SHARE = {False: 0.25, True: 0.3}                              # by "the round has more than one slice": D stays the exception


@dataclasses.dataclass(frozen=True)
class Knobs:
    """the context of a fuzz round"""
    flags: int
    packed: bool
    budget_pct: int

    @property
    def context_flags(self) -> int:
        return self.flags | (_lib.NRTGPU_FLAG_PACKED_POSTINGS if self.packed else 0)


def _pick(rng, seq):
    return seq[int(rng.integers(len(seq)))]


def _fuzz_model(rng, round_: int) -> Model:
    """The context's knobs follow the round's number, each with a period of its own, so that a handful of rounds holds every one of
    them (the flag sets: 7, the slicings: 4, the budgets: 4, shifted by one every four rounds, target_items: 3, the posting layouts:
    2); what the index holds is drawn.  The two slicings that can cut 12 leaves into nine slices are made to: one leaf per slice
    ((500, 1)) draws 9 - 12 leaves; (2000, 2) draws, in every other round of its own, 12 leaves of which 7 are above 2000 docs (a
    slice each) and 5 at most 1025 docs long (two to a slice), in any order: nine slices and more of which some hold two leaves --
    where the item cut at the ninth slice and the re-joined remainder are not "one leaf per part"."""
    slicing = FUZZ_SLICINGS[round_ % 4]
    sizes: List[int] = []
    if slicing == (2000, 2) and (round_ // 4) % 2 == 0:
        for i in range(12):
            pool = [n for n in (BIG_LEAVES if i < 7 else FUZZ_SIZES) if (n > 2000) == (i < 7)]
            room = FUZZ_MAX_DOCS - sum(sizes) - min(BIG_LEAVES) * max(0, 6 - i) - 1025 * min(5, 11 - i)   # (what the leaves still to come need)
            sizes.append(int(_pick(rng, [n for n in pool if n <= room])))
        sizes = [sizes[i] for i in rng.permutation(12)]
    else:
        for _ in range(int(rng.integers(9 if slicing == (500, 1) else 1, 13))):
            fit = [n for n in FUZZ_SIZES if sum(sizes) + n <= FUZZ_MAX_DOCS]
            sizes.append(int(_pick(rng, fit)))
    share = float(_pick(rng, (0.0, 0.0, 0.03, 0.3)))
    live_none = [si for si in range(len(sizes)) if rng.random() < (0.5 if share == 0.0 else 0.25)]
    deletes = [0.0 if si in live_none else share for si in range(len(sizes))]
    without = [(si, int(t)) for si in range(len(sizes)) for t in QUERY_TERMS if rng.random() < 0.1]
    corpus = build_index(sizes, int(rng.integers(1 << 30)), deletes, live_none, without)
    masks = {mid: [synth.random_mask(n, dens, int(rng.integers(1 << 30))) for n in sizes] for mid, dens in FUZZ_MASKS.items()}
    masks[EDGE] = fc.edge_mask(sizes)
    return Model(corpus, masks, slicing, FUZZ_TARGET_ITEMS[round_ % 3])


def _fuzz_request(rng, m: Model, flags: int) -> Req:
    """drawn like tests/test_fuzz_gpu.py::test_fuzz_query_shapes draws, with its legality rules"""
    fixed = not flags & NO_FIXED_POINT
    nt = int(rng.integers(1, 11))
    terms = [int(_pick(rng, FUZZ_TERMS)) for _ in range(nt)]
    boosts = [float(_pick(rng, BOOSTS)) for _ in terms]
    k = int(_pick(rng, (1, 7, 30, 64, 300, 1000, 1024)))
    thr = int(_pick(rng, (1000, 1000, 10, 0, INT_MAX)))
    msm = int(rng.integers(2, nt + 2)) if (fixed and nt > 1 and rng.random() < 0.35) else 0
    kw: dict = dict(filter=int(_pick(rng, (0, 0, 0) + tuple(m.masks))), must_not=int(_pick(rng, (0, 0, 0, 0) + tuple(m.masks))))
    dismax = fixed and msm == 0 and rng.random() < 0.25
    # the second-accumulator shapes: the MaxScore route only
    two_ok = fixed and not flags & NO_PRUNE and nt <= MS_MAX_TERMS and thr != INT_MAX
    must = None
    if dismax:
        kw["dismax"] = float(f32(_pick(rng, (0.05, 0.3, 0.5, 1.0)))) if two_ok and rng.random() < 0.6 else 0.0
    elif fixed and nt >= 2 and msm == 0 and rng.random() < 0.3:
        must = [bool(x) for x in rng.integers(0, 2, size=nt)]
        if not two_ok:
            must = [True] * nt                                              # the conjunction: one accumulator
        elif all(must) or not any(must):
            must[0], must[1] = True, False
    r = with_must(terms, must, boosts, k=k, threshold=thr, **kw) if must else plain(terms, boosts, k=k, threshold=thr, min_should_match=msm, **kw)
    if not r.second_accumulator and rng.random() < 0.06:                 # a bound from outside: a score of the request's own page, an exact count
        r = dataclasses.replace(r, threshold=INT_MAX)
        scores = m.expected(r)[1]
        if len(scores):
            return dataclasses.replace(r, min_competitive_score=float(scores[int(rng.integers(len(scores)))]))
    if rng.random() < CURSOR_SHARE[len(m.slices) > 1]:
        # a cursor from the oracle's own ranking: a hit of the first page; any of the first 1024 hits (the last hit of some earlier
        # page); or the hit that leaves one full page and at most two hits more behind it (of those 1024: the last full page)
        where = int(_pick(rng, (0, 0, 1, 1, 2)))
        docs, scores = m.expected(r if where == 0 else dataclasses.replace(r, k=1024, threshold=INT_MAX))[:2]
        if len(docs):
            at = int(rng.integers(len(docs)))
            if where == 2 and len(docs) > k:
                at = max(0, len(docs) - k - 1 - int(rng.integers(3)))
            r = dataclasses.replace(r, after=(int(docs[at]), float(scores[at])))
    return r


@functools.lru_cache(maxsize=2)
def fuzz_round(base: int, round_: int):
    """-> (model, knobs, [[Req]]): three batches of 8-32 requests, every shape mixed inside a batch.  Replay one case:
    fuzz_round(base, round_)[2][batch][index]."""
    rng = np.random.Generator(np.random.PCG64(base + round_))
    knobs = Knobs(flags=FUZZ_FLAGS[round_ % len(FUZZ_FLAGS)], packed=round_ % 8 >= 4, budget_pct=FUZZ_BUDGETS[(round_ + round_ // 4) % 4])
    m = _fuzz_model(rng, round_)
    return m, knobs, [[_fuzz_request(rng, m, knobs.flags) for _ in range(int(rng.integers(8, 33)))] for _ in range(3)]
