"""The cases of tests/test_final_score_edges_gpu.py (a layout sweep) and tests/test_fuzz_final_score_gpu.py (a seeded differential
fuzz) over the four routes on csrc/finalscore.hiph's skeleton -- search_function_score_batch, search_multi_match_batch,
search_function_score_multi_match_batch, search_text_knn_batch -- built from a seed or an explicit layout.  Pure NumPy, no device:
the index (build_fields: tests/_multi_match_ref.build_index's recipe with the sizes as arguments), the masks, the requests, and what
each request must return, from the four references (tests/_function_score_ref.py, _multi_match_ref.py,
_function_score_multi_match_ref.py, _text_knn_ref.py; nothing of them is restated here).  tests/test_final_score_cases_host.py
checks, without a device, that the cases reach the paths they are meant for and that the routes take every one of them.

  clause   (field, term id, boost)
  request  Req: the entry, the clauses in groups (function_score / text_knn: ONE group over field 0, a SHOULD disjunction), the
           functions, the masks, the knn lists, the page
  Model    an index as the references see it, Model.expected(req) the reference's answer; query_of / manager_of / knn_clauses_of:
           the same request as the binding's objects

The layout numbers are csrc/plan.h's: 64-doc mask words, kTileDocs = 1024-doc sub-tiles, rounds of 12 sub-tiles (funcscore.hip,
knnclauses.hip; 3072 candidate slots) or 8 (multimatch.hip; 2048), kSliceSlots = 8 searcher slices per item, at most 32 clauses, 8
groups, 4 scored fields, 8 functions, k <= 1024.

What the generator leaves out, because the routes refuse it: negative weights, MUST or minimum_should_match > 1 inside a
function-score or text + knn inner query, MUST next to SHOULD inside a group, more than 4 fields / 32 clauses / 8 groups, packed and
no-fixed-point contexts -- and the term in every doc beside other terms, for the reason tests/_column_cases.py gives: the terms
come from _multi_match_ref.TERM_EVERY (one doc in 2 ... 500) and the boosts from a pool three binades wide, which keeps a query's
clause weights within the fixed-point range."""
from __future__ import annotations

import dataclasses
import functools
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from nrtsearch_amd import api, synth
from oracle import oracle

from tests import _function_score_multi_match_ref as fsmm_ref
from tests import _function_score_ref as fs_ref
from tests import _multi_match_ref as mm_ref
from tests import _text_knn_ref as tk_ref

f32 = np.float32
INT_MAX = 2**31 - 1
WORD_DOCS, TILE_DOCS, SLICE_SLOTS = 64, 1024, 8                         # csrc/plan.h
ENTRIES = ("function_score", "multi_match", "function_score_multi_match", "text_knn")
ROUND_TILES = {"function_score": 12, "multi_match": 8, "function_score_multi_match": 8, "text_knn": 12}
CAND_CAP = {"function_score": 3072, "multi_match": 2048, "function_score_multi_match": 2048, "text_knn": 3072}
DEFAULT_SLICING = oracle.DEFAULT_SLICING
TERM_EVERY = mm_ref.TERM_EVERY
TERM_NOWHERE = mm_ref.TERM_NOWHERE
MEAN_LENGTH = (400.0, 150.0, 90.0, 60.0)                                # per field
MODE_PAIRS = tuple((s, b) for s in ("multiply", "sum") for b in ("multiply", "sum", "replace"))
BOOSTS = (1.0, 1.0, 0.5, 2.0, 3.25)
WEIGHTS = (0.25, 0.3, 0.5, 0.75, 1.25, 1.5, 2.5, 3.0, 7.0, 11.0)        # the pools of test_function_score_gpu.py / test_multi_match_gpu.py
Clause = Tuple[int, int, float]
KnnList = Tuple[Tuple[int, ...], Tuple[float, ...], float]              # (global docids, scores, boost)


def EDGE_DOCS(max_doc: int) -> List[int]:
    """the docs of a leaf on and next to the mask word, the sub-tile and the leaf's end"""
    return sorted({d for d in (0, 62, 63, 64, 65, 1022, 1023, 1024, 1025, max_doc - 2, max_doc - 1) if 0 <= d < max_doc})


@dataclasses.dataclass(frozen=True)
class Req:
    entry: str                                              # one of ENTRIES
    groups: Tuple[Tuple[Clause, ...], ...] = ()
    shape: str = "cross_fields"                             # the two multi-match entries
    operator: str = "should"
    msm: object = 0                                         # an int; best_fields also a tuple, one minimum per group
    tie_breaker: float = 0.0
    functions: Tuple[Tuple[int, float], ...] = ()           # the two function-score entries: (mask id or 0, weight)
    score_mode: str = "multiply"
    boost_mode: str = "multiply"
    min_score: float = 0.0
    min_excluded: bool = False
    filter: Tuple[int, ...] = ()                            # mask ids
    must_not: Tuple[int, ...] = ()
    lists: Tuple[KnnList, ...] = ()                         # text_knn
    k: int = 10
    threshold: int = 1000
    after: Optional[Tuple[int, float]] = None               # (global doc, score)

    @property
    def clauses(self) -> Tuple[Clause, ...]:
        return tuple(c for g in self.groups for c in g)

    @property
    def nested(self) -> bool:
        """text_knn: a text query with FILTER / MUST_NOT clauses is no pure disjunction and stays one clause"""
        return bool(self.filter or self.must_not)

    @property
    def grouped(self) -> bool:
        return self.entry.endswith("multi_match")

    @property
    def scored(self) -> bool:
        return self.entry.startswith("function_score")


def describe(r: Req) -> str:
    def short(name, v):
        if name == "lists":
            return "[" + ", ".join(f"{len(d)} docs x {b}" for d, _, b in v) + "]"
        return repr(v)
    return ", ".join(f"{f.name}={short(f.name, getattr(r, f.name))}" for f in dataclasses.fields(r) if getattr(r, f.name) != f.default)


# ---- the index ---------------------------------------------------------------------------------------------------------------------------
def build_fields(leaf_docs: Sequence[int], n_fields: int, seed: int, deletes=0.05, live_none: Sequence[int] = (),
                 without: Sequence[Tuple[int, int, int]] = ()) -> list:
    """[synth.Corpus per field] over the same leaves.  deletes: the deleted share, one number or one per leaf; leaves in live_none
    carry live_bits=None (their share must be 0).  Terms 1-3 are in every edge doc of every leaf, the others in none of them.
    Field 0 holds a few docs of 33 000+ tokens (norm byte >= 128: escape codes), also at each leaf's first and last doc, where
    terms 1-3 have freqs above 12 (escape codes too).  without: (leaf, field, term) triples whose posting list is left out."""
    leaf_docs = tuple(int(n) for n in leaf_docs)
    n_docs, n_leaves = sum(leaf_docs), len(leaf_docs)
    bases = np.concatenate([[0], np.cumsum(leaf_docs)]).astype(np.int64)
    share = np.asarray(deletes if isinstance(deletes, (tuple, list)) else (deletes,) * n_leaves, dtype=np.float64)
    assert len(share) == n_leaves and all(share[si] == 0.0 for si in live_none)
    rng = np.random.default_rng(seed)
    deleted = rng.random(n_docs) < np.repeat(share, leaf_docs)
    first, last = bases[:-1], bases[1:] - 1
    edge = np.array(sorted({int(b) + d for b, n in zip(bases[:-1], leaf_docs) for d in EDGE_DOCS(n)}), dtype=np.int64)
    without = {(int(a), int(b), int(c)) for a, b, c in without}
    fields = []
    for fi in range(n_fields):
        lengths = np.clip(np.rint(np.exp(rng.normal(np.log(MEAN_LENGTH[fi]), 0.5, size=n_docs))), 4, 4000).astype(np.int64)
        if fi == 0:
            n_long = min(9, n_docs)
            lengths[rng.choice(n_docs, n_long, replace=False)] = rng.integers(33_000, 36_000, n_long)
            lengths[first] = lengths[last] = 34_000
        norms = synth.int_to_byte4(lengths)
        postings: Dict[int, Tuple[np.ndarray, np.ndarray]] = {}
        for t, every in TERM_EVERY.items():
            has = rng.random(n_docs) < 1.0 / every
            has[edge] = t <= 3
            d = np.nonzero(has)[0]
            fr = np.minimum(rng.geometric(0.45, size=len(d)), 20)
            high = rng.random(len(d)) < 0.03
            fr[high] = rng.integers(13, 21, int(high.sum()))                          # a few certain escapes
            if fi == 0 and t <= 3:
                fr[np.isin(d, first)] = 13 + t
                fr[np.isin(d, last)] = 17 + t
            postings[t] = (d, fr.astype(np.int32))
        segs, doc_freq = [], {t: 0 for t in postings}
        for si, n in enumerate(leaf_docs):
            base = int(bases[si])
            ids, offs, dd, ff = [], [0], [], []
            for t in sorted(postings):
                d, fr = postings[t]
                lo, hi = np.searchsorted(d, [base, base + n])
                if hi == lo or (si, fi, t) in without:
                    continue
                ids.append(t)
                dd.append(d[lo:hi] - base)
                ff.append(fr[lo:hi])
                offs.append(offs[-1] + int(hi - lo))
                doc_freq[t] += int(hi - lo)
            assert ids, "a leaf without a single posting"
            live = None if si in live_none else mm_ref.words_of(~deleted[base: base + n])
            segs.append(synth.SegmentData(max_doc=n, doc_base=base, norms=norms[base: base + n].copy(), term_ids=np.array(ids, np.int64),
                                          offsets=np.array(offs, np.int64), docids=np.concatenate(dd).astype(np.int32),
                                          freqs=np.concatenate(ff).astype(np.int32), live_bits=live))
        fields.append(synth.Corpus(n_docs=n_docs, doc_count=n_docs, sum_total_term_freq=int(lengths.sum()), segments=segs, doc_freq=doc_freq))
    return fields


# ---- masks -------------------------------------------------------------------------------------------------------------------------------
EDGE, THIRD, SPARSE, DENSE, LASTWORD = 3, 4, 5, 6, 8       # the sweep's mask ids
FUZZ_MASKS = {5: 0.02, 6: 0.4, 7: 0.97}                    # the fuzz's: id -> density; and EDGE


def _words(n: int, docs) -> np.ndarray:
    flags = np.zeros(n, dtype=bool)
    flags[np.asarray(docs, dtype=np.int64)] = True
    return mm_ref.words_of(flags)


def edge_mask(sizes) -> List[np.ndarray]:
    return [_words(n, EDGE_DOCS(n)) for n in sizes]


def sweep_masks(sizes, seed: int) -> Dict[int, List[np.ndarray]]:
    """EDGE: the edge docs of every leaf; THIRD: every third doc; SPARSE 2 %, DENSE 97 %; LASTWORD: set only in the last word of
    every leaf (all of its docs)."""
    return {EDGE: edge_mask(sizes),
            THIRD: [_words(n, np.arange(0, n, 3)) for n in sizes],
            SPARSE: [synth.random_mask(n, 0.02, seed + 2 * si) for si, n in enumerate(sizes)],
            DENSE: [synth.random_mask(n, 0.97, seed + 2 * si + 1) for si, n in enumerate(sizes)],
            LASTWORD: [_words(n, np.arange((n - 1) // WORD_DOCS * WORD_DOCS, n)) for n in sizes]}


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
class Model:
    """An index as the references see it.  fields: [synth.Corpus per field]; masks: id -> words per leaf."""

    def __init__(self, fields, masks: Dict[int, List[np.ndarray]], slicing=DEFAULT_SLICING, target_items: int = 0):
        self.fields, self.masks, self.slicing, self.target_items = fields, masks, tuple(slicing), target_items
        self.segments = fields[0].segments
        self.sizes = [seg.max_doc for seg in self.segments]
        self.n_docs = int(sum(self.sizes))
        self.mask_of = {(si, mid): words[si] for mid, words in masks.items() for si in range(len(self.sizes))}
        self.slices = oracle.corpus_slices(fields[0], self.slicing)
        self._expected: dict = {}
        self._vectors = None

    @property
    def vectors(self) -> List[np.ndarray]:
        if self._vectors is None:
            self._vectors = tk_ref.leaf_vectors(self.fields[0])
        return self._vectors

    def live(self, si: int) -> np.ndarray:
        seg = self.segments[si]
        return np.ones(seg.max_doc, dtype=bool) if seg.live_bits is None else mm_ref._bits(seg.live_bits, seg.max_doc)

    def accept(self, r: Req):
        """liveDocs & FILTER & ~MUST_NOT per leaf as words, or None: the leaves' own liveDocs"""
        if not r.filter and not r.must_not:
            return None
        out = []
        for si, seg in enumerate(self.segments):
            w = synth.accept_words(seg)
            for mid in r.filter:
                w &= self.masks[mid][si]
            for mid in r.must_not:
                w &= ~self.masks[mid][si]
            out.append(w)
        return out

    def _search(self, r: Req):
        common = dict(after=r.after, total_hits_threshold=r.threshold, accept=self.accept(r), slicing=self.slicing)
        scored = dict(functions=r.functions, score_mode=r.score_mode, boost_mode=r.boost_mode, min_score=r.min_score, min_excluded=r.min_excluded,
                      masks=self.mask_of)
        grouped = dict(operator=r.operator, msm=r.msm, tie_breaker=r.tie_breaker)
        info: dict = {}
        if r.entry == "function_score":
            out = fs_ref.search(oracle, self.fields[0], [c[1] for c in r.clauses], r.k, boosts=[c[2] for c in r.clauses], **scored, **common)
        elif r.entry == "multi_match":
            out = mm_ref.search(oracle, self.fields, r.groups, r.shape, r.k, **grouped, **common)
        elif r.entry == "function_score_multi_match":
            out = fsmm_ref.search(oracle, self.fields, r.groups, r.shape, r.k, **grouped, **scored, **common)
        else:
            out = tk_ref.search(oracle, self.fields[0], [c[1] for c in r.clauses], r.k, [(np.asarray(d, np.int64), np.asarray(s, f32), b) for d, s, b in r.lists],
                                nested=r.nested, boosts=[c[2] for c in r.clauses], info=info, **common)
        return out, info.get("kinds")

    def expected(self, r: Req):
        """-> (docs, scores, total_hits, relation_gte), computed once per request; read-only"""
        if r not in self._expected:
            self._expected[r] = self._search(r)
        return self._expected[r][0]

    def kinds(self, r: Req) -> dict:
        """text_knn: the reference's count of listed docs per kind (text / no_text / outside / deleted)"""
        self.expected(r)
        return self._expected[r][1]

    def kept_leaves(self, r: Req) -> List[int]:
        """the leaves that hold a posting of some clause: the parts the planner keeps (text_knn: listed docs keep a leaf too)"""
        out = []
        for si, seg in enumerate(self.segments):
            text = any(len(self.fields[f].segments[si].postings(t)[0]) for f, t, _ in r.clauses)
            listed = any(seg.doc_base <= d < seg.doc_base + seg.max_doc for docs, _, _ in r.lists for d in docs)
            if text or listed:
                out.append(si)
        return out

    def upload(self, ctx):
        """-> (leaves, IndexStatistics)"""
        return mm_ref.upload(api, ctx, self.fields)


# ---- the same request as the binding's objects -------------------------------------------------------------------------------------------
def _flat_inner(r: Req):
    cl = tuple(api.TermQuery(f, t) if b == 1.0 else api.BoostQuery(api.TermQuery(f, t), float(b)) for f, t, b in r.clauses)
    f, mn = tuple(api.MaskFilter(i) for i in r.filter), tuple(api.MaskFilter(i) for i in r.must_not)
    if len(cl) == 1 and not f and not mn:
        return cl[0]
    return api.BooleanQuery(cl, 1 if f else 0, f, mn)      # (with a FILTER clause the SHOULD clauses are optional unless one must match)


def query_of(m: Model, r: Req):
    if r.entry == "function_score":
        return api.FunctionScoreQuery(_flat_inner(r), tuple(api.WeightFunction(float(w), int(i)) for i, w in r.functions), r.score_mode, r.boost_mode,
                                      float(r.min_score), bool(r.min_excluded))
    if r.entry == "multi_match":
        return mm_ref.to_query(api, r.groups, r.shape, r.operator, r.msm, r.tie_breaker, r.filter, r.must_not)
    if r.entry == "function_score_multi_match":
        return fsmm_ref.to_query(api, r.groups, r.shape, r.operator, r.msm, r.tie_breaker, r.functions, r.score_mode, r.boost_mode, r.min_score,
                                 r.min_excluded, r.filter, r.must_not)
    return _flat_inner(r)


def manager_of(r: Req):
    return api.TopScoreDocCollectorManager(r.k, None if r.after is None else api.ScoreDoc(int(r.after[0]), float(r.after[1])), r.threshold)


def knn_clauses_of(r: Req):
    return [api.KnnClause(np.asarray(d, np.int32), np.asarray(s, np.float32), float(b)) for d, s, b in r.lists]


# ---- building blocks of requests ---------------------------------------------------------------------------------------------------------
def flat(tokens, boosts=None) -> Tuple[Tuple[Clause, ...], ...]:
    return (tuple((0, int(t), float(1.0 if boosts is None else boosts[i])) for i, t in enumerate(tokens)),)


def groups_of(shape: str, tokens, field_ids, boosts=None):
    g = (mm_ref.cross_fields_groups if shape == "cross_fields" else mm_ref.best_fields_groups)(tokens, field_ids, boosts)
    return tuple(tuple((int(f), int(t), float(b)) for f, t, b in cl) for cl in g)


def limit_groups(shape: str, tokens8, n_fields: int = 4) -> Tuple[Tuple[Clause, ...], ...]:
    """8 groups x 4 clauses = 32 clauses over 4 distinct fields (fewer where the index has fewer: the fields repeat).  cross_fields:
    one group per token, its term in the four fields; best_fields: group g over field g % 4, four of the tokens each."""
    assert len(tokens8) == 8
    if shape == "cross_fields":
        return tuple(tuple((f % n_fields, int(t), 1.0) for f in range(4)) for t in tokens8)
    return tuple(tuple((g % 4 % n_fields, int(tokens8[(g // 4 * 4 + i) % 8]), 1.0) for i in range(4)) for g in range(8))


def as_list(docs, scores, boost: float) -> KnnList:
    return (tuple(int(d) for d in docs), tuple(float(f32(s)) for s in scores), float(boost))


def _knn(m: Model, query: np.ndarray, k: int, sim: int, boost: float) -> KnnList:
    d, s = tk_ref.knn_list(oracle, m.fields[0], m.vectors, sim, query.astype(f32), k)
    return as_list(d, s, boost)


def _next_page(m: Model, r: Req, at: Optional[int] = None) -> Optional[Req]:
    """the request again with `after` = a hit of its own first page (the last one unless `at` says which)"""
    docs, scores = m.expected(r)[:2]
    if len(docs) == 0:
        return None
    at = len(docs) - 1 if at is None else at
    return dataclasses.replace(r, after=(int(docs[at]), float(scores[at])))


# ---- the layout sweep --------------------------------------------------------------------------------------------------------------------
SINGLE_LEAF = (1, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193, 12287, 12288, 12289)
MULTI_LEAF = ("many_small", "tiny_first", "tiny_last", "eight_slices", "nine_slices", "sixteen_slices", "gaps", "mixed_live")
LAYOUTS = SINGLE_LEAF + MULTI_LEAF
SWEEP_TOKENS = (2, 3, 7)
SWEEP_TOKENS8 = (1, 2, 3, 4, 7, 2, 3, 1)
GAPS_ABSENT, GAPS_ONE_FIELD = (1, 4), (2, 1, 2)            # gaps: the leaves without a query term; (leaf, field, term) absent in one field only
QUERY_TERMS = tuple(sorted(set(SWEEP_TOKENS + SWEEP_TOKENS8)))
N_SWEEP_FIELDS = 4


def layout_of(layout) -> dict:
    """the arguments of build_fields and of the context for one layout"""
    out = dict(deletes=0.05, live_none=(), without=(), slicing=DEFAULT_SLICING, target_items=0)
    if isinstance(layout, int):
        return dict(out, leaf_docs=(layout,), deletes=0.05 if layout >= WORD_DOCS else 0.0)
    if layout == "many_small":
        return dict(out, leaf_docs=tuple((1, 63, 64, 65, 700, 1023, 1024, 1025)[i % 8] for i in range(40)))
    if layout == "tiny_first":
        return dict(out, leaf_docs=(1, 12289), deletes=(0.0, 0.05))
    if layout == "tiny_last":
        return dict(out, leaf_docs=(12289, 1), deletes=(0.05, 0.0))
    if layout in ("eight_slices", "nine_slices", "sixteen_slices"):   # a leaf above sliceMaxDocs is a slice of its own
        return dict(out, leaf_docs=(1025,) * {"eight_slices": 8, "nine_slices": 9, "sixteen_slices": 16}[layout], slicing=(1000, 5))
    if layout == "gaps":
        absent = [(si, fi, t) for si in GAPS_ABSENT for fi in range(N_SWEEP_FIELDS) for t in QUERY_TERMS]
        return dict(out, leaf_docs=(2085,) * 6, without=absent + [GAPS_ONE_FIELD])
    if layout == "mixed_live":
        return dict(out, leaf_docs=(1025, 64, 4097, 1024), deletes=(0.0, 0.3, 0.0, 0.05), live_none=(0, 2))
    raise KeyError(layout)


def edge_list(m: Model, seed: int) -> KnnList:
    """a knn list over the edge docs of every leaf (at most 1024 of them), deleted ones included, worth 50 and more each"""
    docs = np.array([seg.doc_base + d for seg in m.segments for d in EDGE_DOCS(seg.max_doc)], dtype=np.int64)[:1024]
    rng = np.random.Generator(np.random.PCG64(seed))
    return as_list(docs, (50.0 + 10.0 * rng.random(len(docs))).astype(f32), 1.0)


FUNCS = ((EDGE, 8.0), (THIRD, 1.5), (0, 0.5), (SPARSE, 3.0))
EIGHT = ((EDGE, 2.5), (0, 1.25), (THIRD, 0.5), (DENSE, 3.0), (SPARSE, 0.75), (0, 7.0), (LASTWORD, 0.3), (THIRD, 1.5))
RUN_FUNCS = ((THIRD, 2.0), (0, 1.5))                      # with boost_mode "replace": two final scores, long runs of each


@functools.lru_cache(maxsize=2)
def sweep_case(layout):
    """-> (model, {entry: [Req]}, {entry: {"edge": index of the edge-function request, "run": index of the cursor inside a run}})"""
    li = LAYOUTS.index(layout)
    spec = layout_of(layout)
    fields = build_fields(spec["leaf_docs"], N_SWEEP_FIELDS, 3000 + li, spec["deletes"], spec["live_none"], spec["without"])
    m = Model(fields, sweep_masks(spec["leaf_docs"], 4000 + 100 * li), spec["slicing"], spec["target_items"])
    return (m,) + sweep_requests(m, 5000 + li)


def sweep_requests(m: Model, seed: int):
    """the sweep's requests over one model (its masks: sweep_masks) -> ({entry: [Req]}, marks)"""
    nf = len(m.fields)
    first = tuple(range(min(nf, 2)))
    reqs: Dict[str, List[Req]] = {e: [] for e in ENTRIES}
    marks: Dict[str, Dict[str, int]] = {e: {} for e in ENTRIES}
    ks = (1, 10, 1024)

    def add(r: Req, mark: Optional[str] = None) -> Req:
        if mark:
            marks[r.entry][mark] = len(reqs[r.entry])
        reqs[r.entry].append(r)
        return r

    def scored_requests(entry: str, variants):
        """what the two function-score entries share; variants: the inner queries as dicts of Req fields, the first the main one"""
        main = variants[0]
        for k in ks:
            add(Req(entry, k=k, functions=((EDGE, 8.0),), **main), "edge" if k == 10 else None)
        for i, v in enumerate(variants[1:]):
            add(Req(entry, k=ks[i % 3], functions=FUNCS, score_mode=MODE_PAIRS[i % 6][0], boost_mode=MODE_PAIRS[i % 6][1], threshold=(1000, INT_MAX, 0)[i % 3], **v))
        add(Req(entry, functions=((LASTWORD, 3.0),), **main))
        add(Req(entry, functions=FUNCS, filter=(LASTWORD,), **main))
        add(Req(entry, functions=FUNCS, must_not=(THIRD,), k=1024, **main))
        add(Req(entry, functions=FUNCS, filter=(DENSE,), must_not=(SPARSE,), **main))
        add(Req(entry, functions=((0, 2.0),), **main))
        add(Req(entry, **main))
        for sm, bm in MODE_PAIRS:
            add(Req(entry, functions=FUNCS, score_mode=sm, boost_mode=bm, threshold=INT_MAX, **main))
        for sm, bm in (("multiply", "multiply"), ("sum", "sum")):
            add(Req(entry, functions=EIGHT, score_mode=sm, boost_mode=bm, k=1024, **main))
        whole = Req(entry, functions=FUNCS, k=1024, threshold=INT_MAX, **main)
        top = m.expected(whole)[1]
        if len(top) >= 2:   # min_score at a final score the reference itself returned
            for excluded in (True, False):
                add(dataclasses.replace(whole, min_score=float(top[len(top) // 2]), min_excluded=excluded))
        run = Req(entry, functions=RUN_FUNCS, boost_mode="replace", threshold=INT_MAX, **main)
        page2 = _next_page(m, run)
        if page2 is not None:
            add(page2, "run")

    # function_score: a SHOULD disjunction over field 0
    scored_requests("function_score", [dict(groups=flat(SWEEP_TOKENS)), dict(groups=flat(SWEEP_TOKENS, (2.0, 0.5, 1.0))), dict(groups=flat((2,))),
                                       dict(groups=flat((1, 2, 3, 4, 7, 2)))])
    # the two multi-match entries
    shaped = [dict(groups=groups_of(shape, SWEEP_TOKENS, first), shape=shape, operator=op, msm=msm, tie_breaker=tb)
              for shape in ("cross_fields", "best_fields") for op, msm in (("should", 0), ("must", 0), ("should", 2)) for tb in (0.3, 0.0, 1.0)]
    for i, v in enumerate(shaped):
        add(Req("multi_match", k=ks[i % 3], threshold=(1000, INT_MAX, 0)[(i // 3) % 3], **v))
    f1 = nf - 1 if nf < 2 else 1
    two_groups = {"cross_fields": (((0, 2, 1.0), (f1, 2, 1.0)), ((0, 2, 1.0), (f1, 3, 1.0))), "best_fields": (((0, 2, 1.0), (0, 3, 1.0)), ((0, 2, 1.0), (f1, 3, 1.0)))}
    extra = []
    for shape in ("cross_fields", "best_fields"):
        extra.append(dict(groups=limit_groups(shape, SWEEP_TOKENS8, nf), shape=shape, tie_breaker=0.3))                  # 4 fields, 8 x 4 clauses
        extra.append(dict(groups=two_groups[shape], shape=shape, tie_breaker=0.3))                                     # a clause in two groups
        extra.append(dict(groups=groups_of(shape, SWEEP_TOKENS, tuple(range(min(nf, 3))), {0: 2.0, 1: 0.5, 2: 3.25}), shape=shape, tie_breaker=0.3))
    per_group = groups_of("best_fields", SWEEP_TOKENS, first)           # best_fields with a minimum of its own per group: 1, 2, ...
    extra.append(dict(groups=per_group, shape="best_fields", msm=tuple(1 + g % 2 for g in range(len(per_group))), tie_breaker=0.3))
    for v in extra:
        add(Req("multi_match", **v))
    for v in (shaped[0], shaped[9]):
        add(Req("multi_match", filter=(LASTWORD,), **v))
        add(Req("multi_match", must_not=(THIRD,), k=1024, **v))
        add(Req("multi_match", filter=(DENSE,), must_not=(SPARSE,), **v))
    scored_requests("function_score_multi_match", [shaped[0], shaped[9]] + shaped[3:9:2] + shaped[12:18:2] + extra)
    for v in extra[0:4:3]:   # the limits taken together: 4 fields, 32 clauses, 8 functions
        add(Req("function_score_multi_match", functions=EIGHT, score_mode="sum", boost_mode="sum", k=1024, **v))
    # text_knn
    rng = np.random.Generator(np.random.PCG64(seed))
    n_leaves = len(m.sizes)
    small = _knn(m, rng.standard_normal(8), 5, 2, 2.0)
    big = _knn(m, rng.standard_normal(8), min(1024, max(64, n_leaves)), 0, 1.0)
    half = _knn(m, rng.standard_normal(8), 5, 0, 0.5)
    edges = edge_list(m, seed + 1000)
    text = dict(groups=flat(SWEEP_TOKENS))
    for masks in (dict(), dict(filter=(LASTWORD,)), dict(must_not=(THIRD,)), dict(filter=(THIRD,))):   # FLAT, then NESTED
        for i, lists in enumerate(((), (small,), (half, big, edges), (edges,))):
            for k in (ks if i == 2 else (10,)):
                # (the edge list under FILTER THIRD: listed docs outside the accept set)
                add(Req("text_knn", lists=lists, k=k, threshold=(1000, INT_MAX)[i % 2], **masks, **text), "edge" if lists == (edges,) and not masks else None)
    add(Req("text_knn", groups=flat((TERM_NOWHERE,)), lists=(edges, small)))
    add(Req("text_knn", groups=flat((2,), (3.25,)), lists=(big,), k=1024))
    # the second page of every cursor-free request with k = 10
    for entry in ENTRIES:
        for r in list(reqs[entry]):
            if r.after is None and r.k == 10:
                page2 = _next_page(m, r)
                if page2 is not None:
                    add(page2)
    return reqs, marks


# ---- the fuzz ----------------------------------------------------------------------------------------------------------------------------
FUZZ_SIZES = (1, 15, 63, 64, 65, 700, 1023, 1024, 1025, 2085, 5000, 13_400)
FUZZ_MAX_DOCS = 50_000
FUZZ_TOKENS = (1, 2, 3, 4, 5, 6, 7, 9, 11, 12, 13, 1, 2, 3, TERM_NOWHERE)
FUZZ_SLICINGS = (DEFAULT_SLICING, (2000, 2), (500, 1))


def _pick(rng, seq):
    return seq[int(rng.integers(len(seq)))]


def _fuzz_model(rng) -> Model:
    sizes: List[int] = []
    for _ in range(int(rng.integers(1, 13))):
        fit = [n for n in FUZZ_SIZES if sum(sizes) + n <= FUZZ_MAX_DOCS]
        sizes.append(int(_pick(rng, fit)))
    n_fields = int(rng.integers(1, 5))
    share = float(_pick(rng, (0.0, 0.0, 0.03, 0.3)))
    live_none = [si for si in range(len(sizes)) if rng.random() < (0.5 if share == 0.0 else 0.25)]
    deletes = [0.0 if si in live_none else share for si in range(len(sizes))]
    fields = build_fields(sizes, n_fields, int(rng.integers(1 << 30)), deletes, live_none)
    masks = {mid: [synth.random_mask(n, dens, int(rng.integers(1 << 30))) for n in sizes] for mid, dens in FUZZ_MASKS.items()}
    masks[EDGE] = edge_mask(sizes)
    return Model(fields, masks, _pick(rng, FUZZ_SLICINGS), int(_pick(rng, (0, 0, 4096))))


def _fuzz_list(rng, m: Model) -> KnnList:
    """a knn search's own answer, or any docs of the index (deleted ones and docs outside a filter included)"""
    boost = float(_pick(rng, (0.5, 1.0, 2.0)))
    if rng.random() < 0.5:
        return _knn(m, rng.standard_normal(8), int(_pick(rng, (5, 64, 300))), int(_pick(rng, (0, 2))), boost)
    n = min(int(_pick(rng, (1, 5, 64, 1024))), m.n_docs)
    docs = np.sort(rng.choice(m.n_docs, n, replace=False))
    return as_list(docs, (0.05 + 2.95 * rng.random(n)).astype(f32), boost)


def _fuzz_request(rng, m: Model, entry: str) -> Req:
    n_fields = len(m.fields)
    mask_ids = tuple(m.masks)
    big = rng.random() < 0.12                                            # towards the limits: 6-8 tokens, repeats allowed
    n_tok = int(rng.integers(6, 9)) if big else int(rng.integers(1, 5))
    tokens = tuple(int(_pick(rng, FUZZ_TOKENS)) for _ in range(n_tok))
    kw: dict = dict(k=int(_pick(rng, (1, 7, 64, 300, 1024))), threshold=int(_pick(rng, (0, 10, 1000, INT_MAX))))
    if entry.endswith("multi_match"):
        fids = tuple(int(f) for f in (np.arange(n_fields) if big else rng.permutation(n_fields)[: int(rng.integers(1, n_fields + 1))]))
        boosts = {f: float(_pick(rng, BOOSTS)) for f in fids}
        shape = _pick(rng, ("cross_fields", "best_fields"))
        if shape == "best_fields" and big:                                   # at most 8 groups of up to 4 clauses
            groups = tuple(tuple((f, t, boosts[f]) for t in tokens[4 * (g // len(fids)) % n_tok:][:4]) for g, f in enumerate(fids * 2))
        else:
            groups = groups_of(shape, tokens, fids, boosts)
        must = rng.random() < 0.25
        kw.update(groups=groups, shape=shape, operator="must" if must else "should", msm=0 if must else int(rng.integers(0, 3)),
                  tie_breaker=float(_pick(rng, (0.0, 0.3, 1.0, float(np.nextafter(f32(1), f32(0)))))))
    else:
        kw.update(groups=flat(tokens, [float(_pick(rng, BOOSTS)) for _ in tokens]))
    if rng.random() < 0.3:
        kw["filter"] = (int(_pick(rng, mask_ids)),)
    if rng.random() < 0.3:
        kw["must_not"] = (int(_pick(rng, mask_ids)),)
    if entry.startswith("function_score"):
        n_f = 8 if rng.random() < 0.15 else int(rng.integers(0, 8))
        sm, bm = _pick(rng, MODE_PAIRS)
        kw.update(functions=tuple((int(_pick(rng, (0,) + mask_ids)), float(_pick(rng, WEIGHTS))) for _ in range(n_f)), score_mode=sm, boost_mode=bm)
    if entry == "text_knn":
        kw["lists"] = tuple(_fuzz_list(rng, m) for _ in range(int(rng.integers(0, 4))))
    r = Req(entry, **kw)
    if entry.startswith("function_score") and rng.random() < 0.2:        # a min_score from the reference's own scores
        scores = m.expected(r)[1]
        if len(scores):
            r = dataclasses.replace(r, min_score=float(scores[int(rng.integers(len(scores)))]), min_excluded=bool(rng.integers(2)))
    if rng.random() < 0.25:                                              # a cursor from the reference's own first page
        docs = m.expected(r)[0]
        if len(docs):
            r = _next_page(m, r, int(rng.integers(len(docs))))
    return r


@functools.lru_cache(maxsize=2)
def fuzz_round(base: int, round_: int):
    """-> (model, [(entry, [Req])]): two batches of 1-16 requests per entry.  Replay one case: fuzz_round(base, round_)[1][batch][1][index]."""
    rng = np.random.Generator(np.random.PCG64(base + round_))
    m = _fuzz_model(rng)
    batches = []
    for entry in ENTRIES:
        for _ in range(2):
            batches.append((entry, [_fuzz_request(rng, m, entry) for _ in range(int(rng.integers(1, 17)))]))
    return m, batches
