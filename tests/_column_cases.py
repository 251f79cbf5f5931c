"""The cases of tests/test_column_edges_gpu.py (a boundary sweep) and tests/test_fuzz_columns_gpu.py (a seeded differential fuzz) over
the column routes -- nrtgpu_search_sorted_batch, nrtgpu_count_terms_batch, nrtgpu_search_docset_sorted_batch,
nrtgpu_count_docset_terms_batch, the two count entries over single-valued AND multi-valued columns: six entries -- built from a
seed or an explicit layout.  Pure NumPy, no device: the corpus (tests/_field_sort_ref.make_corpus), the masks, the columns per
leaf, the requests, and what each request must return, from the four references (tests/_field_sort_ref.py, _terms_count_ref.py,
_docset_ref.py, _multi_values_ref.py; nothing of them is restated here).  tests/test_column_cases_host.py checks, without a device,
that the cases reach the paths they are meant for.

  column   (arity, kind, name): arity "s" single-valued -- per leaf None or (docs or None = every doc, value bits) -- or "m"
           multi-valued -- per leaf None or (value_docs, value bits); the value pools are tests/test_docset_gpu.py's
  request  Req: the entry, the hit set (a text query's clauses, or a doc set's masks and range clauses), and the sort / the count
  Model    an index as the references see it, Model.expected(req) the reference's answer; query_of / manager_of / sort_of /
           after_of / collector_of: the same request as the binding's objects

The layout numbers are csrc/plan.h's: 64-doc mask words, kTileDocs = 1024-doc sub-tiles, rounds of kScanWaves = 12 sub-tiles
(12 288 docs), kFsCandCap = 3072 candidate slots; planner.cpp: a doc-set query is cut into items of at least kDocsetMinItemTiles =
64 sub-tiles (hostmath::plan_item_counts).

What the generator leaves out, because the routes refuse it: the term in every doc is never a clause beside other terms (its idf
is about 1 / (2 N): 15 binades below a rare term's from some thousand docs on, and a query whose clause weights span more takes
no fixed-point scale); MUST next to SHOULD; a sort or a range over a column that no leaf holds; a sort over a multi-valued column."""
from __future__ import annotations

import dataclasses
import functools
from typing import Dict, List, Optional, Tuple

import numpy as np

from nrtsearch_amd import _lib, api, synth

from tests import _docset_ref as dsr
from tests import _field_sort_ref as fs
from tests import _multi_values_ref as mref
from tests import test_docset_gpu as dg   # the pools of value bits

ALL, NOWHERE = dsr.ALL, 99
KINDS = ("int", "float")
WORD_DOCS, TILE_DOCS, ROUND_TILES, CAND_CAP, DOCSET_MIN_ITEM_TILES = 64, 1024, 12, 3072, 64   # csrc/plan.h, planner.cpp
ROUND_DOCS = ROUND_TILES * TILE_DOCS
DEFAULT_SLICING = (250_000, 5, 1)
ENTRIES = ("sorted", "count", "docset_sorted", "docset_count")
SPECIAL_FLOAT_BOUNDS = np.array([dg.NAN, 0xFFC00001, dg.NZERO, dg.PZERO, dg.NINF, dg.PINF], dtype=np.uint32)
Key = Tuple[str, str, str]


@dataclasses.dataclass(frozen=True)
class Req:
    entry: str                                 # one of ENTRIES
    clauses: Tuple[int, ...] = ()              # text entries: the term ids (repeats count each)
    need: int = 1                              # ... the clauses a hit matches at least
    must: bool = False                         # ... the clauses are MUST (need == len(clauses))
    filters: Tuple[int, ...] = ()              # mask ids
    must_nots: Tuple[int, ...] = ()
    ranges: Tuple[Tuple[Key, int, int], ...] = ()   # doc-set entries: (column, lower bits, upper bits)
    column: Optional[Key] = None               # the sort / count column
    k: int = 10
    reverse: bool = False
    missing: int = 0                           # bits
    threshold: int = 1000
    after: Optional[Tuple[int, int]] = None    # (global doc, value bits)
    max_buckets: int = 1024

    @property
    def docset(self) -> bool:
        return self.entry.startswith("docset")

    @property
    def sorts(self) -> bool:
        return self.entry.endswith("sorted")


class Model:
    """An index as the references see it.  masks: id -> words per leaf; columns: key -> per leaf None or the column's arrays."""

    def __init__(self, corpus, masks: Dict[int, List[np.ndarray]], columns: Dict[Key, list], slicing=DEFAULT_SLICING, target_items: int = 0, flags: int = 0):
        self.corpus, self.masks, self.columns = corpus, masks, columns
        self.slicing, self.target_items, self.flags = slicing, target_items, flags
        self.field = {key: 10 + i for i, key in enumerate(columns)}
        self.sizes = [seg.max_doc for seg in corpus.segments]
        self.n_docs = int(sum(self.sizes))
        self._hits: dict = {}

    def hits(self, r: Req) -> List[np.ndarray]:
        """the request's hit set as words per leaf (computed once per hit set, shared, never written)"""
        memo = (r.docset, r.clauses, r.need, r.filters, r.must_nots, r.ranges)
        if memo not in self._hits:
            f, mn = [self.masks[m] for m in r.filters], [self.masks[m] for m in r.must_nots]
            if r.docset:
                f = f + [mref.any_in_range(self.corpus, key[1], self.columns[key], lo, hi) for key, lo, hi in r.ranges if key[0] == "m"]
                self._hits[memo] = dsr.hit_set(self.corpus, f, mn, [(key[1], self.columns[key], lo, hi) for key, lo, hi in r.ranges if key[0] == "s"])
            else:
                accept = dsr.hit_set(self.corpus, f, mn) if f or mn else None   # (liveDocs & FILTER & ~MUST_NOT)
                self._hits[memo] = mref.text_hits(self.corpus, r.clauses, r.need, accept=accept)
        return self._hits[memo]

    def expected(self, r: Req):
        """sorted: (docs, value bits, total_hits, relation_gte); count: (value bits, counts, n, total_hits, hits_with_value, overflowed)"""
        arity, kind, _ = r.column
        cols = self.columns[r.column]
        if r.sorts:
            return dsr.search(self.corpus, self.hits(r), cols, kind, r.k, r.reverse, r.missing, after=r.after, total_hits_threshold=r.threshold,
                              slicing=self.slicing)
        return (mref.count if arity == "m" else dsr.count)(self.corpus, self.hits(r), cols, kind, r.max_buckets)

    def sorts_as(self, key: Key, doc: int, missing: int) -> int:
        """the bits global doc `doc` sorts as under a single-valued column"""
        for seg, col in zip(self.corpus.segments, self.columns[key]):
            if seg.doc_base <= doc < seg.doc_base + seg.max_doc and col is not None:
                d = doc - seg.doc_base
                if col[0] is None:
                    return int(col[1][d])
                at = int(np.searchsorted(col[0], d))
                return int(col[1][at]) if at < len(col[0]) and int(col[0][at]) == d else missing
        return missing

    def docset_items(self, n_queries: int, n_cus: int = 256) -> int:
        """the items the planner cuts ONE doc-set query of a call of n_queries into (planner.cpp: docset_plan; host_math.h:
        plan_item_counts, the rule for a call whose item count stays inside the target -- true of every call here: <= 16 queries of a
        few items each).  The cost of a query is the sub-tiles of the index."""
        tiles = sum((n + TILE_DOCS - 1) // TILE_DOCS for n in self.sizes)
        target = self.target_items if self.target_items > 0 else n_cus
        per_item = max(DOCSET_MIN_ITEM_TILES, n_queries * tiles // target)
        items = max(1, (tiles + per_item // 2) // per_item)
        assert n_queries * items <= target or n_queries * 2 > target
        return items


# ---- the same request as the binding's objects ---------------------------------------------------------------------------------------
def query_of(m: Model, r: Req):
    f, mn = tuple(api.MaskFilter(i) for i in r.filters), tuple(api.MaskFilter(i) for i in r.must_nots)
    if r.docset:
        return api.DocSetQuery(f, mn, tuple(api.RangeClause(m.field[key], key[1], fs.value_of(key[1], lo), fs.value_of(key[1], hi)) for key, lo, hi in r.ranges))
    terms = tuple(api.TermQuery(0, t) for t in r.clauses)
    if r.must:
        return api.BooleanQuery((), 0, f, mn, terms)
    if len(terms) == 1 and not f and not mn:
        return terms[0]
    return api.BooleanQuery(terms, r.need, f, mn)


def manager_of(r: Req):
    return api.TopScoreDocCollectorManager(r.k, None, r.threshold)


def sort_of(m: Model, r: Req):
    return api.SortField(m.field[r.column], r.column[1], r.reverse, fs.value_of(r.column[1], r.missing))


def after_of(r: Req):
    return None if r.after is None else api.FieldDoc(int(r.after[0]), fs.value_of(r.column[1], r.after[1]))


def collector_of(m: Model, r: Req):
    return api.TermsCollector(m.field[r.column], 10, True, r.column[1])


def describe(r: Req) -> str:
    return ", ".join(f"{f.name}={getattr(r, f.name)!r}" for f in dataclasses.fields(r) if getattr(r, f.name) != f.default)


# ---- columns ---------------------------------------------------------------------------------------------------------------------------
def _no_values():
    return np.zeros(1, np.int32)[:0], np.zeros(1, np.uint32)[:0]   # (slices of real arrays: their data pointers are not NULL)


def _single(rng, n: int, pool: np.ndarray, density: float = 1.0):
    if density >= 1.0:
        return None, rng.choice(pool, size=n).astype(np.uint32)
    d = np.nonzero(rng.random(n) < density)[0].astype(np.int32)
    return d, rng.choice(pool, size=len(d)).astype(np.uint32)


def _multi(rng, per: np.ndarray, pool: np.ndarray):
    """`per` values for each doc; a third of the docs with two or more hold their first value twice"""
    docs = np.repeat(np.arange(len(per), dtype=np.int32), per)
    vals = rng.choice(pool, size=len(docs)).astype(np.uint32)
    first = (np.cumsum(per) - per)[(per >= 2) & (rng.random(len(per)) < 0.34)]
    vals[first + 1] = vals[first]
    return docs, vals


def _pool(kind: str, name: str) -> np.ndarray:
    if name == "both":
        return np.concatenate([dg.POOLS[(kind, "five")], dg.POOLS[(kind, "edge")]])
    return dg.POOLS[(kind, name)]


# ---- the boundary sweep ------------------------------------------------------------------------------------------------------------------
# max_doc on and next to the 64-doc word, the 1024-doc sub-tile and the 12-sub-tile round; then layouts in which an item's
# sub-tiles cross from one leaf into the next on such a boundary.  In HOLES every column is absent from leaf 1 and holds no value
# on leaf 2.
SINGLE_LEAF = (1, WORD_DOCS - 1, WORD_DOCS, WORD_DOCS + 1, TILE_DOCS - 1, TILE_DOCS, TILE_DOCS + 1, ROUND_DOCS - 1, ROUND_DOCS, ROUND_DOCS + 1)
HOLES = (TILE_DOCS + 1, TILE_DOCS, TILE_DOCS - 1, 40)
LAYOUTS = tuple((n,) for n in SINGLE_LEAF) + ((TILE_DOCS, 1, TILE_DOCS - 1), (WORD_DOCS, WORD_DOCS + 1, WORD_DOCS - 1, 1), (ROUND_DOCS, 1), (1, ROUND_DOCS), HOLES)
SWEEP_SINGLE = ("best", "edgevals", "sparse_last", "sparse_nolast")
SWEEP_MULTI = ("last2", "only_last", "steps", "last65", "empty")


def edge_docs(n: int) -> List[int]:
    return sorted({d for d in (0, WORD_DOCS - 1, WORD_DOCS, TILE_DOCS - 1, TILE_DOCS, n - 2, n - 1) if 0 <= d < n})


def _sweep_columns(rng, kind: str, n: int) -> dict:
    """The sweep's columns on one leaf of n docs.  The edge docs decide the answers:
      best           dense; the edge docs hold, in turn, values below and above everyone else's: the head of the page in both
                     directions.  No kind minimum anywhere: a padded slot read as a doc (code 0) would rank first ascending and
                     count as a value no doc holds
      edgevals       dense over the edge pool; the edge docs hold the kind's extremes (INT32_MIN / INT32_MAX; -inf, two NaNs, +inf)
      sparse_last    about half of the docs and the LAST one; sparse_nolast: the same without the last one -- the tail `has` word
      last2          0..2 values per doc, the last doc 2: on a leaf of 1024 n docs start[d + 1] is the entry behind the padding
      only_last      the last doc alone holds values (3): every start[] entry before the last is 0
      steps          one value per doc; docs 63, 64, 1023, 1024 hold 0, 1, 2, 0
      last65         the last doc holds 65 values (more than a wave has lanes), doc 0 one
      empty          a column in which no doc has a value"""
    e = edge_docs(n)
    five, edge, many = dg.POOLS[(kind, "five")], dg.POOLS[(kind, "edge")], dg.POOLS[(kind, "many")]
    out = {}
    if kind == "int":
        best = rng.integers(-1000, 1001, size=n).astype(np.int32)
        for i, d in enumerate(e):
            best[d] = (fs.INT32_MIN + 1 + i) if i % 2 == 0 else (fs.INT32_MAX - 1 - i)
        extremes = dg._i([fs.INT32_MIN, fs.INT32_MAX])
    else:
        best = rng.uniform(-100.0, 100.0, size=n).astype(np.float32)
        for i, d in enumerate(e):
            best[d] = np.float32(1e30 * (1 + i) * (-1.0 if i % 2 == 0 else 1.0))
        extremes = np.array([dg.NINF, dg.NAN, 0xFFC12345, dg.PINF], dtype=np.uint32)
    out[("s", kind, "best")] = (None, best.view(np.uint32))
    vals = rng.choice(edge, size=n).astype(np.uint32)
    vals[e] = extremes[np.arange(len(e)) % len(extremes)]
    out[("s", kind, "edgevals")] = (None, vals)
    half = rng.random(n) < 0.5
    for name, last in (("sparse_last", True), ("sparse_nolast", False)):
        half[n - 1] = last
        d = np.nonzero(half)[0].astype(np.int32)
        out[("s", kind, name)] = (d, rng.choice(five, size=len(d)).astype(np.uint32))
    per = rng.integers(0, 3, size=n)
    per[n - 1] = 2
    out[("m", kind, "last2")] = _multi(rng, per, five)
    per = np.zeros(n, dtype=np.int64)
    per[n - 1] = 3
    out[("m", kind, "only_last")] = _multi(rng, per, edge)
    per = np.ones(n, dtype=np.int64)
    for d, c in ((WORD_DOCS - 1, 0), (WORD_DOCS, 1), (TILE_DOCS - 1, 2), (TILE_DOCS, 0)):
        if d < n:
            per[d] = c
    out[("m", kind, "steps")] = _multi(rng, per, five)
    per = np.zeros(n, dtype=np.int64)
    per[0], per[n - 1] = 1, 65
    docs = np.repeat(np.arange(n, dtype=np.int32), per)
    out[("m", kind, "last65")] = (docs, many[len(many) - len(docs):].astype(np.uint32))
    out[("m", kind, "empty")] = _no_values()
    return out


def dirty(words: np.ndarray, n: int) -> np.ndarray:
    """the words with every bit at and beyond doc n set"""
    w = np.array(words, dtype=np.uint64)
    if n % WORD_DOCS:
        w[-1] |= ~np.uint64((1 << (n % WORD_DOCS)) - 1)
    return w


@functools.lru_cache(maxsize=4)
def sweep_case(layout: Tuple[int, ...], deletes: bool):
    """-> (model, {entry: [Req]}) of one layout.  Terms: 1 in every doc, 2 in half; masks 5 (density 0.6) and 6 (0.2) as in the other
    tests of these routes."""
    li = LAYOUTS.index(layout)
    corpus = fs.make_corpus(layout, {ALL: 1.0, 2: 0.5}, seed=100 + li, delete_fraction=0.1 if deletes else 0.0)
    rng = np.random.default_rng(200 + li)
    columns: Dict[Key, list] = {}
    for si, n in enumerate(layout):
        for kind in KINDS:
            for key, col in _sweep_columns(rng, kind, n).items():
                if layout == HOLES and si in (1, 2):
                    col = None if si == 1 else _no_values()
                columns.setdefault(key, []).append(col)
    masks = {mid: [synth.random_mask(seg.max_doc, dens, 40 * mid + si) for si, seg in enumerate(corpus.segments)] for mid, dens in ((5, 0.6), (6, 0.2))}
    m = Model(corpus, masks, columns)
    n_docs, page = m.n_docs, min(m.n_docs, 1024)
    full = {kind: (fs.KIND_MIN[kind], fs.KIND_MAX[kind]) for kind in KINDS}
    four = ((("s", "int", "best"), int(dg._i([-1000])[0]), fs.KIND_MAX["int"]), (("m", "float", "last2"), int(dg._f([-3.0])[0]), int(dg._f([2.0])[0])),
            (("s", "float", "edgevals"), dg.NINF, dg.NAN), (("m", "int", "steps"),) + full["int"])
    text_sets = [dict(clauses=(ALL,)), dict(clauses=(2,)), dict(clauses=(2,), filters=(5,), must_nots=(6,)), dict(clauses=(2, 2), need=2, must=True)]
    doc_sets = [dict(), dict(filters=(5,)), dict(must_nots=(6,))]
    doc_sets += [dict(ranges=((("s", kind, "best"),) + full[kind],)) for kind in KINDS]      # every doc with a value, never a padded slot
    doc_sets += [dict(ranges=((("m", kind, "steps"),) + full[kind],)) for kind in KINDS]
    doc_sets += [dict(filters=(5,), ranges=four)]
    reqs: Dict[str, List[Req]] = {e: [] for e in ENTRIES}
    for entry, sets in (("sorted", text_sets), ("docset_sorted", doc_sets)):
        for si, hs in enumerate(sets):
            for kind in KINDS:
                for name in SWEEP_SINGLE if si < 3 else ("best", "sparse_nolast"):
                    key, mb = ("s", kind, name), fs.KIND_MAX[kind]
                    for rev in (False, True):
                        base = Req(entry, column=key, reverse=rev, missing=mb, **hs)
                        reqs[entry] += [dataclasses.replace(base, k=k) for k in sorted({1, page})]
                        if si == 0:   # two cursors: the last hit of a first page; the very last doc of the index
                            first = m.expected(dataclasses.replace(base, k=max(page // 2, 1)))
                            if len(first[0]):
                                reqs[entry].append(dataclasses.replace(base, k=max(page // 2, 1), after=(int(first[0][-1]), int(first[1][-1]))))
                            reqs[entry].append(dataclasses.replace(base, k=page, after=(n_docs - 1, m.sorts_as(key, n_docs - 1, mb))))
    for entry, sets in (("count", text_sets), ("docset_count", doc_sets)):
        for hs in sets:
            for kind in KINDS:
                for key in [("s", kind, n) for n in SWEEP_SINGLE] + [("m", kind, n) for n in SWEEP_MULTI]:
                    base = Req(entry, column=key, **hs)
                    distinct = m.expected(dataclasses.replace(base, max_buckets=65536))[2]
                    reqs[entry] += [dataclasses.replace(base, max_buckets=b) for b in (distinct, distinct - 1) if b >= 1]
    return m, reqs


# ---- the fuzz ----------------------------------------------------------------------------------------------------------------------------
# The issue's pool of leaf sizes, and ONE size beyond it, drawn for at most one leaf of a round: no index over the pool alone reaches
# the 96 sub-tiles from which a doc-set query is cut into two items (1.5 x DOCSET_MIN_ITEM_TILES; four leaves of 40 000 have 160, but
# a round almost never draws them).
FUZZ_SIZES = (1, 40, 63, 64, 65, 1000, 1023, 1024, 1025, 3000, 12288, 12289, 13000, 40000)
FUZZ_LARGE = 100_000
FUZZ_TERMS = {ALL: 1.0, 2: 0.6, 3: 0.3, 4: 0.05}
FUZZ_SINGLE = {"wide": ("many", 1.0), "edge": ("both", 1.0), "sparse": ("five", 0.5), "holes": ("edge", 1.0)}   # name -> (pool, density)
FUZZ_MULTI = {"wide": "many", "edge": "both", "holes": "five"}
FLAGS = (_lib.NRTGPU_FLAG_PACKED_POSTINGS, _lib.NRTGPU_FLAG_NO_FIXED_POINT)


def _pick(rng, seq):
    return seq[int(rng.integers(len(seq)))]


def _fuzz_model(rng, round_: int) -> Model:
    n_leaves = int(rng.integers(1, 5))
    sizes: List[int] = []
    for _ in range(n_leaves):
        sizes.append(int(_pick(rng, FUZZ_SIZES + (() if FUZZ_LARGE in sizes else (FUZZ_LARGE,)))))
    corpus = fs.make_corpus(sizes, FUZZ_TERMS, seed=int(rng.integers(1 << 30)), delete_fraction=float(_pick(rng, (0.0, 0.0, 0.03, 0.3))))
    masks = {mid: [synth.random_mask(n, dens, int(rng.integers(1 << 30))) for n in sizes] for mid, dens in ((5, _pick(rng, (0.02, 0.4, 0.97))), (6, _pick(rng, (0.02, 0.4, 0.97))))}
    columns: Dict[Key, list] = {}
    for kind in KINDS:
        for arity, names in (("s", FUZZ_SINGLE), ("m", FUZZ_MULTI)):
            for name in names:
                # "holes": no value on one leaf, absent from a random subset of the others -- never from all
                state = ["present"] * n_leaves
                if name == "holes" and n_leaves >= 2:
                    order = rng.permutation(n_leaves)
                    state[order[0]] = "empty"
                    for si in order[2:]:
                        state[si] = "absent" if rng.random() < 0.5 else "present"
                cols = []
                for si, n in enumerate(sizes):
                    if state[si] != "present":
                        cols.append(None if state[si] == "absent" else _no_values())
                    elif arity == "s":
                        cols.append(_single(rng, n, _pool(kind, names[name][0]), names[name][1]))
                    else:
                        cols.append(_multi(rng, rng.integers(0, 4, size=n), _pool(kind, names[name])))
                columns[(arity, kind, name)] = cols
    flags = FLAGS[(round_ // 4) % 2] if round_ % 4 == 3 else 0
    return Model(corpus, masks, columns, slicing=_pick(rng, (DEFAULT_SLICING, (1000, 5, 1))), target_items=int(_pick(rng, (0, 64))), flags=flags)


def _text_hit_set(rng) -> dict:
    """term, OR of 2-6 clauses with repeats, min_should_match, all-MUST, masks.  The term in every doc stands alone (module docstring)."""
    shape = _pick(rng, ("term", "or", "msm", "must", "masks", "everywhere"))
    others = (2, 3, 4, 2, 3, 4, NOWHERE)
    if shape == "everywhere":
        n = int(rng.integers(1, 4))
        return dict(clauses=(ALL,) * n, need=int(rng.integers(1, n + 1))) if rng.random() < 0.5 else dict(clauses=(ALL,) * n, need=n, must=True)
    if shape == "term":
        return dict(clauses=(int(_pick(rng, others)),))
    n = int(rng.integers(2, 7))
    clauses = tuple(int(_pick(rng, others)) for _ in range(n))
    if shape == "msm":
        return dict(clauses=clauses, need=int(rng.integers(2, n + 1)))
    if shape == "must":
        clauses = clauses[: int(rng.integers(1, 5))]
        return dict(clauses=clauses, need=len(clauses), must=True)
    if shape == "masks":
        f, mn = _pick(rng, (((5,), ()), ((), (6,)), ((5,), (6,)), ((6,), (5,))))
        return dict(clauses=clauses, filters=f, must_nots=mn)
    return dict(clauses=clauses)


def _bound(rng, key: Key) -> int:
    if key[1] == "float" and rng.random() < 0.25:
        return int(_pick(rng, SPECIAL_FLOAT_BOUNDS))
    names = FUZZ_SINGLE[key[2]][0] if key[0] == "s" else FUZZ_MULTI[key[2]]
    return int(_pick(rng, _pool(key[1], names)))


def _doc_set(rng, m: Model) -> dict:
    """0-2 filters, 0-2 must-nots, 0-4 range clauses over columns of either arity; bounds from the pools in any order (lower > upper,
    NaN and signed-zero bounds included)"""
    keys = list(m.columns)
    f = tuple(int(i) for i in rng.permutation([5, 6])[: int(rng.integers(0, 3))])
    mn = tuple(int(i) for i in rng.permutation([5, 6])[: int(rng.integers(0, 3))])
    if rng.random() < 0.8:   # (a mask on both sides leaves nothing: keep that rare)
        mn = tuple(i for i in mn if i not in f)
    ranges = []
    for _ in range(int(rng.integers(0, 5))):
        key = _pick(rng, keys)
        lo, hi = _bound(rng, key), _bound(rng, key)
        if rng.random() < 0.85 and int(fs.order_key(key[1], [lo])[0]) > int(fs.order_key(key[1], [hi])[0]):
            lo, hi = hi, lo   # (lower > upper keeps nothing: one range in thirteen stays that way)
        if rng.random() < 0.3:   # a half-open range
            lo, hi = (fs.KIND_MIN[key[1]], hi) if rng.random() < 0.5 else (lo, fs.KIND_MAX[key[1]])
        ranges.append((key, lo, hi))
    return dict(filters=f, must_nots=mn, ranges=tuple(ranges))


def _fuzz_request(rng, m: Model, entry: str) -> Req:
    hs = _doc_set(rng, m) if entry.startswith("docset") else _text_hit_set(rng)
    kind = _pick(rng, KINDS)
    if entry.endswith("sorted"):
        key = ("s", kind, _pick(rng, tuple(FUZZ_SINGLE)))
        pool = _pool(kind, FUZZ_SINGLE[key[2]][0])
        r = Req(entry, column=key, k=int(_pick(rng, (1, 7, 64, 300, 1000, 1024))), reverse=bool(rng.integers(2)),
                missing=int(_pick(rng, (fs.KIND_MIN[kind], fs.KIND_MAX[kind], int(_pick(rng, pool))))), threshold=int(_pick(rng, (1000, 10, 0, 2**31 - 1))), **hs)
        if rng.random() < 0.3:   # a cursor: three in four a hit of the first page, else any (doc, pool value)
            first = m.expected(r)
            if rng.random() < 0.75 and len(first[0]):
                at = int(rng.integers(len(first[0])))
                r = dataclasses.replace(r, after=(int(first[0][at]), int(first[1][at])))
            else:
                r = dataclasses.replace(r, after=(int(rng.integers(m.n_docs)), int(_pick(rng, pool))))
        return r
    arity = _pick(rng, ("s", "m"))
    key = (arity, kind, _pick(rng, tuple(FUZZ_SINGLE if arity == "s" else FUZZ_MULTI)))
    r = Req(entry, column=key, **hs)
    distinct = m.expected(dataclasses.replace(r, max_buckets=65536))[2]
    return dataclasses.replace(r, max_buckets=int(_pick(rng, [b for b in (distinct, distinct - 1, distinct + 1, 1, 65536) if b >= 1])))


@functools.lru_cache(maxsize=2)
def fuzz_round(base: int, round_: int):
    """-> (model, [(entry, [Req])]): four batches of 1-16 requests per entry.  A flagged round (round_ % 4 == 3) issues doc-set
    requests only.  Replay one case: fuzz_round(base, round_)[1][batch][1][index]."""
    rng = np.random.Generator(np.random.PCG64(base + round_))
    m = _fuzz_model(rng, round_)
    batches = []
    for entry in ENTRIES:
        if m.flags and not entry.startswith("docset"):
            continue
        for _ in range(4):
            batches.append((entry, [_fuzz_request(rng, m, entry) for _ in range(int(rng.integers(1, 17)))]))
    return m, batches
