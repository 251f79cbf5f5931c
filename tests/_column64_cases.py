"""The cases of tests/test_column64_edges_gpu.py (a boundary sweep) and tests/test_fuzz_columns64_gpu.py (a seeded differential fuzz)
over the routes that read 64-BIT doc value columns -- nrtgpu_search_sorted64_batch, nrtgpu_search_docset_sorted64_batch,
nrtgpu_segment_set_mask_from_values64, nrtgpu_count_ranges_batch and nrtgpu_count_docset_ranges_batch over LONG / DOUBLE columns:
five entries -- built from a seed or an explicit layout.  Pure NumPy, no device.  The design is tests/_column_cases.py's, whose Model,
layouts, edge docs and fuzz pieces are used here, not copied; what each request must return comes from the references alone
(tests/_field_sort64_ref.py: search, text_hits, docset_hits; _value_masks64_ref.mask; _range_count_ref.count;
_multi_values_ref.any_in_range for a doc set's multi-valued 32-bit range clauses; _docset_ref for a text query's accept words):
nothing of the library's coding of the values or of its packed keys is restated here.  tests/test_column64_cases_host.py checks,
without a device, that the cases reach the paths they are meant for.

  column   (arity, kind, name): the 64-bit ones ("s", "long" | "double", name) -- per leaf None (the leaf lacks the column) or (docs or
           None = every doc, value bits uint64) -- and three 32-bit ones for the doc sets' own range clauses, as in _column_cases
  request  Req: _column_cases.Req and, for the count entries, the ranges to count; for mask64 the leaf and the clauses
  Model    _column_cases.Model with the 64-bit references behind hits() / expected(), and fits(): whether a sort's window fits the key

Whether a sort FITS is computed here from include/nrtgpu.h's statement of the rule alone -- span + 3 <= 2^(64 - db) - 1, db the bits
of the greatest global docid, span the distance of the least and the greatest value of the column IN THE KIND'S ORDER
(_field_sort64_ref.order_int: a step of one ulp, and the step from -0.0 to +0.0, is 1) -- over plain Python ints; it never calls
nrtgpu_sort_key64."""
from __future__ import annotations

import dataclasses
import functools
import types
from typing import Dict, List, Optional, Tuple

import numpy as np

from nrtsearch_amd import api, synth

from tests import _column_cases as cc
from tests import _docset_ref as dsr
from tests import _field_sort64_ref as f64
from tests import _field_sort_ref as fs
from tests import _multi_values_ref as mref
from tests import _range_count_ref as rcr
from tests import _value_masks64_ref as vm

ALL = cc.ALL
KINDS = ("long", "double")
ENTRIES = ("sorted64", "docset_sorted64", "mask64", "ranges64", "docset_ranges64")
BATCH_ENTRIES = ("sorted64", "docset_sorted64", "ranges64", "docset_ranges64")   # the entries that take a batch of queries
Key = cc.Key
EPOCH = 1_700_000_000_000
NAN, NAN_PAYLOAD = f64.CANONICAL_NAN, 0x7FF8000000000123
NINF, PINF, NZERO, PZERO, DBL_MAX = 0xFFF0000000000000, 0x7FF0000000000000, 0x8000000000000000, 0, 0x7FEFFFFFFFFFFFFF
KIND_MIN = {"long": f64.bits_of("long", f64.INT64_MIN), "double": NINF}    # the least and the greatest value in the kind's order
KIND_MAX = {"long": f64.bits_of("long", f64.INT64_MAX), "double": NAN}
# a cursor value below every column's window here that is not the kind's minimum (the clamp trap of tests/test_field_sort64_gpu.py)
TRAP = {"long": f64.bits_of("long", f64.INT64_MIN + 5), "double": f64.bits_of("double", -1e300)}


def _u64(values) -> np.ndarray:
    return np.array([int(v) & (f64.U64 - 1) for v in values], dtype=np.uint64)


ULPS = (0, 1, 2, 3, 77, 2**10, 2**20, 2**29, 2**29 + 1, 2**30 - 2, 2**30 - 1, 5)   # tests/test_field_sort64_gpu.py's DOUBLE_POOL
# The pools the columns draw from.  long/halves: eight values that agree in their low 32 bits (j 2^32 + 5) and eight that agree in
# their high word: a compare of either half alone ties.  double/pos: 1.5 + j ulp; neg: -1.5 - j ulp, the same j; zeros: the two
# zeros (a span of 1); naninf: the greatest finite double, +inf, NaNs under three payloads and both sign bits (a span of 2^51 + 1).
POOLS = {
    ("long", "halves"): _u64([(j << 32) + 5 for j in range(1, 9)] + [(4 << 32) + 1000 * j + 7 for j in range(8)]),
    ("double", "pos"): _u64([f64.bits_of("double", 1.5) + j for j in ULPS]),
    ("double", "neg"): _u64([f64.bits_of("double", -1.5) + j for j in ULPS]),
    ("double", "zeros"): _u64([NZERO, PZERO]),
    ("double", "naninf"): _u64([DBL_MAX, PINF, NAN, 0x7FF0000000000001, 0xFFF8000000000123]),
}
# per column a value INSIDE its window that no doc holds (None: the window has no such value -- zeros: a span of 1; naninf: nothing
# lies between the greatest finite double, +inf and NaN; empty: no window)
GAP = {
    ("long", "best"): f64.bits_of("long", EPOCH + 5000), ("long", "halves"): (2 << 32) + 6, ("long", "sparse_last"): (2 << 32) + 6,
    ("long", "sparse_nolast"): (2 << 32) + 6, ("long", "empty"): None,
    ("double", "pos"): f64.bits_of("double", 1.5) + 4, ("double", "neg"): f64.bits_of("double", -1.5) + 4, ("double", "zeros"): None,
    ("double", "naninf"): None, ("double", "sparse_last"): f64.bits_of("double", -1.5) + 4,
}
SORT_COLUMNS = tuple(("s",) + kn for kn in GAP)            # every 64-bit column, in the order above
FUZZ_COLUMNS = tuple(key for key in SORT_COLUMNS if key[2] != "naninf")
# the bounds the fuzz draws ranges, cursors and clauses from: the pools, the kinds' extremes, the special doubles
BOUNDS = {
    "long": np.concatenate([POOLS[("long", "halves")], _u64([EPOCH - 1000, EPOCH, EPOCH + 1000, EPOCH - 2**34, EPOCH + 2**34, f64.INT64_MIN, f64.INT64_MAX, 0, -1])]),
    "double": np.concatenate([POOLS[("double", "pos")], POOLS[("double", "neg")], POOLS[("double", "zeros")], POOLS[("double", "naninf")], _u64([NINF, NAN_PAYLOAD])]),
}
# the three 32-bit columns of every index, for the doc sets' own range clauses (names and pools are _column_cases' fuzz columns')
RANGE_COLUMNS = (("s", "int", "edge"), ("m", "int", "wide"), ("m", "float", "edge"))
R_SINGLE, R_MULTI_INT, R_MULTI_FLOAT = RANGE_COLUMNS


@dataclasses.dataclass(frozen=True)
class Req(cc.Req):
    count_ranges: Tuple[Tuple[int, int], ...] = ()   # ranges64 / docset_ranges64: (lower bits, upper bits), both inclusive
    leaf: int = 0                                    # mask64: the leaf ...
    value_clauses: Tuple[tuple, ...] = ()            # ... and (column, "exists") / (column, "range", lower bits, upper bits)

    @property
    def sorts(self) -> bool:
        return self.entry.endswith("sorted64")

    @property
    def counts(self) -> bool:
        return self.entry.endswith("ranges64")


class Model(cc.Model):
    """_column_cases.Model (masks, columns, field ids, docset_items) with the 64-bit references behind it.  hits(): bool per doc."""

    def hits(self, r: Req) -> List[np.ndarray]:
        memo = (r.docset, r.clauses, r.need, r.filters, r.must_nots, r.ranges)
        if memo not in self._hits:
            f, mn = [self.masks[m] for m in r.filters], [self.masks[m] for m in r.must_nots]
            if r.docset:
                f = f + [mref.any_in_range(self.corpus, key[1], self.columns[key], lo, hi) for key, lo, hi in r.ranges if key[0] == "m"]
                self._hits[memo] = f64.docset_hits(self.corpus, f, mn, [(self.columns[key], key[1], lo, hi) for key, lo, hi in r.ranges if key[0] == "s"])
            else:
                accept = dsr.hit_set(self.corpus, f, mn) if f or mn else None   # (liveDocs & FILTER & ~MUST_NOT)
                self._hits[memo] = f64.text_hits(self.corpus, r.clauses, r.need, accept=accept)
        return self._hits[memo]

    def expected(self, r: Req):
        """sorted: (docs, value bits, total_hits, relation_gte); ranges: (counts, total_hits, hits_with_value); mask64: (words, count)"""
        if r.entry == "mask64":
            n = self.sizes[r.leaf]
            words = vm.mask(n, [(self.columns[c[0]][r.leaf], c[0][1], tuple(c[1:])) for c in r.value_clauses])
            return words, int(fs._bits(words, n).sum())
        kind, cols = r.column[1], self.columns[r.column]
        if r.sorts:
            return f64.search(self.corpus, self.hits(r), cols, kind, r.k, r.reverse, r.missing, after=r.after, total_hits_threshold=r.threshold, slicing=self.slicing)
        return rcr.count(self.corpus, self.hits(r), cols, kind, list(r.count_ranges))

    def window(self, key: Key) -> Optional[Tuple[int, int]]:
        """the least and the greatest value of the column over the leaves, as order_int; None: no leaf holds a value"""
        keys = [f64.order_key(key[1], col[1]) for col in self.columns[key] if col is not None and len(col[1])]
        return (int(min(k.min() for k in keys)), int(max(k.max() for k in keys))) if keys else None

    def doc_bits(self) -> int:
        return max(1, (self.n_docs - 1).bit_length())

    def fits(self, key: Key) -> bool:
        """include/nrtgpu.h: THE SORT FITS iff span + 3 <= 2^(64 - db) - 1 (module docstring)"""
        w = self.window(key)
        span = 0 if w is None else w[1] - w[0]
        return span + 3 <= 2 ** (64 - self.doc_bits()) - 1

    def value_docs(self, key: Key) -> int:
        """the docs that have a value in the column"""
        return sum(0 if col is None else (n if col[0] is None else len(col[0])) for n, col in zip(self.sizes, self.columns[key]))


# ---- the same request as the binding's objects (query_of and manager_of are _column_cases') -------------------------------------------
query_of, manager_of, describe = cc.query_of, cc.manager_of, cc.describe


def sort_of(m: Model, r: Req):
    return api.SortField64(m.field[r.column], r.column[1], r.reverse, f64.value_of(r.column[1], r.missing))


def after_of(r: Req):
    return None if r.after is None else api.FieldDoc(int(r.after[0]), f64.value_of(r.column[1], r.after[1]))


def counter_of(m: Model, r: Req):
    return api.RangeCounter(m.field[r.column], r.column[1], tuple(r.count_ranges))


def clauses_of(m: Model, r: Req):
    return [api.ValueClause64.exists(m.field[c[0]]) if c[1] == "exists" else api.ValueClause64("range", m.field[c[0]], c[0][1], int(c[2]), int(c[3]))
            for c in r.value_clauses]


# ---- columns ---------------------------------------------------------------------------------------------------------------------------
def _no_values64():
    return np.zeros(1, np.int32)[:0], np.zeros(1, np.uint64)[:0]   # (n = 0 with docs given; slices of real arrays: no NULL pointer)


def _columns64(rng, n: int, naninf: bool = True) -> dict:
    """The 64-bit columns on one leaf of n docs.  The edge docs (_column_cases.edge_docs) decide the answers:
      long/best            dense around an epoch-millis base; the edge docs hold, in turn, values below and above everyone else's by
                           more than 2^33: the head of the page in both directions, every compare crossing the low word.  No
                           INT64_MIN anywhere: a padded slot read as a doc would rank first ascending
      long/halves          dense over the halves pool: ties decide most ranks
      long/sparse_last     about half of the docs and the LAST one; sparse_nolast: the same without the last one -- the tail `has` word
      long/empty           a column in which no doc has a value
      double/pos, neg      dense, 1.5 + j ulp and -1.5 - j ulp; zeros: -0.0 and +0.0 only
      double/naninf        the greatest finite double, +inf and NaNs; the edge docs hold the pool's members in turn
      double/sparse_last   about half of the docs and the last one, over neg's pool"""
    e = cc.edge_docs(n)
    out = {}
    best = EPOCH + rng.integers(-1000, 1001, size=n).astype(np.int64)
    for i, d in enumerate(e):
        best[d] = EPOCH - 2**34 - i if i % 2 == 0 else EPOCH + 2**34 + i
    out[("s", "long", "best")] = (None, best.view(np.uint64))
    halves = POOLS[("long", "halves")]
    out[("s", "long", "halves")] = (None, rng.choice(halves, size=n))
    half = rng.random(n) < 0.5
    for name, last in (("sparse_last", True), ("sparse_nolast", False)):
        half[n - 1] = last
        d = np.nonzero(half)[0].astype(np.int32)
        out[("s", "long", name)] = (d, rng.choice(halves, size=len(d))) if len(d) else _no_values64()
    out[("s", "long", "empty")] = _no_values64()
    for name in ("pos", "neg", "zeros", "naninf"):
        vals = rng.choice(POOLS[("double", name)], size=n)
        if name == "naninf":
            vals[e] = POOLS[("double", name)][np.arange(len(e)) % 5]
        out[("s", "double", name)] = (None, vals)
    half = rng.random(n) < 0.5
    half[n - 1] = True
    d = np.nonzero(half)[0].astype(np.int32)
    out[("s", "double", "sparse_last")] = (d, rng.choice(POOLS[("double", "neg")], size=len(d)))
    if not naninf:
        del out[("s", "double", "naninf")]
    return out


def _held(m: Model, key: Key) -> List[int]:
    """the values of the column that sit on edge docs, leaf after leaf (empty: the column holds no value)"""
    out = []
    for n, col in zip(m.sizes, m.columns[key]):
        if col is None or not len(col[1]):
            continue
        if col[0] is None:
            out += [int(col[1][d]) for d in cc.edge_docs(n)]
        else:
            out += [int(col[1][0]), int(col[1][len(col[1]) // 2]), int(col[1][-1])]
    return out


def _ordered(kind: str, a: int, b: int) -> Tuple[int, int]:
    return (a, b) if f64.order_int(kind, a) <= f64.order_int(kind, b) else (b, a)


def missing_values(m: Model, key: Key) -> List[int]:
    """the kind's minimum, its maximum, a value some doc holds, a value inside the window that no doc holds, (doubles) a NaN with a payload"""
    kind = key[1]
    held = _held(m, key)
    out = [KIND_MIN[kind], KIND_MAX[kind]] + held[:1] + ([GAP[key[1:]]] if GAP[key[1:]] is not None else [])
    return out + ([NAN_PAYLOAD] if kind == "double" else [])


def range_lists(m: Model, key: Key) -> List[Tuple[Tuple[int, int], ...]]:
    """-> [the named ranges, the same filled up to 64]: single-value ranges at the edge docs' values, the full range, two overlapping
    ranges, an empty range; the filler pairs values of the kind's bounds, in order"""
    kind = key[1]
    held = list(dict.fromkeys(_held(m, key)))[:6] or [int(BOUNDS[kind][0])]
    by_order = sorted(set(held) | {int(b) for b in BOUNDS[kind][:8]}, key=lambda b: f64.order_int(kind, b))
    q = len(by_order)
    named = [(v, v) for v in held] + [(KIND_MIN[kind], KIND_MAX[kind]), (by_order[0], by_order[q // 2]), (by_order[q // 4], by_order[-1]), (by_order[-1], by_order[0])]
    if f64.order_int(kind, by_order[-1]) == f64.order_int(kind, by_order[0]):
        named[-1] = (KIND_MAX[kind], KIND_MIN[kind])
    filler = [_ordered(kind, int(BOUNDS[kind][i % len(BOUNDS[kind])]), int(BOUNDS[kind][(i * 7 + 3) % len(BOUNDS[kind])])) for i in range(64 - len(named))]
    return [tuple(named), tuple(named + filler)]


def _mask_requests(m: Model, leaf: int) -> List[Req]:
    """exists; [kind min, kind max]; a range between values of edge docs; lower > upper; two clauses over two columns; for doubles
    [NaN, NaN], [-inf, +inf] and [-0.0, +0.0] -- over every 64-bit column the leaf holds"""
    keys = [key for key in SORT_COLUMNS if key in m.columns and m.columns[key][leaf] is not None]
    out = []
    for i, key in enumerate(keys):
        kind, col = key[1], m.columns[key][leaf]
        e = [int(col[1][d]) for d in cc.edge_docs(m.sizes[leaf])] if col[0] is None else [int(v) for v in col[1][[0, -1]]] if len(col[1]) else [int(BOUNDS[kind][0])] * 2
        lo, hi = _ordered(kind, e[0], e[-1])
        other = keys[(i + 1) % len(keys)]
        sets = [((key, "exists"),), ((key, "range", KIND_MIN[kind], KIND_MAX[kind]),), ((key, "range", lo, hi),), ((key, "range", KIND_MAX[kind], KIND_MIN[kind]),),
                ((key, "range", lo, KIND_MAX[kind]), (other, "exists")), ((key, "range", KIND_MIN[kind], hi), (other, "range", KIND_MIN[other[1]], KIND_MAX[other[1]]))]
        if f64.order_int(kind, lo) < f64.order_int(kind, hi):
            sets.append(((key, "range", hi, lo),))
        if kind == "double":
            sets += [((key, "range", NAN, 0xFFF8000000000123),), ((key, "range", NINF, PINF),), ((key, "range", NZERO, PZERO),)]
        out += [Req("mask64", leaf=leaf, value_clauses=vc) for vc in sets]
    return out


def _range32_columns(rng, n: int) -> dict:
    """the three 32-bit columns on one leaf: a single-valued int, a multi-valued int with 0-3 values per doc, a multi-valued float"""
    return {R_SINGLE: cc._single(rng, n, cc._pool("int", "both")), R_MULTI_INT: cc._multi(rng, rng.integers(0, 4, size=n), cc._pool("int", "many")),
            R_MULTI_FLOAT: cc._multi(rng, rng.integers(0, 4, size=n), cc._pool("float", "both"))}


def doc_set_shapes() -> List[dict]:
    """no range clause; a single-valued one; a multi-valued one (int, float); both beside masks: docset_sort_kernel<DocsetSort64, false> and <true>
    and both MULTI forms of the wide range-count kernel run"""
    i32, f32 = (lambda v: fs.bits_of("int", v)), (lambda v: fs.bits_of("float", v))
    return [dict(), dict(filters=(5,)), dict(must_nots=(6,)),
            dict(ranges=((R_SINGLE, fs.KIND_MIN["int"], fs.KIND_MAX["int"]),)),                     # every doc with a value, never a padded slot
            dict(ranges=((R_SINGLE, i32(-1), i32(1)),)),
            dict(ranges=((R_MULTI_INT, i32(-2000), i32(9000)),)),
            dict(ranges=((R_MULTI_FLOAT, f32(-1.5), f32(3.25)),)),
            dict(filters=(5,), must_nots=(6,), ranges=((R_MULTI_INT, i32(-9000), i32(4000)), (R_SINGLE, i32(-1), fs.KIND_MAX["int"])))]


@functools.lru_cache(maxsize=4)
def sweep_case(layout: Tuple[int, ...], deletes: bool):
    """-> (model, {entry: [Req]}) of one layout of _column_cases.LAYOUTS.  Terms: 1 in every doc, 2 in half; masks 5 (density 0.6) and
    6 (0.2).  In HOLES every column is absent from leaf 1 and holds no value on leaf 2."""
    li = cc.LAYOUTS.index(layout)
    corpus = fs.make_corpus(layout, {ALL: 1.0, 2: 0.5}, seed=300 + li, delete_fraction=0.1 if deletes else 0.0)
    rng = np.random.default_rng(400 + li)
    columns: Dict[Key, list] = {}
    for si, n in enumerate(layout):
        for key, col in {**_columns64(rng, n), **_range32_columns(rng, n)}.items():
            if layout == cc.HOLES and si in (1, 2):
                col = None if si == 1 else (cc._no_values() if key in RANGE_COLUMNS else _no_values64())
            columns.setdefault(key, []).append(col)
    masks = {mid: [synth.random_mask(seg.max_doc, dens, 50 * mid + si) for si, seg in enumerate(corpus.segments)] for mid, dens in ((5, 0.6), (6, 0.2))}
    m = Model(corpus, masks, columns)
    n_docs, page = m.n_docs, min(m.n_docs, 1024)
    text_sets = [dict(clauses=(ALL,)), dict(clauses=(2,)), dict(clauses=(2,), filters=(5,), must_nots=(6,)), dict(clauses=(2, 2), need=2, must=True)]
    doc_sets = doc_set_shapes()
    reqs: Dict[str, List[Req]] = {e: [] for e in ENTRIES}
    for entry, sets in (("sorted64", text_sets), ("docset_sorted64", doc_sets)):
        turn = 0
        for key in SORT_COLUMNS:
            kind = key[1]
            for rev in (False, True):
                for mb in missing_values(m, key):          # the hit sets take turns: every one meets every kind of missing value
                    base = Req(entry, column=key, reverse=rev, missing=mb, **sets[turn % len(sets)])
                    turn += 1
                    reqs[entry] += [dataclasses.replace(base, k=k) for k in sorted({1, page})]
                # four cursors over the whole index: the last hit of a half page; the very last doc of the index; a value outside
                # the window that is not the missing value (the clamp trap); the missing value itself
                base = Req(entry, column=key, reverse=rev, missing=KIND_MAX[kind], **sets[0])
                reqs[entry].append(dataclasses.replace(base, k=page))   # (the unfiltered page itself)
                first = m.expected(dataclasses.replace(base, k=max(page // 2, 1)))
                if len(first[0]):
                    reqs[entry].append(dataclasses.replace(base, k=max(page // 2, 1), after=(int(first[0][-1]), int(first[1][-1]))))
                reqs[entry].append(dataclasses.replace(base, k=page, after=(n_docs - 1, m.sorts_as(key, n_docs - 1, KIND_MAX[kind]))))
                base = dataclasses.replace(base, missing=KIND_MIN[kind], k=max(page // 2, 1))
                reqs[entry] += [dataclasses.replace(base, after=(0, TRAP[kind])), dataclasses.replace(base, after=(n_docs // 2, KIND_MIN[kind]))]
    for leaf in range(len(layout)):
        reqs["mask64"] += _mask_requests(m, leaf)
    for ci, key in enumerate(SORT_COLUMNS):
        lists = range_lists(m, key)
        reqs["ranges64"] += [Req("ranges64", column=key, count_ranges=lists[(ci + ti) % 2], **text_sets[(ci + ti) % len(text_sets)]) for ti in range(2)]
        reqs["docset_ranges64"] += [Req("docset_ranges64", column=key, count_ranges=lists[(ci + di) % 2], **hs) for di, hs in enumerate(doc_sets)]
        reqs["docset_ranges64"].append(Req("docset_ranges64", column=key, count_ranges=((KIND_MIN[key[1]], KIND_MAX[key[1]]),)))   # the full range under match-all
    return m, reqs


# ---- the fuzz ----------------------------------------------------------------------------------------------------------------------------
def _fuzz_model(rng, round_: int) -> Model:
    """_column_cases' fuzz index -- 1-4 leaves of FUZZ_SIZES, at most one of FUZZ_LARGE docs, deletes, two masks, the context's
    slicing, target_items, a flag every fourth round -- keeping its three range columns, with the 64-bit columns (all but naninf)
    drawn behind it; a sparse column is absent from one leaf of half of the indexes that have two or more"""
    m32 = cc._fuzz_model(rng, round_)
    columns: Dict[Key, list] = {key: m32.columns[key] for key in RANGE_COLUMNS}
    per_leaf = [_columns64(rng, n, naninf=False) for n in m32.sizes]
    for key in FUZZ_COLUMNS:
        cols = [leaf[key] for leaf in per_leaf]
        if key[2].startswith("sparse") and len(cols) >= 2 and rng.random() < 0.5:
            cols[int(rng.integers(len(cols)))] = None
        columns[key] = cols
    return Model(m32.corpus, m32.masks, columns, slicing=m32.slicing, target_items=m32.target_items, flags=m32.flags)


def _bounds64(rng, kind: str) -> Tuple[int, int]:
    """two of the kind's bounds, in any order: one pair in seven stays lower > upper"""
    lo, hi = int(cc._pick(rng, BOUNDS[kind])), int(cc._pick(rng, BOUNDS[kind]))
    return _ordered(kind, lo, hi) if rng.random() < 0.85 else (lo, hi)


def _fuzz_request(rng, m: Model, entry: str) -> Req:
    hs = cc._doc_set(rng, types.SimpleNamespace(columns={key: m.columns[key] for key in RANGE_COLUMNS})) if entry.startswith("docset") else cc._text_hit_set(rng)
    key = cc._pick(rng, FUZZ_COLUMNS)
    kind = key[1]
    if entry.endswith("ranges64"):
        return Req(entry, column=key, count_ranges=tuple(_bounds64(rng, kind) for _ in range(int(cc._pick(rng, (1, 2, 3, 5, 17, 64, int(rng.integers(1, 65))))))), **hs)
    r = Req(entry, column=key, k=int(cc._pick(rng, (1, 7, 64, 300, 1000, 1024))), reverse=bool(rng.integers(2)), missing=int(cc._pick(rng, missing_values(m, key))),
            threshold=int(cc._pick(rng, (1000, 10, 0, 2**31 - 1))), **hs)
    if rng.random() < 0.3:   # a cursor: three in four a hit of the first page, else any doc with a bound, a kind extreme, a value outside the window
        first = m.expected(r)
        if rng.random() < 0.75 and len(first[0]):
            at = int(rng.integers(len(first[0])))
            r = dataclasses.replace(r, after=(int(first[0][at]), int(first[1][at])))
        else:
            value = int(cc._pick(rng, (int(cc._pick(rng, BOUNDS[kind])), KIND_MIN[kind], KIND_MAX[kind], TRAP[kind])))
            r = dataclasses.replace(r, after=(int(rng.integers(m.n_docs)), value))
    return r


def _fuzz_mask_request(rng, m: Model) -> Req:
    """1-3 clauses over the 64-bit columns one leaf holds: exists, or a range between two of the kind's bounds"""
    leaf = int(rng.integers(len(m.sizes)))
    keys = [key for key in FUZZ_COLUMNS if m.columns[key][leaf] is not None]
    clauses = []
    for _ in range(int(rng.integers(1, 4))):
        key = cc._pick(rng, keys)
        clauses.append((key, "exists") if rng.random() < 0.25 else (key, "range") + _bounds64(rng, key[1]))
    return Req("mask64", leaf=leaf, value_clauses=tuple(clauses))


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
            n = int(rng.integers(1, 17))
            batches.append((entry, [_fuzz_mask_request(rng, m) if entry == "mask64" else _fuzz_request(rng, m, entry) for _ in range(n)]))
    return m, batches
