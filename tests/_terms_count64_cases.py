"""The indexes and requests of tests/test_terms_count64_gpu.py and the seeded fuzz it runs, built from explicit layouts or a seed.
Pure NumPy until upload() / run() are called; what each request must return comes from tests/_terms_count64_ref.py alone.
tests/test_terms_count64_host.py checks, without a device, the condition every fuzz round must meet.

  column   (kind, name), kind "long" | "double": per leaf None (the leaf lacks the column) or (docs or None = every doc, value bits
           uint64).  Beside them every index has two 32-bit int columns for the doc sets' own range clauses: R_SINGLE (single-valued)
           and R_MULTI (0-3 values per doc)
  request  Req: a text query (clauses, need / must, masks) or a doc set (masks, 32-bit range clauses), the counted column, max_buckets
"""
from __future__ import annotations

import dataclasses
import functools
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from nrtsearch_amd import api, synth

from tests import _docset_ref as dsr
from tests import _field_sort64_ref as f64
from tests import _field_sort_ref as fs
from tests import _multi_values_ref as mref
from tests import _terms_count64_ref as ref
from tests._column64_cases import POOLS as POOLS64

Key = Tuple[str, str]
EPOCH = 1_700_000_000_000
INT64_MIN, INT64_MAX = f64.INT64_MIN, f64.INT64_MAX
R_SINGLE_FIELD, R_MULTI_FIELD, FIRST_COLUMN_FIELD = 8, 9, 20
MASKS = ((5, 0.6), (6, 0.2))


def u64(values) -> np.ndarray:
    return np.array([int(v) & (f64.U64 - 1) for v in values], dtype=np.uint64)


D = lambda v: f64.bits_of("double", v)   # noqa: E731
NANS = (0x7FF8000000000000, 0x7FF0000000000001, 0xFFF8000000000123, 0x7FF8000000000123)   # three payloads, both signs
LONG_EDGE = u64([INT64_MIN, INT64_MIN + 1, -1, 0, 1, INT64_MAX - 1, INT64_MAX])
DOUBLE_EDGE = u64([0xFFF0000000000000, 0x8000000000000000, 0, 1, 0x7FEFFFFFFFFFFFFF, 0x7FF0000000000000]) # -inf, -0.0, +0.0, least subnormal, DBL_MAX, +inf
# the value pools of index A's columns.  many: 700 values, neighbours further apart than 2^29 (longs) / spread over both signs
# (doubles): a bucket key that keeps either half of the value merges some
POOLS: Dict[Key, np.ndarray] = {
    ("long", "const"): u64([EPOCH]),
    ("long", "two"): u64([EPOCH, EPOCH + 2**32]),
    ("long", "many"): u64([EPOCH + (j - 350) * (2**29 + 1) for j in range(700)]),
    ("long", "halves"): POOLS64[("long", "halves")],
    ("long", "edge"): LONG_EDGE,
    ("long", "min_only"): u64([INT64_MIN]),
    ("long", "min3"): u64([INT64_MIN, -7, EPOCH]),
    ("long", "max_only"): u64([INT64_MAX]),
    ("long", "max3"): u64([INT64_MAX, -7, EPOCH]),
    ("double", "const"): u64([D(3.25)]),
    ("double", "two"): u64([D(3.25), D(-3.25)]),
    ("double", "many"): u64([D(1.5) + j * (2**21 + 1) for j in range(350)] + [D(-1.5) + j * (2**21 + 1) for j in range(350)]),
    ("double", "edge"): np.concatenate([DOUBLE_EDGE, u64(NANS)]),
}
EXTREMES = {"long": u64([INT64_MIN, INT64_MAX, 0, -1]), "double": u64([0xFFF0000000000000, NANS[0], NANS[2], 0x8000000000000000, 0])}


@dataclasses.dataclass(frozen=True)
class Req:
    column: Key
    max_buckets: int
    docset: bool = False
    clauses: Tuple[int, ...] = (1,)
    need: int = 1
    must: bool = False
    filters: Tuple[int, ...] = ()
    must_nots: Tuple[int, ...] = ()
    ranges: Tuple[Tuple[str, int, int], ...] = ()   # doc sets: ("s" | "m", lower, upper) over R_SINGLE / R_MULTI, ints, inclusive


class Index:
    def __init__(self, corpus, columns: Dict[Key, list], masks: Dict[int, list], r_single: list, r_multi: list,
                 slicing: Optional[Tuple[int, int, int]] = None, target_items: int = 0):
        self.corpus, self.columns, self.masks, self.r_single, self.r_multi = corpus, columns, masks, r_single, r_multi
        self.slicing, self.target_items = slicing, target_items
        self.sizes = [seg.max_doc for seg in corpus.segments]
        self.field = {key: FIRST_COLUMN_FIELD + i for i, key in enumerate(columns)}
        self._hits: dict = {}

    def hits(self, r: Req):
        memo = (r.docset, r.clauses, r.need, r.must, r.filters, r.must_nots, r.ranges)
        if memo not in self._hits:
            f, mn = [self.masks[m] for m in r.filters], [self.masks[m] for m in r.must_nots]
            if r.docset:
                f = f + [mref.any_in_range(self.corpus, "int", self.r_multi, fs.bits_of("int", lo), fs.bits_of("int", hi)) for a, lo, hi in r.ranges if a == "m"]
                rs = [("int", self.r_single, fs.bits_of("int", lo), fs.bits_of("int", hi)) for a, lo, hi in r.ranges if a == "s"]
                self._hits[memo] = dsr.hit_set(self.corpus, f, mn, rs)
            else:
                accept = dsr.hit_set(self.corpus, f, mn) if f or mn else None   # (liveDocs & FILTER & ~MUST_NOT)
                self._hits[memo] = ref.text_hits(self.corpus, r.clauses, len(r.clauses) if r.must else r.need, accept=accept)
        return self._hits[memo]

    def expected(self, r: Req):
        return ref.count(self.corpus, self.hits(r), self.columns[r.column], r.column[0], r.max_buckets)

    def distinct(self, r: Req) -> int:
        return ref.distinct(self.corpus, self.hits(r), self.columns[r.column], r.column[0])

    def unvalued(self, r: Req) -> int:
        return ref.unvalued_hits(self.corpus, self.hits(r), self.columns[r.column])

    def collector(self, r: Req) -> api.TermsCollector:
        return api.TermsCollector(self.field[r.column], 10, True, r.column[0])


def query_of(r: Req):
    f, mn = tuple(api.MaskFilter(m) for m in r.filters), tuple(api.MaskFilter(m) for m in r.must_nots)
    if r.docset:
        return api.DocSetQuery(f, mn, tuple(api.RangeClause(R_SINGLE_FIELD if a == "s" else R_MULTI_FIELD, "int", int(lo), int(hi)) for a, lo, hi in r.ranges))
    t = tuple(api.TermQuery(0, c) for c in r.clauses)
    if r.must:
        return api.BooleanQuery((), 0, f, mn, t)
    if len(t) == 1 and not f and not mn:
        return t[0]
    return api.BooleanQuery(t, max(r.need, 1), f, mn)


def describe(r: Req) -> str:
    return (f"{'docset' if r.docset else 'text'} {r.column[0]}/{r.column[1]} max_buckets {r.max_buckets} clauses {r.clauses} need {r.need} must {r.must} "
            f"filters {r.filters} must_nots {r.must_nots} ranges {r.ranges}")


def _values(col):
    """(values, docs) as add_doc_values* takes them (an empty column: slices of real arrays, no NULL pointer)"""
    if col[0] is not None and len(col[0]) == 0:
        return np.zeros(1, col[1].dtype)[:0], np.zeros(1, np.int32)[:0]
    return np.ascontiguousarray(col[1]), None if col[0] is None else np.ascontiguousarray(col[0], dtype=np.int32)


def upload(ctx, ix: Index, more=None):
    """-> (leaves, searcher); more(g, si): further uploads before the seal"""
    leaves = []
    for si, seg in enumerate(ix.corpus.segments):
        g = api.GpuSegment(ctx, seg.max_doc, seg.doc_base)
        leaves.append(g)
        g.add_field_norms(0, seg.norms)
        g.add_terms(0, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
        for key, cols in ix.columns.items():
            if cols[si] is not None:
                v, d = _values(cols[si])
                g.add_doc_values64(ix.field[key], key[0], v if v.dtype == np.uint64 else v.astype(np.uint64), d)
        if ix.r_single[si] is not None:
            v, d = _values(ix.r_single[si])
            g.add_doc_values(R_SINGLE_FIELD, "int", v if v.dtype == np.uint32 else v.astype(np.uint32), d)
        if ix.r_multi[si] is not None:
            vd, vb = ix.r_multi[si]
            if len(vd):
                g.add_doc_values_multi(R_MULTI_FIELD, "int", np.ascontiguousarray(vb, dtype=np.uint32), np.ascontiguousarray(vd, dtype=np.int32))
            else:
                g.add_doc_values_multi(R_MULTI_FIELD, "int", np.zeros(1, np.uint32)[:0], np.zeros(1, np.int32)[:0])
        if more is not None:
            more(g, si)
        g.seal()
        if seg.live_bits is not None:
            g.set_live_docs(seg.live_bits)
        for mid, words in ix.masks.items():
            g.set_mask(mid, words[si])
    return leaves, api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics.from_corpus(ix.corpus))


def run(searcher, ix: Index, reqs: Sequence[Req]):
    """one call of the entry the requests belong to (all text or all doc sets)"""
    assert len({r.docset for r in reqs}) == 1
    fn = api.count_docset_terms64_batch if reqs[0].docset else api.count_terms64_batch
    return fn(searcher, [query_of(r) for r in reqs], [ix.collector(r) for r in reqs], [r.max_buckets for r in reqs])


def supported(searcher, ix: Index, r: Req) -> bool:
    fn = api.count_docset_terms64_supported if r.docset else api.count_terms64_supported
    return fn(searcher, query_of(r), ix.collector(r), r.max_buckets)


def check(name: str, kind: str, got, exp) -> None:
    bits, counts, n, total, with_value, overflowed = exp
    assert got.overflowed == bool(overflowed), f"{name}: overflowed {got.overflowed}, the reference says {overflowed}"
    assert got.total_hits == total, f"{name}: total_hits {got.total_hits}, the reference counts {total}"
    assert got.hits_with_value == with_value, f"{name}: hits_with_value {got.hits_with_value}, the reference counts {with_value}"
    assert got.value_bits.dtype == np.uint64 and got.values.dtype == f64.DTYPES[kind], f"{name}: dtypes"
    assert got.value_bits.tolist() == bits.tolist(), f"{name}: values and their order"
    assert got.counts.tolist() == counts.tolist(), f"{name}: counts"
    assert len(got.counts) == n, f"{name}: n_buckets"


# ---- the 32-bit columns of the doc sets' range clauses ---------------------------------------------------------------------------------
def _range32(rng, n: int):
    """-> (R_SINGLE: a value in -3..3 on ~90 % of the docs, R_MULTI: 0-3 values in -3000..3000 per doc as (value docs, value bits))"""
    d = np.nonzero(rng.random(n) < 0.9)[0].astype(np.int32)
    single = (d, rng.integers(-3, 4, size=len(d)).astype(np.int32).view(np.uint32))
    per_doc = rng.integers(0, 4, size=n)
    vd = np.repeat(np.arange(n, dtype=np.int32), per_doc)
    multi = (vd, rng.integers(-3000, 3001, size=len(vd)).astype(np.int32).view(np.uint32))
    return single, multi


def _masks(corpus, seed: int):
    return {mid: [synth.random_mask(seg.max_doc, dens, seed + 50 * mid + si) for si, seg in enumerate(corpus.segments)] for mid, dens in MASKS}


# ---- index A -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def index_a() -> Index:
    """leaves of 2500, 700 and 300 docs, 5 % deletes; every column on every doc of leaf 0, on ~80 % of leaf 1, absent from leaf 2"""
    sizes = (2500, 700, 300)
    corpus = fs.make_corpus(sizes, {1: 0.5, 2: 0.3, 3: 0.2}, seed=21, delete_fraction=0.05)
    rng = np.random.default_rng(22)
    d1 = np.nonzero(rng.random(sizes[1]) < 0.8)[0].astype(np.int32)
    columns = {}
    for key, pool in POOLS.items():
        v0 = rng.choice(pool, size=sizes[0])
        v0[: len(pool)] = pool          # every value of the pool is there
        columns[key] = [(None, v0), (d1, rng.choice(pool, size=len(d1))), None]
    r32 = [_range32(rng, n) for n in sizes]
    return Index(corpus, columns, _masks(corpus, 0), [s for s, _ in r32], [m for _, m in r32])


TEXT_SHAPES = (dict(clauses=(1,)), dict(clauses=(1, 2, 3)), dict(clauses=(1, 2, 3), need=2), dict(clauses=(1, 2), must=True),
               dict(clauses=(1, 2, 3), filters=(5,), must_nots=(6,)))
DOCSET_SHAPES = (dict(), dict(filters=(5,)), dict(filters=(5,), must_nots=(6,)), dict(ranges=(("s", -1, 2),)), dict(ranges=(("m", -500, 1500),)),
                 dict(filters=(5,), ranges=(("m", -2000, 0), ("s", -3, 1))))


def shapes(docset: bool):
    return [dict(docset=True, **s) for s in DOCSET_SHAPES] if docset else [dict(s) for s in TEXT_SHAPES]


# ---- the fuzz ------------------------------------------------------------------------------------------------------------------------
FUZZ_POOLS: Dict[Key, np.ndarray] = {
    ("long", "two"): POOLS[("long", "two")],
    ("long", "many"): POOLS[("long", "many")],
    ("long", "halves"): POOLS[("long", "halves")],
    ("long", "edge"): np.concatenate([LONG_EDGE, EXTREMES["long"]]),
    ("double", "many"): POOLS[("double", "many")],
    ("double", "edge"): np.concatenate([POOLS[("double", "edge")], EXTREMES["double"]]),
    ("double", "const"): POOLS[("double", "const")],
}
FUZZ_SIZES = (1, 2, 63, 64, 65, 200, 700, 1023, 1024, 1025, 2049, 3000)


def _pick(rng, seq):
    return seq[int(rng.integers(len(seq)))]


@functools.lru_cache(maxsize=2)
def fuzz_round(base: int, round_: int):
    """-> (index, [[Req]]): 1-3 leaves of 1-3000 docs, random presence, deletes, masks, slicing / target_items; four batches (two text,
    two doc sets) of 1-16 requests over both kinds, max_buckets drawn around the distinct count of each request's hits.
    Replay one case: fuzz_round(base, round_)[1][batch][index]."""
    rng = np.random.Generator(np.random.PCG64(base + round_))
    sizes = tuple(int(_pick(rng, FUZZ_SIZES)) if rng.random() < 0.7 else int(rng.integers(1, 3001)) for _ in range(int(rng.integers(1, 4))))
    corpus = fs.make_corpus(sizes, {1: 1.0, 2: 0.5, 3: 0.1}, seed=base + 1000 + round_, delete_fraction=float(_pick(rng, (0.0, 0.1, 0.3))))
    columns: Dict[Key, list] = {}
    for key, pool in FUZZ_POOLS.items():
        cols = []
        for n in sizes:
            presence = float(_pick(rng, (1.0, 0.9, 0.5, 0.0)))
            if presence == 0.0 and len(sizes) > 1 and rng.random() < 0.5:
                cols.append(None)            # the leaf lacks the column
                continue
            d = np.nonzero(rng.random(n) < presence)[0].astype(np.int32)
            cols.append((None, rng.choice(pool, size=n)) if presence == 1.0 else (d, rng.choice(pool, size=len(d))))
        if all(c is None for c in cols):
            cols[0] = (None, rng.choice(pool, size=sizes[0]))   # (a column resident on no leaf is a refusal, not a case)
        columns[key] = cols
    r32 = [_range32(rng, n) for n in sizes]
    slicing = _pick(rng, (None, None, (1000, 5, 1), (1000, 2, 1)))
    ix = Index(corpus, columns, _masks(corpus, base + round_), [s for s, _ in r32], [m for _, m in r32], slicing=slicing,
               target_items=int(_pick(rng, (0, 0, 7, 64))))
    keys = list(FUZZ_POOLS)
    batches = []
    for docset in (False, True, False, True):
        reqs = []
        for _ in range(int(rng.integers(1, 17))):
            r = Req(_pick(rng, keys), 1, **_pick(rng, shapes(docset)))
            n = ix.distinct(r)
            b = int(_pick(rng, (n, n - 1, n + 1, max(n // 2, 1), 2 * n + 3, 1, 4096)))
            reqs.append(dataclasses.replace(r, max_buckets=min(max(b, 1), 65536)))
        batches.append(reqs)
    return ix, batches
