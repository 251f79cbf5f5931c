"""The numeric range facet (nrtgpu_count_ranges_batch, nrtgpu_count_docset_ranges_batch) through the C ABI on the device, against
tests/_range_count_ref.py.  Every comparison is exact equality of (counts, total_hits, hits_with_value).  Needs a real MI355X."""
import ctypes as C

import numpy as np
import pytest

from nrtsearch_amd import _lib, api, synth

from tests import _column_cases as cc
from tests import _field_sort_ref as fs
from tests import _multi_values_ref as mv
from tests import _range_count_ref as ref

pytestmark = pytest.mark.gpu
TERMS = {1: 0.5, 2: 0.3, 3: 0.2}
T = {t: api.TermQuery(0, t) for t in (1, 2, 3, 99)}
# the terms tests' eight shapes: (name, query, clauses, clauses a hit matches at least, reads the masks)
QUERIES = [
    ("term", T[1], (1,), 1, False),
    ("or3", api.BooleanQuery((T[1], T[2], T[3])), (1, 2, 3), 1, False),
    ("msm2of3", api.BooleanQuery((T[1], T[2], T[3]), 2), (1, 2, 3), 2, False),
    ("must2", api.BooleanQuery((), 0, (), (), (T[1], T[2])), (1, 2), 2, False),
    ("masks", api.BooleanQuery((T[1], T[2], T[3]), 1, (api.MaskFilter(5),), (api.MaskFilter(6),)), (1, 2, 3), 1, True),
    ("nowhere", T[99], (99,), 1, False),
    ("msm2_dup", api.BooleanQuery((T[2], T[2], T[3]), 2), (2, 2, 3), 2, False),
    ("must3_dup", api.BooleanQuery((), 0, (), (), (T[1], T[1], T[2])), (1, 1, 2), 3, False),
]
FIELD = {"int": 10, "float": 11, "long": 12, "double": 13}
MCOL = 15   # a multi-valued int column, for the doc set's own range clauses
ALL = api.DocSetQuery()


@pytest.fixture(scope="module", autouse=True)
def two_column_postings():
    """The text entry refuses packed postings (tested below): these contexts keep the two-column layout also where the whole suite
    runs with NRTGPU_PACKED_POSTINGS=1."""
    mp = pytest.MonkeyPatch()
    mp.delenv("NRTGPU_PACKED_POSTINGS", raising=False)
    yield
    mp.undo()


@pytest.fixture(scope="module")
def ctx(two_column_postings):
    c = api.GpuContext(device_id=0, max_batch=256)
    yield c
    c.close()


def release(leaves):
    for l in leaves:
        l.release()


def same(name, got, exp):
    counts, total, valued = exp
    assert got.total_hits == total, f"{name}: total_hits {got.total_hits}, the reference counts {total}"
    assert got.hits_with_value == valued, f"{name}: hits_with_value {got.hits_with_value}, the reference has {valued}"
    assert got.counts.dtype == np.int64 and got.counts.tolist() == counts, f"{name}: counts {got.counts.tolist()}, the reference has {counts}"


def add_column(g, field, kind, bits, docs=None):
    if kind in ref.WIDE:
        g.add_doc_values64(field, kind, np.asarray(bits, dtype=np.uint64), docs)
    else:
        g.add_doc_values(field, kind, np.asarray(bits, dtype=np.uint32), docs)


def counter(kind, ranges, field=None):
    return api.RangeCounter(FIELD[kind] if field is None else field, kind, tuple(ranges))


# ---- index A: leaves of 3000, 1500 and 40 docs, 1 % deletes; a column of each kind on 80 % of leaf 0, all of leaf 1, absent from
# ---- leaf 2; a multi-valued int column (two values per doc) for the doc set's range clauses
class IndexA:
    def __init__(self, ctx, corpus):
        rng = np.random.default_rng(41)
        self.corpus = corpus
        self.columns = {}
        for kind in ref.KINDS:
            pool = np.array(ref.POOL[kind], dtype=ref.BITS_DTYPE[kind])
            d0 = np.nonzero(rng.random(3000) < 0.8)[0].astype(np.int32)
            self.columns[kind] = [(d0, rng.choice(pool, size=len(d0))), (None, rng.choice(pool, size=1500)), None]
        self.multi = []
        for seg in corpus.segments:
            vd = np.repeat(np.arange(seg.max_doc, dtype=np.int32), 2)
            self.multi.append((vd, rng.integers(-50, 50, size=len(vd)).astype(np.int32).view(np.uint32)))
        self.masks = {(si, mid): synth.random_mask(seg.max_doc, dens, 40 * mid + si)
                      for si, seg in enumerate(corpus.segments) for mid, dens in ((5, 0.6), (6, 0.2))}
        for si, seg in enumerate(corpus.segments):   # mask 8: whole 64-doc words without an accepted doc
            w = np.full((seg.max_doc + 63) // 64, 2**64 - 1, dtype=np.uint64)
            w[1::3] = 0
            w[16:32] = 0                             # (and the whole second 1024-doc sub-tile of leaves 0 and 1)
            self.masks[(si, 8)] = w
        self.accept = [synth.accept_words(seg, self.masks[(si, 5)], self.masks[(si, 6)]) for si, seg in enumerate(corpus.segments)]
        self.leaves = []
        for si, seg in enumerate(corpus.segments):
            g = api.GpuSegment(ctx, seg.max_doc, seg.doc_base)
            g.add_field_norms(0, seg.norms)
            g.add_terms(0, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
            for kind, cols in self.columns.items():
                if cols[si] is not None:
                    add_column(g, FIELD[kind], kind, cols[si][1], cols[si][0])
            g.add_doc_values_multi(MCOL, "int", self.multi[si][1], self.multi[si][0])
            g.seal()
            g.set_live_docs(seg.live_bits)
            self.leaves.append(g)
        for (si, mid), bits in self.masks.items():
            self.leaves[si].set_mask(mid, bits)
        self.searcher = api.GpuIndexSearcher(ctx, self.leaves, api.IndexStatistics.from_corpus(corpus))

    def mask(self, mid):
        return [self.masks[(si, mid)] for si in range(len(self.corpus.segments))]

    def text_hits(self, clauses, need, masked, **kw):
        return ref.text_hits(self.corpus, clauses, need, accept=self.accept if masked else None, **kw)

    def expect(self, kind, hits, ranges):
        return ref.count(self.corpus, hits, self.columns[kind], kind, ranges)


@pytest.fixture(scope="module")
def ix(ctx):
    corpus = fs.make_corpus([3000, 1500, 40], TERMS, seed=5, delete_fraction=0.01)
    assert all(seg.live_bits is not None for seg in corpus.segments)
    x = IndexA(ctx, corpus)
    yield x
    release(x.leaves)


@pytest.mark.parametrize("kind", ref.KINDS)
def test_every_query_shape_over_every_range_list(ix, kind):
    lists = ref.range_lists(kind)
    cases = [(name, ranges, q) for name, ranges in lists for q in QUERIES]
    before = ix.searcher.ctx.stats()
    got = api.count_ranges_batch(ix.searcher, [q[1] for _, _, q in cases], [counter(kind, ranges) for _, ranges, _ in cases])
    d = api.GpuContext.last_diagnostics()
    after = ix.searcher.ctx.stats()
    assert d["items_maxscore"] == 0 and d["items_scan"] >= len(cases) * 5 // 8
    assert after["scan_launches"] == before["scan_launches"] + 1 and after["fixed_point_launches"] == before["fixed_point_launches"] + 1
    assert after["maxscore_launches"] == before["maxscore_launches"]
    by_name = {}
    for (name, ranges, (qname, _, clauses, need, masked)), rc in zip(cases, got):
        exp = ix.expect(kind, ix.text_hits(clauses, need, masked), ranges)
        same(f"{kind}_{name}_{qname}", rc, exp)
        assert (exp[1] == 0) == (qname == "nowhere") and (exp[2] < exp[1] or qname == "nowhere")   # some hit lacks a value
        by_name[(name, qname)] = exp[0]
    # what the lists are for, read off the reference (so the comparison above is not vacuous)
    c = by_name[("nested", "or3")]
    assert c[0] >= c[1] >= c[2] > 0 and c[0] > c[2]
    c = by_name[("twice", "or3")]
    assert c[0] == c[1] > 0
    c = by_name[("touching", "or3")]
    assert c[0] > 0 and c[1] > 0
    assert by_name[("empty", "or3")][0] == 0 and by_name[("empty", "or3")][1] > 0 and by_name[("none_inside", "or3")] == [0]
    assert by_name[("single", "or3")][0] > 0 and by_name[("to_greatest", "or3")][0] > 0 and by_name[("from_least", "or3")][0] > 0
    c = by_name[("sixty_four", "or3")]
    assert len(c) == 64 and sum(x == 0 for x in c) >= 5 and sum(x > 0 for x in c) >= 20
    assert api.count_ranges_supported(ix.searcher, QUERIES[2][1], counter(kind, lists[0][1])) is True


def test_what_only_a_full_width_compare_gets_right(ix):
    """INT64 values that agree in their low words (5, 2^32 + 5, 2^33 + 5) fall into three ranges; 1.5 + j ulp into seven; the three
    NaN payloads into [NaN, NaN] and out of [-inf, +inf]; -0.0 and +0.0 into different ranges."""
    L, D, F = (lambda v: ref.bits_of("long", v)), (lambda v: ref.bits_of("double", v)), (lambda v: ref.bits_of("float", v))
    hits = ix.text_hits((1, 2, 3), 1, False)
    or3 = QUERIES[1][1]
    longs = [(L(5), L(5)), (L(2**32 + 5), L(2**32 + 5)), (L(2**33 + 5), L(2**33 + 5)), (L(0), L(2**32 - 1)), (L(2**32), L(2**63 - 1)), (L(-2**32 - 5), L(-1))]
    doubles = [(D(1.5) + j, D(1.5) + j) for j in range(7)] + [(0x7FF8000000000000, 0x7FF8000000000000), (D(-np.inf), D(np.inf)), (D(-0.0), D(-0.0)), (D(0.0), D(0.0))]
    got = api.count_ranges_batch(ix.searcher, [or3, or3], [counter("long", longs), counter("double", doubles)])
    for kind, ranges, rc in (("long", longs, got[0]), ("double", doubles, got[1])):
        exp = ix.expect(kind, hits, ranges)
        same(f"full_width_{kind}", rc, exp)
        assert all(c > 0 for c in exp[0]) and len(set(exp[0][:3])) > 1
    floats = [(0x7FC00000, 0xFFC12345), (F(-np.inf), F(np.inf)), (F(-0.0), F(-0.0)), (F(0.0), F(0.0)), (F(-0.0), F(0.0))]
    rc = api.count_ranges_batch(ix.searcher, [or3], [counter("float", floats)])[0]
    exp = ix.expect("float", hits, floats)
    same("full_width_float", rc, exp)
    assert exp[0][0] > 0 and exp[0][0] + exp[0][1] == exp[2] and exp[0][2] + exp[0][3] == exp[0][4] and exp[0][2] > 0 and exp[0][3] > 0


# ---- 13 000 docs in one leaf: ONE item, every wave of it shares the LDS counters ----------------------------------------------------
def test_one_item_whose_waves_share_the_counters(ctx):
    n = 13_000
    corpus = fs.make_corpus([n], {1: 0.6, 2: 0.01}, seed=8)
    seg = corpus.segments[0]
    rng = np.random.default_rng(9)
    columns = {kind: [(None, rng.choice(np.array(ref.POOL[kind], dtype=ref.BITS_DTYPE[kind]), size=n))] for kind in ref.KINDS}
    g = api.GpuSegment(ctx, n, 0)
    try:
        g.add_field_norms(0, seg.norms)
        g.add_terms(0, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
        for kind in ref.KINDS:
            add_column(g, FIELD[kind], kind, columns[kind][0][1])
        g.seal()
        searcher = api.GpuIndexSearcher(ctx, [g], api.IndexStatistics.from_corpus(corpus))
        hits = ref.text_hits(corpus, (1,), 1)
        for kind in ref.KINDS:
            lists = ref.range_lists(kind)
            got = api.count_ranges_batch(searcher, [T[1]], [counter(kind, lists[-1][1])])
            assert api.GpuContext.last_diagnostics()["items_scan"] == 1
            same(f"one_item_{kind}_sixty_four", got[0], ref.count(corpus, hits, columns[kind], kind, lists[-1][1]))
            got = api.count_ranges_batch(searcher, [T[1]] * len(lists), [counter(kind, r) for _, r in lists])
            for (name, r), rc in zip(lists, got):
                same(f"one_item_{kind}_{name}", rc, ref.count(corpus, hits, columns[kind], kind, r))
            assert got[0].total_hits > 7000
    finally:
        g.release()


# ---- 300 000 docs: a query cut into several items, which meet in the global counters ---------------------------------------------
def test_several_items_meet_in_the_global_counters(ctx):
    n = 300_000
    corpus = fs.make_corpus([n], {1: 1.0}, seed=10)
    seg = corpus.segments[0]
    mod = (np.arange(n) % 1000).astype(np.int64)
    i_bits = mod.astype(np.int32).view(np.uint32)
    l_bits = (mod + 2**32 - 500).view(np.uint64)
    g = api.GpuSegment(ctx, n, 0)
    try:
        g.add_field_norms(0, seg.norms)
        g.add_terms(0, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
        g.add_doc_values(7, "int", i_bits)
        g.add_doc_values64(8, "long", l_bits)
        g.seal()
        searcher = api.GpuIndexSearcher(ctx, [g], api.IndexStatistics.from_corpus(corpus))
        hits = [np.ones(n, dtype=bool)]
        I, L = (lambda v: ref.bits_of("int", v)), (lambda v: ref.bits_of("long", v + 2**32 - 500))
        four = [(0, 99), (100, 499), (50, 149), (999, 5000)]
        got = api.count_ranges_batch(searcher, [T[1]], [counter("int", [(I(a), I(b)) for a, b in four], 7)])
        assert api.GpuContext.last_diagnostics()["items_scan"] >= 2    # (the planner cuts the query: its items share the counters)
        same("items_int", got[0], ref.count(corpus, hits, [(None, i_bits)], "int", [(I(a), I(b)) for a, b in four]))
        assert got[0].counts.tolist() == [100 * 300, 400 * 300, 100 * 300, 300] and got[0].total_hits == n == got[0].hits_with_value
        # a batch whose queries have different n_ranges: the cut_off / counter_off arithmetic
        rng = np.random.default_rng(12)
        for kind, field, bits, B in (("long", 8, l_bits, L), ("int", 7, i_bits, I)):
            lists = []
            for n_ranges in (1, 5, 64, 3, 64, 2):
                ends = rng.integers(-20, 1020, size=(n_ranges, 2))
                lists.append([(B(int(min(a, b))), B(int(max(a, b)))) for a, b in ends])
            got = api.count_ranges_batch(searcher, [T[1]] * len(lists), [counter(kind, r, field) for r in lists])
            assert api.GpuContext.last_diagnostics()["items_scan"] >= 2 * len(lists)
            for i, (r, rc) in enumerate(zip(lists, got)):
                same(f"items_batch_{kind}_{i}", rc, ref.count(corpus, hits, [(None, bits)], kind, r))
        docs = api.count_docset_ranges_batch(searcher, [ALL, ALL], [counter("long", lists[2], 8), counter("long", [(L(0), L(99))], 8)])
        same("items_docset_0", docs[0], ref.count(corpus, hits, [(None, l_bits)], "long", lists[2]))
        same("items_docset_1", docs[1], ([30000], n, n))
    finally:
        g.release()


# ---- max_doc at the word and sub-tile edges, a counted value in the last doc, stray mask bits beyond it ---------------------------
@pytest.mark.parametrize("n", [63, 64, 65, 1023, 1024, 1025])
def test_max_doc_edges_with_a_counted_value_in_the_last_doc(ctx, n):
    corpus = fs.make_corpus([n], {1: 1.0}, seed=20 + n % 7)
    seg = corpus.segments[0]
    vals = np.arange(n, dtype=np.int64)
    i_bits, l_bits = vals.astype(np.int32).view(np.uint32), (vals + 2**32 - 10).view(np.uint64)
    live = np.full((n + 63) // 64, 2**64 - 1, dtype=np.uint64)
    live[0] &= ~np.uint64(2)                       # doc 1 deleted
    if n % 64:
        live[-1] &= np.uint64((1 << (n % 64)) - 1)
    keep = synth.random_mask(n, 0.7, 300 + n)
    keep[(n - 1) >> 6] |= np.uint64(1 << ((n - 1) & 63))   # the last doc stays
    g = api.GpuSegment(ctx, n, 0)
    try:
        g.add_field_norms(0, seg.norms)
        g.add_terms(0, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
        g.add_doc_values(7, "int", i_bits)
        g.add_doc_values64(8, "long", l_bits)
        g.seal()
        g.set_live_docs(cc.dirty(live, n))         # ones at and beyond max_doc: ignored
        g.set_mask(5, cc.dirty(keep, n))
        searcher = api.GpuIndexSearcher(ctx, [g], api.IndexStatistics.from_corpus(corpus))
        hits = [fs._bits(live, n) & fs._bits(keep, n)]
        I, L = (lambda v: ref.bits_of("int", v)), (lambda v: ref.bits_of("long", v + 2**32 - 10))
        for kind, field, bits, B in (("int", 7, i_bits, I), ("long", 8, l_bits, L)):
            ranges = [(B(n - 1), B(n - 1)), (B(0), B(n - 1)), (B(n), B(n + 2000)), (B(n - 2), B(n + 5)), (B(1), B(1))]
            exp = ref.count(corpus, hits, [(None, bits)], kind, ranges)
            assert exp[0][0] == 1 and exp[0][1] == exp[2] == exp[1] and exp[0][2] == 0 and exp[0][4] == 0
            text = api.count_ranges_batch(searcher, [api.BooleanQuery((T[1],), 1, (api.MaskFilter(5),))], [counter(kind, ranges, field)])[0]
            same(f"edge_{n}_{kind}_text", text, exp)
            docs = api.count_docset_ranges_batch(searcher, [api.DocSetQuery((api.MaskFilter(5),))], [counter(kind, ranges, field)])[0]
            same(f"edge_{n}_{kind}_docset", docs, exp)
    finally:
        g.release()


def test_a_fork_with_more_deletes_reads_the_shared_column(ix):
    corpus = ix.corpus
    lives, forks = [], []
    try:
        for si, (seg, leaf) in enumerate(zip(corpus.segments, ix.leaves)):
            n = (seg.max_doc + 63) // 64
            live = seg.live_bits[:n] & ~synth.random_mask(seg.max_doc, 0.3, 900 + si)[:n]
            lives.append(live)
            forks.append(leaf.fork(live))
        searcher = api.GpuIndexSearcher(ix.searcher.ctx, forks, api.IndexStatistics.from_corpus(corpus))
        _, query, clauses, need, _ = QUERIES[2]
        for kind in ("int", "double"):
            ranges = ref.range_lists(kind)[1][1]
            got = api.count_ranges_batch(searcher, [query], [counter(kind, ranges)])[0]
            same(f"fork_{kind}", got, ix.expect(kind, ref.text_hits(corpus, clauses, need, live=lives), ranges))
            parent = api.count_ranges_batch(ix.searcher, [query], [counter(kind, ranges)])[0]
            same(f"fork_parent_{kind}", parent, ix.expect(kind, ix.text_hits(clauses, need, False), ranges))
            assert parent.total_hits > got.total_hits and parent.hits_with_value > got.hits_with_value
            docs = api.count_docset_ranges_batch(searcher, [ALL], [counter(kind, ranges)])[0]
            same(f"fork_docset_{kind}", docs, ix.expect(kind, ref.docset_hits(_with_live(corpus, lives)), ranges))
    finally:
        release(forks)


class _Leaf:
    def __init__(self, seg, live):
        self.max_doc, self.doc_base, self.live_bits = seg.max_doc, seg.doc_base, live


class _with_live:
    """the corpus with other liveDocs words (what the doc-set reference reads of a corpus)"""
    def __init__(self, corpus, lives):
        self.segments = [_Leaf(seg, live) for seg, live in zip(corpus.segments, lives)]


# ---- the doc-set entry ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ref.KINDS)
def test_doc_sets_over_every_range_list(ix, kind):
    """Match-all, FILTER / MUST_NOT masks, the doc set's own 32-bit range clauses -- single-valued, multi-valued, both -- beside a
    count over a column of either width, and a mask that leaves whole 64-doc words (and a whole sub-tile) without an accepted doc."""
    I = lambda v: ref.bits_of("int", v)   # noqa: E731
    RC = api.RangeClause
    icols = ix.columns["int"]
    any_multi = mv.any_in_range(ix.corpus, "int", ix.multi, I(-10), I(3))
    sets = [
        ("all", ALL, ref.docset_hits(ix.corpus)),
        ("masks", api.DocSetQuery((api.MaskFilter(5),), (api.MaskFilter(6),)), ref.docset_hits(ix.corpus, [ix.mask(5)], [ix.mask(6)])),
        ("range32", api.DocSetQuery(ranges=(RC(FIELD["int"], "int", -1, 9),)), ref.docset_hits(ix.corpus, ranges32=((icols, "int", I(-1), I(9)),))),
        ("range_multi", api.DocSetQuery(ranges=(RC(MCOL, "int", -10, 3),)), ref.docset_hits(ix.corpus, [any_multi])),
        ("range_both", api.DocSetQuery((api.MaskFilter(5),), (), (RC(MCOL, "int", -10, 3), RC(FIELD["int"], "int", -1000, 500))),
         ref.docset_hits(ix.corpus, [ix.mask(5), any_multi], (), ((icols, "int", I(-1000), I(500)),))),
        ("empty_words", api.DocSetQuery((api.MaskFilter(8),)), ref.docset_hits(ix.corpus, [ix.mask(8)])),
        ("nothing", api.DocSetQuery(ranges=(RC(FIELD["int"], "int", 9, -1),)), [np.zeros(s.max_doc, dtype=bool) for s in ix.corpus.segments]),
    ]
    lists = ref.range_lists(kind)
    cases = [(sname, d, hits, lname, ranges) for sname, d, hits in sets for lname, ranges in lists]
    got = api.count_docset_ranges_batch(ix.searcher, [c[1] for c in cases], [counter(kind, c[4]) for c in cases])
    totals = {}
    for (sname, _, hits, lname, ranges), rc in zip(cases, got):
        exp = ix.expect(kind, hits, ranges)
        same(f"docset_{kind}_{sname}_{lname}", rc, exp)
        totals[sname] = exp[1:]
    assert totals["nothing"] == (0, 0) and all(totals[s][0] > 100 and 0 < totals[s][1] <= totals[s][0] for s in totals if s != "nothing")
    assert totals["all"][1] < totals["all"][0]   # some hit lacks a value
    assert totals["masks"][0] < totals["all"][0] and totals["range_both"][0] < totals["range_multi"][0] and totals["empty_words"][0] < totals["all"][0]
    assert api.count_docset_ranges_supported(ix.searcher, sets[4][1], counter(kind, lists[0][1])) is True


def test_the_doc_set_entry_runs_over_packed_postings():
    corpus = fs.make_corpus([1500, 70], {1: 0.5}, seed=13)
    rng = np.random.default_rng(14)
    c = api.GpuContext(device_id=0, max_batch=16, flags=_lib.NRTGPU_FLAG_PACKED_POSTINGS)
    leaves = []
    try:
        columns = {kind: [(None, rng.choice(np.array(ref.POOL[kind], dtype=ref.BITS_DTYPE[kind]), size=seg.max_doc)) for seg in corpus.segments]
                   for kind in ("int", "long")}
        for si, seg in enumerate(corpus.segments):
            g = api.GpuSegment(c, seg.max_doc, seg.doc_base)
            leaves.append(g)
            g.add_field_norms(0, seg.norms)
            g.add_terms(0, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
            for kind in columns:
                add_column(g, FIELD[kind], kind, columns[kind][si][1])
            g.seal()
        s = api.GpuIndexSearcher(c, leaves, api.IndexStatistics.from_corpus(corpus))
        for kind in columns:
            ranges = ref.range_lists(kind)[-1][1]
            got = api.count_docset_ranges_batch(s, [ALL], [counter(kind, ranges)])[0]
            same(f"packed_{kind}", got, ref.count(corpus, ref.docset_hits(corpus), columns[kind], kind, ranges))
            assert api.count_ranges_supported(s, T[1], counter(kind, ranges)) is False      # the text entry refuses the flag
            with pytest.raises(_lib.NrtGpuError) as e:
                api.count_ranges_batch(s, [T[1]], [counter(kind, ranges)])
            assert e.value.code == _lib.NRTGPU_ERR_UNSUPPORTED
    finally:
        release(leaves)
        c.close()


# ---- cross-checks that do not go through the new reference ---------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["int", "float"])
def test_range_counts_equal_the_sums_of_the_terms_routes_buckets(ix, kind):
    """total_hits and hits_with_value equal nrtgpu_count_terms_batch's; every range count equals the sum of that route's buckets
    whose value lies in the range (the order written out by _field_sort_ref.order_key)."""
    lists = ref.range_lists(kind)
    terms = api.count_terms_batch(ix.searcher, [q[1] for q in QUERIES], [api.TermsCollector(FIELD[kind], 10, True, kind)] * len(QUERIES), 1024)
    docset_terms = api.count_docset_terms_batch(ix.searcher, [ALL], [api.TermsCollector(FIELD[kind], 10, True, kind)], 1024)[0]
    checked = 0
    for lname, ranges in lists:
        got = api.count_ranges_batch(ix.searcher, [q[1] for q in QUERIES], [counter(kind, ranges)] * len(QUERIES))
        got.append(api.count_docset_ranges_batch(ix.searcher, [ALL], [counter(kind, ranges)])[0])
        for tc, rc in zip(terms + [docset_terms], got):
            assert not tc.overflowed and rc.total_hits == tc.total_hits and rc.hits_with_value == tc.hits_with_value
            keys = fs.order_key(kind, tc.value_bits)
            for (lo, hi), n in zip(ranges, rc.counts.tolist()):
                inside = (keys >= ref.order_int(kind, lo)) & (keys <= ref.order_int(kind, hi))
                assert n == int(tc.counts[inside].sum()), (kind, lname, hex(lo), hex(hi))
                checked += n > 0
    assert checked > 300


@pytest.mark.parametrize("kind", ["long", "double"])
def test_total_hits_over_a_64_bit_column_equal_the_terms_routes(ix, kind):
    """total_hits does not depend on the counted column: the terms route over the int column counts the same hits."""
    ranged = api.count_ranges_batch(ix.searcher, [q[1] for q in QUERIES], [counter(kind, ref.range_lists(kind)[0][1])] * len(QUERIES))
    terms = api.count_terms_batch(ix.searcher, [q[1] for q in QUERIES], [api.TermsCollector(FIELD["int"], 10)] * len(QUERIES), 1024)
    assert [c.total_hits for c in ranged] == [t.total_hits for t in terms] and sum(c.total_hits for c in ranged) > 5000
    docs = api.count_docset_ranges_batch(ix.searcher, [ALL], [counter(kind, ref.range_lists(kind)[0][1])])[0]
    assert docs.total_hits == api.count_docset_terms_batch(ix.searcher, [ALL], [api.TermsCollector(FIELD["int"], 10)], 1024)[0].total_hits


# ---- eight seeded fuzz rounds of mixed batches over both entries and all kinds --------------------------------------------------
@pytest.fixture(scope="module")
def fuzz_ix(ctx):
    corpus = ref.fuzz_corpus()
    columns = ref.fuzz_columns(corpus)
    leaves = []
    for si, seg in enumerate(corpus.segments):
        g = api.GpuSegment(ctx, seg.max_doc, seg.doc_base)
        g.add_field_norms(0, seg.norms)
        g.add_terms(0, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
        for kind in ref.KINDS:
            if columns[kind][si] is not None:
                add_column(g, ref.FUZZ_FIELD[kind], kind, columns[kind][si][1], columns[kind][si][0])
        g.seal()
        g.set_live_docs(seg.live_bits)
        leaves.append(g)
    yield corpus, columns, api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics.from_corpus(corpus))
    release(leaves)


@pytest.mark.parametrize("seed", range(ref.FUZZ_ROUNDS))
def test_fuzz_round(fuzz_ix, seed):
    """Every drawn request is run and asserted; none is skipped or refused (tests/test_range_count_host.py holds the rounds to
    their three shapes on the reference alone)."""
    corpus, columns, searcher = fuzz_ix
    ran = 0
    for entry, reqs in ref.fuzz_round(seed):
        counters = [api.RangeCounter(ref.FUZZ_FIELD[kind], kind, tuple(ranges)) for kind, _, ranges in reqs]
        if entry == "text":
            queries = []
            for _, (terms, need, must), _ in reqs:
                tq = tuple(api.TermQuery(0, t) for t in terms)
                queries.append(api.BooleanQuery((), 0, (), (), tq) if must else api.BooleanQuery(tq, need))
            got = api.count_ranges_batch(searcher, queries, counters)
        else:
            docsets = [ALL if spec is None else api.DocSetQuery(ranges=(api.RangeClause(ref.FUZZ_FIELD["int"], "int", fs.value_of("int", spec[0]),
                                                                                        fs.value_of("int", spec[1])),)) for _, spec, _ in reqs]
            got = api.count_docset_ranges_batch(searcher, docsets, counters)
        assert len(got) == len(reqs)
        for i, (req, rc) in enumerate(zip(reqs, got)):
            same(f"fuzz_{seed}_{entry}_{i}_{req[0]}", rc, ref.fuzz_expect(corpus, columns, entry, req))
            ran += 1
    assert ran >= 12


# ---- refusals that need a device -------------------------------------------------------------------------------------------------
def _raw(searcher, entry, query, c, tweak=None, predicate=True, mgr=None):
    """The entry's status for one query; the predicate must agree (it has no output to judge)."""
    L = _lib.load()
    rc, outs, counts, keep = api._marshal_range_counters([c])
    if tweak:
        tweak(rc, outs)
    if entry == "text":
        m = api._marshal_range_queries(searcher, [query], [c], None if mgr is None else [mgr])
        r = L.nrtgpu_count_ranges_batch(searcher.ctx._h, searcher._segs, searcher._bases, len(searcher.leaves), m.queries, rc, 1, outs)
        text = L.nrtgpu_last_error().decode()
        r2 = L.nrtgpu_count_ranges_supported(searcher.ctx._h, searcher._segs, len(searcher.leaves), m.queries, rc)
    else:
        ds, dkeep = api._marshal_docsets([query], [mgr or api.TopScoreDocCollectorManager(1)])
        r = L.nrtgpu_count_docset_ranges_batch(searcher.ctx._h, searcher._segs, searcher._bases, len(searcher.leaves), ds, rc, 1, outs)
        text = L.nrtgpu_last_error().decode()
        r2 = L.nrtgpu_count_docset_ranges_supported(searcher.ctx._h, searcher._segs, len(searcher.leaves), ds, rc)
    if predicate:
        assert r2 == r, f"the predicate ({r2}) and the call ({r}) disagree: {text}"
    return r, text


def test_refusals(ix):
    s = ix.searcher
    inv, uns = _lib.NRTGPU_ERR_INVALID_ARG, _lib.NRTGPU_ERR_UNSUPPORTED
    or3 = QUERIES[1][1]
    R = ref.range_lists("long")[0][1]
    ok = counter("long", R)

    def n_ranges(v):
        return lambda rc, outs: setattr(rc[0], "n_ranges", v)

    def null_ranges(rc, outs):
        rc[0].ranges = C.POINTER(_lib.ValueRange)()

    def null_counts(rc, outs):
        outs[0].counts = C.POINTER(C.c_int64)()

    for entry, q, unresident in (("text", or3, api.BooleanQuery((T[1],), 1, (api.MaskFilter(77),))), ("docset", ALL, api.DocSetQuery((), (api.MaskFilter(78),)))):
        refusals = [
            ("n_ranges 0", inv, q, ok, dict(tweak=n_ranges(0))),
            ("n_ranges 65", inv, q, ok, dict(tweak=n_ranges(65))),
            ("ranges NULL", inv, q, ok, dict(tweak=null_ranges)),
            ("a high word over a 32-bit column", inv, q, counter("int", [(3, 2**32 + 9)]), {}),
            ("capacity below n_ranges", inv, q, ok, dict(tweak=lambda rc, outs: setattr(outs[0], "capacity", 2), predicate=False)),
            ("counts NULL", inv, q, ok, dict(tweak=null_counts, predicate=False)),
            ("reserved 1", inv, q, ok, dict(tweak=lambda rc, outs: setattr(outs[0], "reserved", 1), predicate=False)),
            ("numHits 0", inv, q, ok, dict(mgr=api.TopScoreDocCollectorManager(0))),
            ("n_ranges 0 over no column", inv, q, counter("long", R, 55), dict(tweak=n_ranges(0))),
            ("no column on any leaf", uns, q, counter("long", R, 55), {}),
            ("a multi-valued count column", uns, q, counter("int", [(3, 9)], MCOL), {}),
            ("a mask that is not resident", uns, unresident, ok, {}),
        ]
        if entry == "text":
            refusals += [
                ("dismax", uns, api.DisjunctionMaxQuery((T[1], T[2])), ok, {}),
                ("MUST next to SHOULD", uns, api.BooleanQuery((T[2],), 0, (), (), (T[1],)), ok, {}),
                ("min_competitive_score", uns, or3, ok, dict(mgr=api.TopScoreDocCollectorManager(10, None, 1000, 0.5))),
                ("numHits 2000", uns, or3, ok, dict(mgr=api.TopScoreDocCollectorManager(2000))),
            ]
        else:
            refusals.append(("a range clause over a 64-bit column", uns, api.DocSetQuery(ranges=(api.RangeClause(FIELD["long"], "int", 0, 5),)), ok, {}))
        for name, code, query, c, kw in refusals:
            r, text = _raw(s, entry, query, c, **kw)
            assert r == code, f"{entry}: {name}: status {r}: {text}"
            assert "query 0" in text, f"{entry}: {name}: {text}"
        # a batch that mixes widths; an invalid argument in query 1 before an unsupported query 0
        call = api.count_ranges_batch if entry == "text" else api.count_docset_ranges_batch
        with pytest.raises(_lib.NrtGpuError) as e:
            call(s, [q, q], [ok, counter("int", [(3, 9)])])
        assert e.value.code == uns and "split" in str(e.value) and "query 1" in str(e.value)
        with pytest.raises(_lib.NrtGpuError) as e:
            call(s, [q, q], [counter("long", R, 55), counter("int", [(3, 2**32 + 9)])])
        assert e.value.code == inv and "query 1" in str(e.value)
        same(f"after_refusals_{entry}", call(s, [q], [ok])[0], ix.expect("long", ix.text_hits((1, 2, 3), 1, False) if entry == "text" else ref.docset_hits(ix.corpus), R))
    # the fixed-point analysis of the final-score routes, the known limit it is on the terms route
    wide = api.BooleanQuery((T[1], api.BoostQuery(T[2], 2.0 ** -20)))
    r, text = _raw(s, "text", wide, ok)
    assert r == uns and "fixed-point" in text
    # NULL arguments with a context
    q0, r0, o0, d0 = _lib.Bm25Query(), _lib.RangeCount(), _lib.RangeCounts(), _lib.DocsetQuery()
    L = _lib.load()
    assert L.nrtgpu_count_ranges_batch(s.ctx._h, s._segs, s._bases, 3, None, C.byref(r0), 1, C.byref(o0)) == inv
    assert L.nrtgpu_count_ranges_batch(s.ctx._h, s._segs, s._bases, 3, C.byref(q0), C.byref(r0), 1, None) == inv
    assert L.nrtgpu_count_docset_ranges_batch(s.ctx._h, s._segs, s._bases, 3, C.byref(d0), None, 1, C.byref(o0)) == inv
    assert L.nrtgpu_count_docset_ranges_supported(s.ctx._h, s._segs, 3, None, C.byref(r0)) == inv


def test_leaves_that_disagree_on_the_kind(ctx, ix):
    leaves = []
    try:
        for seg, kind in zip(ix.corpus.segments, ("long", "double", "long")):
            g = api.GpuSegment(ctx, seg.max_doc, seg.doc_base)
            leaves.append(g)
            g.add_field_norms(0, seg.norms)
            g.add_terms(0, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
            g.add_doc_values64(7, kind, np.zeros(seg.max_doc, dtype=np.uint64))
            g.seal()
        s = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics.from_corpus(ix.corpus))
        for entry, q in (("text", T[1]), ("docset", ALL)):
            r, text = _raw(s, entry, q, counter("long", [(0, 5)], 7))
            assert r == _lib.NRTGPU_ERR_INVALID_ARG and "kinds" in text and "query 0" in text
    finally:
        release(leaves)


@pytest.mark.parametrize("flag", [_lib.NRTGPU_FLAG_PACKED_POSTINGS, _lib.NRTGPU_FLAG_NO_FIXED_POINT])
def test_contexts_the_text_entry_refuses(flag):
    corpus = fs.make_corpus([200], {1: 0.5}, seed=13)
    c = api.GpuContext(device_id=0, max_batch=16, flags=flag)
    leaves = []
    try:
        bits = np.arange(200, dtype=np.uint32)
        leaves = fs.upload(c, corpus, "int", [(None, bits)], column_field=7)
        s = api.GpuIndexSearcher(c, leaves, api.IndexStatistics.from_corpus(corpus))
        r, text = _raw(s, "text", T[1], counter("int", [(3, 90)], 7))
        assert r == _lib.NRTGPU_ERR_UNSUPPORTED and "NRTGPU_FLAG" in text
        r, text = _raw(s, "docset", ALL, counter("int", [(3, 90)], 7))
        assert r == 0, text
        got = api.count_docset_ranges_batch(s, [ALL], [counter("int", [(3, 90)], 7)])[0]
        same("flagged_docset", got, ref.count(corpus, ref.docset_hits(corpus), [(None, bits)], "int", [(3, 90)]))
    finally:
        release(leaves)
        c.close()
