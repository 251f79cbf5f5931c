"""The MaxScore walk's HALF GROUPS (csrc/maxscore.hip: walk_units): a window's essential clauses are streamed as one sequence of
8-posting units, 64 units per instruction; when 32 units or fewer are left the window's last instruction runs the walk's body at
FOUR postings per lane (lane l: half l & 1 of unit v0 + (l >> 1)).  Checked here, against the oracle's exhaustive scorer (docids,
score bits, totalHits, relation): leaves of 131 072 and 70 000 docs (two full windows; a full one and a short last one) built by
hand so that a window's last instruction holds 1, 31, 32, 33 and 64 units (33 and 64: the full body), a window whose only
instruction is a half one, a clause boundary inside a half instruction with a doc in both clauses, clauses that begin at every
position of a 16-byte word and in an odd half of a unit, a sparse clause whose cell is coarser than the window, postings no score
table serves and postings of deleted docs, a candidate-buffer overflow called from the half body, the packed layout, and one
query of every shape.  NRTGPU_MS_HALF_GROUPS=0 (development library) is the walk without half groups: the same arrays.

How the sizes are known: walk_model() restates, from the postings, what the kernel streams in a window -- per clause the range
its cell table gives, counted in 8-posting units from the range's 16-byte aligned begin.  Every clause of a window is streamed
as long as the last (densest, lightest) clause alone can still reach the k-th best score: each leaf holds one PLANTED posting of
that clause -- the highest freq a table serves in a doc of length 1, every other doc being long -- that no k docs beat
(planted_bound; the sized fixture checks it against the oracle's k-th score).
Needs a real MI355X."""
import numpy as np
import pytest

from nrtsearch_amd import _lib, api, synth
from tests.test_walk_rows_gpu import Index, bq, check, same_arrays, segment

pytestmark = pytest.mark.gpu
WIN_TILES, TILE = 64, 1024          # csrc/plan.h: kMsWinTiles, kTileDocs
CELL_POSTINGS = 4                   # csrc/segment.cpp: kCellPostings
TERMS = [1, 2, 3, 4, 5]             # sparsest (heaviest) first: the walk's clause order; 5 is the last clause
K, THR = 10, 100
ONE_SLICE = (10_000_000, 1000)
AVGDL = 400


def cell_shift(count, n_tiles):
    budget, shift = max(1, count // CELL_POSTINGS), 0
    while ((n_tiles - 1) >> shift) + 1 > budget:
        shift += 1
    return shift


def walk_model(max_doc, postings):
    """postings: {term: ascending docids}, laid out in the columns in term-id order from an aligned base.  Per window: the clauses
    in walk order as (term, begin, count, units), begin = the absolute index of the clause's first posting of the window."""
    n_tiles = (max_doc + TILE - 1) // TILE
    ids = sorted(postings)
    start = dict(zip(ids, np.concatenate([[0], np.cumsum([len(postings[t]) for t in ids])]).tolist()))
    order = sorted(ids, key=lambda t: (len(postings[t]), t))
    assert len({len(postings[t]) for t in ids}) == len(ids), "clause order: the doc freqs must differ"
    wins = []
    for t0 in range(0, n_tiles, WIN_TILES):
        t1 = min(t0 + WIN_TILES, n_tiles)
        cl = []
        for t in order:
            d = postings[t]
            sh = cell_shift(len(d), n_tiles)
            lo = int(np.searchsorted(d, ((t0 >> sh) << sh) * TILE))
            hi = int(np.searchsorted(d, ((((t1 - 1) >> sh) + 1) << sh) * TILE))
            begin = start[t] + lo
            cl.append((t, begin, hi - lo, (hi - lo + (begin & 3) + 7) // 8 if hi > lo else 0, sh))
        wins.append(cl)
    return wins


def last_units(win):
    total = sum(c[3] for c in win)
    return 64 if total and total % 64 == 0 else total % 64


class Leaf:
    """One leaf of five terms.  base[t] = postings per FULL window of term t (scaled for a short window); tune = [(term, window,
    wanted size of the window's last instruction)], applied in order; both = the planted doc sits in clauses 4 AND 5, at the
    end of window `both`, where clause 5 has few postings: the boundary between the two lies inside the last instruction."""

    def __init__(self, max_doc, seed, base, tune, both=None, deleted=0.03):
        rng = np.random.Generator(np.random.PCG64(seed))
        self.max_doc = max_doc
        n_wins = (max_doc + WIN_TILES * TILE - 1) // (WIN_TILES * TILE)
        spans = [(w * WIN_TILES * TILE, min((w + 1) * WIN_TILES * TILE, max_doc)) for w in range(n_wins)]
        plant_win = both if both is not None else 0
        self.planted = spans[plant_win][1] - 1   # (the window's last doc: the last posting of its clauses there)
        perms = {t: [lo + rng.permutation(hi - lo) for lo, hi in spans] for t in TERMS}
        for t in ([4, 5] if both is not None else [5]):   # the planted doc is in every prefix of its permutation
            p = perms[t][plant_win]
            i = int(np.nonzero(p == self.planted)[0][0])
            p[0], p[i] = p[i], p[0]
        counts = {t: [max(1, base[t] * (hi - lo) // (WIN_TILES * TILE)) for lo, hi in spans] for t in TERMS}
        if 1 in base and base[1] * n_wins < 2 * CELL_POSTINGS:   # (the sparse clause: a handful of postings in the whole leaf)
            counts[1] = [base[1]] * n_wins
        if both is not None:
            counts[5][both] = 100
        make = lambda: {t: np.concatenate([np.sort(perms[t][w][:counts[t][w]]) for w in range(n_wins)]) for t in TERMS}
        for _ in range(8):   # (a count moves the begin of everything behind it in the columns: again until every size holds)
            if all(last_units(walk_model(max_doc, make())[w]) == want for _, w, want in tune):
                break
            for term, w, want in tune:
                first = counts[term][w]
                for n in range(first, first + 64 * 8 + 8):
                    counts[term][w] = n
                    if last_units(walk_model(max_doc, make())[w]) == want:
                        break
                else:
                    raise AssertionError(f"no count of term {term} gives window {w} a last instruction of {want} units")
        self.docids = make()
        self.model = walk_model(max_doc, self.docids)
        for term, w, want in tune:
            assert last_units(self.model[w]) == want, (term, w, want, self.model[w])
        # docs: long ones (75 x the average length the corpus statistics state -- AVGDL; a longer one and the clause's scores span
        # more binades than the fixed-point sums of the MaxScore route take), 2 % just long enough for a norm byte that leaves the
        # score tables; the planted doc has length 1
        lengths = np.where(rng.random(max_doc) < 0.02, 36_000, 30_000)
        lengths[self.planted] = 1
        self.norms = synth.int_to_byte4(lengths)
        assert (self.norms >= 128).any()
        self.freqs = {}
        for t in TERMS:
            n = len(self.docids[t])
            f = np.where(rng.random(n) < 0.05, rng.integers(13, 21, n), rng.integers(1, 13, n))   # 5 %: freqs no table serves
            if t == 5 or (t == 4 and both is not None):
                f[np.searchsorted(self.docids[t], self.planted)] = 12
            self.freqs[t] = f
        dead = rng.random(max_doc) < deleted
        dead[self.planted] = False
        live = np.zeros((max_doc + 63) // 64 * 64, dtype=bool)
        live[:max_doc] = ~dead
        self.live_bits = np.packbits(live.reshape(-1, 64), axis=1, bitorder="little").view(np.uint64).reshape(-1).copy() if deleted else None

    def segment(self, doc_base=0):
        return segment(self.max_doc, doc_base, self.norms, {t: (self.docids[t], self.freqs[t]) for t in TERMS}, self.live_bits)


def corpus_of(leaves):
    segs, base = [], 0
    for l in leaves:
        segs.append(l.segment(base))
        base += l.max_doc
    return synth.Corpus(n_docs=base, doc_count=base, sum_total_term_freq=AVGDL * base, segments=segs,
                        doc_freq={t: int(sum(len(l.docids[t]) for l in leaves)) for t in TERMS})


BASE = {1: 3, 2: 300, 3: 700, 4: 1500, 5: 3000}   # term 1: 6 postings in the leaf -- ONE cell, coarser than a window
LEAVES = {   # name: (max_doc, seed, tune, both)
    "1_and_31": (131_072, 1, [(5, 0, 1), (5, 1, 31)], None),
    "32_and_33": (131_072, 2, [(5, 0, 32), (5, 1, 33)], None),
    "64_and_32": (131_072, 3, [(5, 0, 64), (5, 1, 32)], None),
    "33_and_short_1": (70_000, 4, [(5, 0, 33), (5, 1, 1)], None),
    "31_and_short_64": (70_000, 5, [(5, 0, 31), (5, 1, 64)], None),
    "boundary_in_a_half": (131_072, 6, [(5, 0, 32), (4, 1, 31)], 1),
    "boundary_in_a_short_half": (70_000, 7, [(5, 0, 1), (4, 1, 20)], 1),
}
QUERIES = [TERMS, [5, 4], [5, 3, 1], [4, 5, 2]]


@pytest.fixture(scope="module")
def leaves():
    return {name: Leaf(m, seed, BASE, tune, both) for name, (m, seed, tune, both) in LEAVES.items()}


def planted_bound(corpus):
    """(a little below) what clause 5 adds to the planted doc: freq 12, length 1"""
    n, df = corpus.doc_count, corpus.doc_freq[5]
    return 0.95 * np.log(1 + (n - df + 0.5) / (df + 0.5)) * 12 / (12 + 1.2 * 0.25)


@pytest.fixture(scope="module")
def sized(oracle, leaves):
    """One corpus per leaf; the oracle's answers to QUERIES, computed once."""
    out = {}
    for name, leaf in leaves.items():
        corpus = corpus_of([leaf])
        out[name] = (corpus, [oracle.search_bm25(corpus, q, K, total_hits_threshold=THR) for q in QUERIES])
        for docs, scores, _, gte in out[name][1]:   # clause 5 alone reaches the k-th score to the end: no clause ever leaves the stream
            assert docs[0] == leaf.planted and scores[K - 1] < planted_bound(corpus) and gte, (name, scores)
    return out


def test_the_leaves_have_the_shapes_they_are_meant_to_have(leaves):
    """(no search: the model's account of what the five-clause query streams in every window)"""
    sizes, begins, odd_half, coarse, boundary = set(), set(), False, False, 0
    for name, leaf in leaves.items():
        n_tiles = (leaf.max_doc + TILE - 1) // TILE
        for w, win in enumerate(leaf.model):
            last = last_units(win)
            sizes.add(last)
            for t, begin, count, units, sh in win:
                if count:
                    begins.add(begin & 3)
                    odd_half |= ((begin >> 2) & 1) == 1
                    coarse |= (1 << sh) > WIN_TILES and n_tiles > WIN_TILES and count > 0
            if LEAVES[name][3] == w:   # clause 5's units are fewer than the last instruction's: clause 4's last unit is in it too
                assert win[-1][0] == 5 and win[-2][0] == 4 and 0 < win[-1][3] < last <= 32, (name, win)
                assert leaf.planted == leaf.docids[4][-1] == leaf.docids[5][-1]
                boundary += 1
    assert sizes >= {1, 31, 32, 33, 64}, sizes
    assert begins == {0, 1, 2, 3} and odd_half and coarse and boundary == 2, (begins, odd_half, coarse, boundary)
    # (a window whose ONLY instruction is a half one: every window of the tiny_windows fixture)


def run_sized(ctx, sized):
    out = {}
    for name, (corpus, _) in sized.items():
        ix = Index(ctx, corpus)
        try:
            mgr = api.TopScoreDocCollectorManager(K, None, THR)
            out[name] = ix.searcher.search_batch([bq(q) for q in QUERIES], [mgr] * len(QUERIES))
        finally:
            ix.close()
    return out


@pytest.mark.parametrize("layout", ["two_columns", "packed", "deletes_as_a_mask"])
def test_last_instructions_of_every_size(layout, sized, leaves):
    flags = {"two_columns": 0, "packed": _lib.NRTGPU_FLAG_PACKED_POSTINGS, "deletes_as_a_mask": _lib.NRTGPU_FLAG_NO_LIVE_FOLD}[layout]
    ctx = api.GpuContext(device_id=0, max_batch=16, flags=flags)
    try:
        ctx.reset_stats()
        got = run_sized(ctx, sized)
        assert ctx.stats()["maxscore_items"] > 0
        for name, res in got.items():
            for i, r in enumerate(res):
                check(f"{layout}_{name}_{i}", r, sized[name][1][i], K, THR)
                # the planted doc is the best hit, once (a doc in two clauses of one instruction is evaluated once)
                assert r.docs[0] == leaves[name].planted and len(set(r.docs.tolist())) == len(r.docs), f"{layout}_{name}_{i}: {r.docs[:3]}"
    finally:
        ctx.close()


# ---- a window whose only instruction is a half one; an overflow of the candidate buffer called from the half body ------------------
@pytest.fixture(scope="module")
def tiny_windows(oracle):
    """Eight leaves of 131 072 docs in one searcher slice (one work item of 16 windows), a dense clause pair of 2 x ~100 postings
    per window: EVERY instruction of the walk is a half one (<= 32 units).  k = 1000: until the first meeting every evaluated
    doc is a candidate, and the item evaluates more docs than the buffer holds -- the meeting is called from the half body."""
    leaves = [Leaf(131_072, 20 + i, {1: 3, 2: 5, 3: 9, 4: 90, 5: 105}, [], None) for i in range(8)]
    for l in leaves:
        for win in l.model:
            assert 0 < sum(c[3] for c in win) <= 32, win
    corpus = corpus_of(leaves)
    assert sum(len(l.docids[5]) for l in leaves) > 1000 and sum(len(np.union1d(l.docids[4], l.docids[5])) for l in leaves) > 2304 + 512
    queries = [[4, 5], TERMS]
    return corpus, queries, [oracle.search_bm25(corpus, q, 1000, total_hits_threshold=1000, slicing=ONE_SLICE) for q in queries]


def run_tiny(ctx, tiny_windows):
    corpus, queries, _ = tiny_windows
    ctx.set_slicing(*ONE_SLICE)
    ix = Index(ctx, corpus)
    try:
        mgr = api.TopScoreDocCollectorManager(1000, None, 1000)
        return ix.searcher.search_batch([bq(q) for q in queries], [mgr] * len(queries))
    finally:
        ix.close()
        ctx.set_slicing()


@pytest.mark.parametrize("packed", [False, True], ids=["two_columns", "packed"])
def test_only_half_instructions_and_an_overflow_among_them(packed, tiny_windows):
    ctx = api.GpuContext(device_id=0, max_batch=16, flags=_lib.NRTGPU_FLAG_PACKED_POSTINGS if packed else 0)
    try:
        ctx.reset_stats()
        got = run_tiny(ctx, tiny_windows)
        assert ctx.stats()["maxscore_items"] == len(got), "a query of this index is one work item"
        for i, r in enumerate(got):
            check(f"tiny_{packed}_{i}", r, tiny_windows[2][i], 1000, 1000)
    finally:
        ctx.close()


# ---- one query of every shape ----------------------------------------------------------------------------------------------------
SHAPE_LEAVES = ["32_and_33", "31_and_short_64"]


@pytest.fixture(scope="module")
def shaped(oracle, leaves):
    out = {}
    for name in SHAPE_LEAVES:
        corpus = corpus_of([leaves[name]])
        mask = synth.random_mask(corpus.segments[0].max_doc, 0.4, 900)
        tq = tuple(api.TermQuery(0, t) for t in TERMS)
        o = lambda **kw: oracle.search_bm25(corpus, TERMS, K, total_hits_threshold=THR, **kw)
        out[name] = (corpus, mask, [
            ("msm2", api.BooleanQuery(tq, 2), o(min_should_match=2)),
            ("filter", api.BooleanQuery(tq, 1, (api.MaskFilter(3),)), o(accept=[synth.accept_words(corpus.segments[0], mask, None)])),
            ("dismax_0", api.DisjunctionMaxQuery(tq, 0.0), o(dismax=0.0)),
            ("dismax_0.3", api.DisjunctionMaxQuery(tq, 0.3), o(dismax=0.3)),
            ("must_should", api.BooleanQuery(tq[1:], must=tq[:1]), o(must=[True, False, False, False, False])),
            ("must_dense", api.BooleanQuery(tq[:4], must=tq[4:]), oracle.search_bm25(corpus, [5, 1, 2, 3, 4], K, total_hits_threshold=THR, must=[True, False, False, False, False])),
        ])
    return out


def run_shaped(ctx, shaped):
    out = {}
    for name, (corpus, mask, cases) in shaped.items():
        ix = Index(ctx, corpus)
        try:
            ix.leaves[0].set_mask(3, mask)
            mgr = api.TopScoreDocCollectorManager(K, None, THR)
            out[name] = (ix.searcher.search_batch([c[1] for c in cases], [mgr] * len(cases)), [ix.searcher.search(c[1], mgr) for c in cases])
        finally:
            ix.close()
    return out


@pytest.mark.parametrize("packed", [False, True], ids=["two_columns", "packed"])
def test_query_shapes(packed, shaped):
    ctx = api.GpuContext(device_id=0, max_batch=16, flags=_lib.NRTGPU_FLAG_PACKED_POSTINGS if packed else 0)
    try:
        ctx.reset_stats()
        got = run_shaped(ctx, shaped)
        assert ctx.stats()["maxscore_items"] > 0
        for name, (together, alone) in got.items():
            for (shape, _, exp), a, b in zip(shaped[name][2], together, alone):
                check(f"{packed}_{name}_{shape}_batch", a, exp, K, THR)
                check(f"{packed}_{name}_{shape}_alone", b, exp, K, THR)
    finally:
        ctx.close()


# ---- A/B: the walk without half groups returns the same arrays ---------------------------------------------------------------------
def both_walks(monkeypatch, run):
    out = []
    for half in ("1", "0"):
        monkeypatch.setenv("NRTGPU_MS_HALF_GROUPS", half)
        out.append(run())
    return out


@pytest.mark.parametrize("packed", [False, True], ids=["two_columns", "packed"])
def test_ab_the_same_arrays_without_half_groups(dev_lib, monkeypatch, sized, tiny_windows, shaped, packed):
    ctx = api.GpuContext(device_id=0, max_batch=16, flags=_lib.NRTGPU_FLAG_PACKED_POSTINGS if packed else 0)
    try:
        a, b = both_walks(monkeypatch, lambda: run_sized(ctx, sized))
        for name in a:
            for i, (x, y) in enumerate(zip(a[name], b[name])):
                same_arrays(f"ab_{name}_{i}", x, y)
                check(f"ab_{name}_{i}", y, sized[name][1][i], K, THR)
        a, b = both_walks(monkeypatch, lambda: run_tiny(ctx, tiny_windows))
        for i, (x, y) in enumerate(zip(a, b)):
            same_arrays(f"ab_tiny_{i}", x, y)
        a, b = both_walks(monkeypatch, lambda: run_shaped(ctx, shaped))
        for name in a:
            for part_a, part_b in zip(a[name], b[name]):
                for i, (x, y) in enumerate(zip(part_a, part_b)):
                    same_arrays(f"ab_{name}_{shaped[name][2][i][0]}", x, y)
    finally:
        ctx.close()
