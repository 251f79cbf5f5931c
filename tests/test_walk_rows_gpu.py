"""The MaxScore route's WALK ROWS (csrc/plan.h: DWalkRow): the plan expansion works out, once per (query, leaf), what every wave
that enters a segment used to work out for itself -- each clause's exact maximum score in the leaf, the suffix sums (maxima for a
DisjunctionMaxQuery) and the clause's record -- and the walk copies them.  Checked here: the rows themselves against a brute-force
restatement over ALL postings (development library: nrtgpu_debug_walk_rows / nrtgpu_debug_walk_value), and the searches that read
them -- leaves that hold different subsets of a query's terms, items of many parts (both ways of finding a window's part, both
window orders, fine windows, helpers), the query shapes -- against the oracle's exhaustive scorer: docids, score bits, totalHits,
relation.  NRTGPU_MS_WALK_ROWS=0 (development library) is the walk that computes the bounds itself: the same arrays.
Needs a real MI355X."""
import numpy as np
import pytest

from nrtsearch_amd import _lib, api, synth

pytestmark = pytest.mark.gpu
INT_MAX = 2**31 - 1


def check(name, got, exp, k, thr):
    edocs, escores, etotal, egte = exp
    assert got.docs.tolist() == edocs.tolist(), f"{name}: docids/ranks differ"
    assert got.scores.view(np.uint32).tolist() == escores.view(np.uint32).tolist(), f"{name}: score bits differ"
    assert got.relation_gte == egte, f"{name}: relation"
    if egte:
        assert max(thr, k) < got.total_hits <= etotal, f"{name}: lower bound {got.total_hits} not in ({max(thr, k)}, {etotal}]"
    else:
        assert got.total_hits == etotal, f"{name}: totalHits {got.total_hits} != {etotal}"


def same_arrays(name, a, b):
    assert a.docs.tolist() == b.docs.tolist() and a.scores.view(np.uint32).tolist() == b.scores.view(np.uint32).tolist(), f"{name}: hits differ"
    assert a.relation_gte == b.relation_gte and (a.relation_gte or a.total_hits == b.total_hits), f"{name}: relation / exact count differ"


def bq(terms, boosts=None):
    cl = [api.TermQuery(0, int(t)) if boosts is None else api.BoostQuery(api.TermQuery(0, int(t)), float(boosts[i])) for i, t in enumerate(terms)]
    return cl[0] if len(cl) == 1 else api.BooleanQuery(tuple(cl))


def segment(max_doc, doc_base, norms, postings, live_bits=None):
    """postings: {term id: (ascending docids, freqs)}"""
    ids = sorted(postings)
    counts = [len(postings[t][0]) for t in ids]
    cat = lambda i: np.concatenate([np.asarray(postings[t][i], dtype=np.int32) for t in ids]) if ids else np.zeros(0, np.int32)
    return synth.SegmentData(max_doc=int(max_doc), doc_base=int(doc_base), norms=np.ascontiguousarray(norms, dtype=np.uint8),
                             term_ids=np.asarray(ids, dtype=np.int64), offsets=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64),
                             docids=np.ascontiguousarray(cat(0)), freqs=np.ascontiguousarray(cat(1)), live_bits=live_bits)


def recut(corpus, leaf_docs, keep=None):
    """The same index cut into leaves of leaf_docs docs (a multiple of 64: liveDocs words are not split); keep(leaf, term) == False
    drops a term's postings from a leaf.  Index-global statistics follow the postings that are left."""
    assert len(corpus.segments) == 1 and leaf_docs % 64 == 0
    src = corpus.segments[0]
    segs, df = [], {int(t): 0 for t in src.term_ids}
    for li, base in enumerate(range(0, src.max_doc, leaf_docs)):
        size = min(leaf_docs, src.max_doc - base)
        post = {}
        for t in src.term_ids:
            d, f = src.postings(int(t))
            lo, hi = np.searchsorted(d, [base, base + size])
            if hi > lo and (keep is None or keep(li, int(t))):
                post[int(t)] = (d[lo:hi] - base, f[lo:hi])
                df[int(t)] += int(hi - lo)
        live = None if src.live_bits is None else src.live_bits[base // 64: (base + size + 63) // 64].copy()
        segs.append(segment(size, base, src.norms[base: base + size], post, live))
    return synth.Corpus(n_docs=corpus.n_docs, doc_count=corpus.doc_count, sum_total_term_freq=corpus.sum_total_term_freq, segments=segs,
                        doc_freq={t: n for t, n in df.items() if n > 0})


class Index:
    def __init__(self, ctx, corpus):
        self.corpus = corpus
        self.leaves = [api.GpuSegment.from_data(ctx, s) for s in corpus.segments]
        self.searcher = api.GpuIndexSearcher(ctx, self.leaves, api.IndexStatistics.from_corpus(corpus))

    def close(self):
        for l in self.leaves:
            l.release()


# ---- 1. the rows ----------------------------------------------------------------------------------------------------------------
# Three leaves of 8192 docs, two fields.  Field 0: term 1 occurs only with freq > 12 (no posting a score table can serve: the
# frontier is the escape entry alone), term 2 only in docs whose norm byte is >= 128 (the same, by the norm), term 3 with both
# kinds of posting, terms 4 and 5 ordinary (5 is rare: a heavy clause, so that the clauses' fixed-point scales differ).  Field 1:
# term 7 over short docs with small freqs (every posting served by a score table).  Leaf 1 lacks term 5.
# What the seal keeps of a term's postings that no score table serves is ONE pair -- their largest freq and their smallest norm byte
# (plan.h: DTermAux.esc_*) -- so the clause's bound is the score of that pair: the term's exact maximum where one posting has both,
# a bound above it otherwise.  Terms 1 - 3 get such a posting planted in every leaf (the equality below is then exact); term 6 is
# term 1's twin without one: its row must hold the pair's score, at or above every posting's.
ROW_LEAF = 8192
PLANTED = (1, 2, 3)


def rows_index():
    rng = np.random.Generator(np.random.PCG64(77))
    n = 3 * ROW_LEAF
    len0 = np.where(rng.random(n) < 0.2, rng.integers(20_000, 400_000, n), rng.integers(3, 300, n))
    len1 = rng.integers(1, 60, n)
    nb0, nb1 = synth.int_to_byte4(len0), synth.int_to_byte4(len1)
    assert (nb0 >= 128).any() and (nb0 < 128).any() and (nb1 < 128).all()

    def draw(p, freq_lo, freq_hi, only=None):
        sel = rng.random(n) < p
        if only is not None:
            sel &= only
        d = np.nonzero(sel)[0]
        return d, rng.integers(freq_lo, freq_hi + 1, len(d))

    field0 = {1: draw(0.05, 13, 60), 2: draw(0.3, 1, 9, nb0 >= 128), 3: draw(0.2, 1, 30), 4: draw(0.4, 1, 5), 5: draw(0.003, 1, 4),
              6: draw(0.05, 13, 60)}
    field1 = {7: draw(0.1, 1, 10)}
    leaves = []
    for li in range(3):
        base = li * ROW_LEAF
        cut = lambda post, drop=(): {t: (d[(d >= base) & (d < base + ROW_LEAF)] - base, f[(d >= base) & (d < base + ROW_LEAF)])
                                     for t, (d, f) in post.items() if t not in drop}
        leaves.append((cut(field0, drop=(5,) if li == 1 else ()), cut(field1)))
        for t in PLANTED:   # the posting with the smallest norm byte among those no table serves gets the largest freq among them
            d, f = leaves[li][0][t]
            nb = nb0[base + d]
            esc = np.nonzero((f > 12) | (nb >= 128))[0]
            f[esc[np.argmin(nb[esc])]] = f[esc].max() + 1
    stats = api.IndexStatistics()
    stats.fields[0] = api.CollectionStatistics(n, int(len0.sum()))
    stats.fields[1] = api.CollectionStatistics(n, int(len1.sum()))
    for f, post in ((0, field0), (1, field1)):
        for t in post:
            stats.doc_freq[(f, t)] = int(sum(len(l[f][t][0]) for l in leaves if t in l[f]))
    return leaves, (nb0, nb1), stats


def test_rows_hold_the_exact_bounds_of_every_clause(dev_lib):
    leaves, norms, stats = rows_index()
    ctx = api.GpuContext(device_id=0, max_batch=16)
    segs = []
    try:
        for li, (p0, p1) in enumerate(leaves):
            g = api.GpuSegment(ctx, ROW_LEAF, li * ROW_LEAF)
            for f, post in ((0, p0), (1, p1)):
                sd = segment(ROW_LEAF, li * ROW_LEAF, norms[f][li * ROW_LEAF: (li + 1) * ROW_LEAF], post)
                g.add_field_norms(f, sd.norms)
                g.add_terms(f, sd.term_ids, sd.offsets, sd.docids, sd.freqs)
            g.seal()
            segs.append(g)
        sr = api.GpuIndexSearcher(ctx, segs, stats)
        T = lambda f, t, boost=None: api.TermQuery(f, t) if boost is None else api.BoostQuery(api.TermQuery(f, t), boost)
        cases = [   # (name, query, its clauses as (field, term, boost) in query order, suffix MAXIMA?)
            ("sum", api.BooleanQuery((T(0, 1), T(0, 2), T(0, 3), T(0, 4), T(0, 5))), [(0, 1, 1), (0, 2, 1), (0, 3, 1), (0, 4, 1), (0, 5, 1)], False),
            ("no_posting_has_both", api.BooleanQuery((T(0, 6), T(0, 4), T(0, 3))), [(0, 6, 1), (0, 4, 1), (0, 3, 1)], False),
            ("boosted", api.BooleanQuery((T(0, 3), T(0, 4, 7.5), T(0, 1, 0.25))), [(0, 3, 1), (0, 4, 7.5), (0, 1, 0.25)], False),
            ("two_fields", api.BooleanQuery((T(1, 7), T(0, 3), T(0, 5), T(0, 2))), [(1, 7, 1), (0, 3, 1), (0, 5, 1), (0, 2, 1)], False),
            ("dismax", api.DisjunctionMaxQuery((T(0, 1), T(0, 3), T(1, 7), T(0, 5)), 0.0), [(0, 1, 1), (0, 3, 1), (1, 7, 1), (0, 5, 1)], True),
            ("dismax_tie", api.DisjunctionMaxQuery((T(0, 1), T(0, 3), T(0, 4)), 0.3), [(0, 1, 1), (0, 3, 1), (0, 4, 1)], False),
            ("one_clause", T(0, 2), [(0, 2, 1)], False),
        ]
        mgr = api.TopScoreDocCollectorManager(10, None, 100)
        begin, count, rows = sr.debug_walk_rows([c[1] for c in cases], [mgr] * len(cases))
        sim = api.BM25Similarity()
        seen = set()
        for qi, (name, _, clauses, use_max) in enumerate(cases):
            fields = []
            for f, _, _ in clauses:
                if f not in fields:
                    fields.append(f)
            for li in range(3):
                here = [(ci, f, t, b) for ci, (f, t, b) in enumerate(clauses) if t in leaves[li][f]]
                assert count[qi, li] == len(here) and begin[qi, li] >= 0, f"{name}, leaf {li}: rows {count[qi, li]} at {begin[qi, li]}"
                weight = lambda f, t, b: np.float32(np.float32(b) * sim.idf(stats.doc_freq[(f, t)], stats.fields[f].doc_count))
                # the walk's clause order: heaviest first, ties sparsest first, then query order
                here.sort(key=lambda c: (-float(weight(c[1], c[2], c[3])), len(leaves[li][c[1]][c[2]][0]), c[0]))
                r = rows[begin[qi, li]: begin[qi, li] + count[qi, li]]
                ubs = []
                for ri, (ci, f, t, b) in enumerate(here):
                    row = r[ri]
                    assert row["weight"] == weight(f, t, b), f"{name}, leaf {li}, row {ri}: weight"
                    flags = int(row["flags"])
                    fx_shift, cache_slot = (flags >> 4) & 15, (flags >> 8) & 255
                    assert cache_slot == fields.index(f), f"{name}, leaf {li}, row {ri}: normInverse table"
                    d, fr = leaves[li][f][t]
                    pairs = np.unique(np.stack([fr, norms[f][li * ROW_LEAF + d]], axis=1), axis=0)
                    vals = api.debug_walk_value(float(row["weight"]), pairs[:, 0], pairs[:, 1], sim.norm_cache(stats.fields[f]), int(row["fx_scale"]), fx_shift)
                    served = (pairs[:, 0] <= 12) & (pairs[:, 1] < 128)
                    if (f, t) != (0, 6):
                        assert int(row["ub"]) == int(vals.max()), f"{name}, leaf {li}, row {ri}: ub {row['ub']} != the best posting's {vals.max()}"
                    else:   # the frontier restated: the best posting a table serves, the (largest freq, smallest norm byte) of the others
                        assert not served.any()
                        pair = api.debug_walk_value(float(row["weight"]), [pairs[:, 0].max()], [pairs[:, 1].min()], sim.norm_cache(stats.fields[f]),
                                                    int(row["fx_scale"]), fx_shift)
                        assert int(row["ub"]) == int(pair[0]) >= int(vals.max()), f"{name}, leaf {li}, row {ri}: ub {row['ub']}, the pair's {pair[0]}, best posting {vals.max()}"
                        seen.add("above_every_posting" if int(row["ub"]) > int(vals.max()) else "attained")
                    assert int(vals.min()) >= 1
                    ubs.append(int(row["ub"]))
                    seen.add(("escape_only" if not served.any() else "both_kinds" if not served.all() else "table_only"))
                    seen.add("shifted" if fx_shift else "unshifted")
                    seen.add("second_field" if cache_slot else "first_field")
                for ri in range(len(here)):
                    after = (max(ubs[ri + 1:], default=0) if use_max else sum(ubs[ri + 1:]))
                    assert int(r[ri]["u_after"]) == after, f"{name}, leaf {li}, row {ri}: u_after"
                    assert int(r[ri]["suffix"]) == (max(ubs[ri], after) if use_max else ubs[ri] + after), f"{name}, leaf {li}, row {ri}: S_c"
        assert seen >= {"escape_only", "both_kinds", "table_only", "shifted", "unshifted", "second_field", "first_field", "above_every_posting"}, seen
    finally:
        for g in segs:
            g.release()
        ctx.close()


# ---- 2 - 4: searches that read the rows, against the oracle ------------------------------------------------------------------------
RANKS = [1, 2, 5, 9, 20, 60, 150, 400]
ONE_SLICE = (10_000_000, 1000)   # every leaf in one searcher slice: a query is ONE work item, whatever the number of leaves


@pytest.fixture(scope="module")
def differ(oracle):
    """Three leaves of 12 288 docs: leaf 1 lacks the query's rarest (heaviest) term -- the other clauses' ranks shift -- and leaf 2
    lacks all of them (it holds a term no query asks for).  1-clause and 8-clause queries; the oracle's answers, computed once."""
    corpus = recut(synth.build_corpus(36_864, RANKS + [3000], n_segments=1), 12_288,
                   keep=lambda leaf, t: leaf == 0 or (leaf == 1 and t != 400) or (leaf == 2 and t == 3000))
    assert len(corpus.segments) == 3 and corpus.segments[2].term_ids.tolist() == [3000] and 400 not in corpus.segments[1].term_ids
    queries = [RANKS, [400], [1], [2, 400], [400, 150, 60, 20, 9, 5, 2, 1]]
    settings = [(10, 50), (100, 1000), (1000, 1000), (20, INT_MAX)]
    exp = {(i, s): oracle.search_bm25(corpus, t, s[0], total_hits_threshold=s[1]) for i, t in enumerate(queries) for s in settings}
    return corpus, queries, settings, exp


def run_differ(ctx, differ):
    corpus, queries, settings, exp = differ
    ix = Index(ctx, corpus)
    try:
        return {s: ix.searcher.search_batch([bq(t) for t in queries], [api.TopScoreDocCollectorManager(s[0], None, s[1])] * len(queries)) for s in settings}
    finally:
        ix.close()


@pytest.mark.parametrize("library", ["product", "development"])
def test_leaves_that_hold_different_terms(library, differ, request):
    if library == "development":
        request.getfixturevalue("dev_lib")
    ctx = api.GpuContext(device_id=0, max_batch=16)
    try:
        ctx.reset_stats()
        got = run_differ(ctx, differ)
        assert ctx.stats()["maxscore_items"] > 0
        for s, res in got.items():
            for i in range(len(res)):
                check(f"differ_{library}_{s}_{i}", res[i], differ[3][(i, s)], *s)
    finally:
        ctx.close()


PART_QUERIES = [[1, 5, 20, 150, 400], [2, 9, 60], RANKS, [5, 400], [150], [9, 20, 150, 400]]
PART_SETTINGS = [(10, 100), (200, 1000)]


@pytest.fixture(scope="module", params=[40, 70], ids=["40_leaves", "70_leaves"])
def many_parts(request, oracle):
    """40 / 70 leaves of 2048 docs in one searcher slice: a query is one work item of 40 parts (the part of a window is found by
    a ballot over the lanes) / of 70 (by the search part by part), a doc window each."""
    n = request.param
    corpus = recut(synth.build_corpus(n * 2048, RANKS, n_segments=1), 2048)
    assert len(corpus.segments) == n
    exp = {(i, s): oracle.search_bm25(corpus, t, s[0], total_hits_threshold=s[1], slicing=ONE_SLICE) for i, t in enumerate(PART_QUERIES) for s in PART_SETTINGS}
    return corpus, exp


def run_many_parts(ctx, corpus, mode):
    """mode "batch": the queries in one call, 72 copies of them -- a launch of that many items gives its heaviest queries the fine
    doc windows; "single": one query per call -- the launch's other workgroups join the one item as helpers."""
    ctx.set_slicing(*ONE_SLICE)
    ix = Index(ctx, corpus)
    try:
        out = {}
        for s in PART_SETTINGS:
            mgr = api.TopScoreDocCollectorManager(s[0], None, s[1])
            if mode == "batch":
                reps = 12
                ctx.reset_stats()
                res = ix.searcher.search_batch([bq(t) for t in PART_QUERIES] * reps, [mgr] * (len(PART_QUERIES) * reps))
                assert ctx.stats()["maxscore_items"] == len(res), "a query of this index is one work item"
                for j, r in enumerate(res[len(PART_QUERIES):]):
                    same_arrays(f"copy_{j}", r, res[j % len(PART_QUERIES)])
                out[s] = res[:len(PART_QUERIES)]
            else:
                out[s] = [ix.searcher.search(bq(t), mgr) for t in PART_QUERIES]
        return out
    finally:
        ix.close()
        ctx.set_slicing()


@pytest.mark.parametrize("mode", ["batch", "single"])
@pytest.mark.parametrize("scatter", ["0", "1"], ids=["docid_order", "scattered"])
def test_items_of_many_parts(dev_lib, monkeypatch, many_parts, scatter, mode):
    corpus, exp = many_parts
    monkeypatch.setenv("NRTGPU_MS_SCATTER", scatter)
    ctx = api.GpuContext(device_id=0, max_batch=128)
    try:
        got = run_many_parts(ctx, corpus, mode)
        for s, res in got.items():
            for i in range(len(res)):
                check(f"parts_{len(corpus.segments)}_{scatter}_{mode}_{s}_{i}", res[i], exp[(i, s)], *s)
    finally:
        ctx.close()


SHAPE_TERMS = [2, 9, 60, 400]


@pytest.fixture(scope="module")
def shaped(oracle):
    """The query shapes over four leaves with deleted docs: minimumNumberShouldMatch 2, DisjunctionMaxQuery with tie breaker 0 and
    0.3, MUST + SHOULD, a FILTER mask.  (name, query, the oracle's answer)."""
    corpus = recut(synth.build_corpus(32_768, RANKS, n_segments=1, delete_fraction=0.03), 8192)
    masks = [synth.random_mask(seg.max_doc, 0.4, 500 + si) for si, seg in enumerate(corpus.segments)]
    tq = tuple(api.TermQuery(0, t) for t in SHAPE_TERMS)
    k, thr = 50, 100
    o = lambda **kw: oracle.search_bm25(corpus, SHAPE_TERMS, k, total_hits_threshold=thr, **kw)
    cases = [
        ("msm2", api.BooleanQuery(tq, 2), o(min_should_match=2)),
        ("dismax_0", api.DisjunctionMaxQuery(tq, 0.0), o(dismax=0.0)),
        ("dismax_0.3", api.DisjunctionMaxQuery(tq, 0.3), o(dismax=0.3)),
        ("must_should", api.BooleanQuery(tq[1:], must=tq[:1]), o(must=[True, False, False, False])),
        ("two_must", api.BooleanQuery(tq[:1] + tq[3:], must=tq[1:3]), oracle.search_bm25(corpus, [9, 60, 2, 400], k, total_hits_threshold=thr, must=[True, True, False, False])),
        ("filter", api.BooleanQuery(tq, 1, (api.MaskFilter(3),)), o(accept=[synth.accept_words(seg, masks[si], None) for si, seg in enumerate(corpus.segments)])),
        ("plain", api.BooleanQuery(tq), o()),
    ]
    return corpus, masks, cases, k, thr


def run_shaped(ctx, shaped):
    corpus, masks, cases, k, thr = shaped
    ix = Index(ctx, corpus)
    try:
        for leaf, m in zip(ix.leaves, masks):
            leaf.set_mask(3, m)
        mgr = api.TopScoreDocCollectorManager(k, None, thr)
        together = ix.searcher.search_batch([c[1] for c in cases], [mgr] * len(cases))
        alone = [ix.searcher.search(c[1], mgr) for c in cases]   # (a batch of one shape: the kernel variant that shape alone asks for)
        return together, alone
    finally:
        ix.close()


@pytest.mark.parametrize("layout", ["two_columns", "packed", "deletes_as_a_mask"])
def test_query_shapes(layout, shaped):
    """packed: the one-word-per-posting layout (deletes are never folded into it); deletes_as_a_mask: the two-column layout with
    the deleted docs left in the postings -- both walks test liveDocs when a doc's score is complete."""
    flags = {"two_columns": 0, "packed": _lib.NRTGPU_FLAG_PACKED_POSTINGS, "deletes_as_a_mask": _lib.NRTGPU_FLAG_NO_LIVE_FOLD}[layout]
    ctx = api.GpuContext(device_id=0, max_batch=16, flags=flags)
    try:
        ctx.reset_stats()
        together, alone = run_shaped(ctx, shaped)
        assert ctx.stats()["maxscore_items"] > 0
        for (name, _, exp), a, b in zip(shaped[2], together, alone):
            check(f"{layout}_{name}_batch", a, exp, shaped[3], shaped[4])
            check(f"{layout}_{name}_alone", b, exp, shaped[3], shaped[4])
    finally:
        ctx.close()


# ---- 5. A/B: the walk that works the bounds out itself returns the same arrays ------------------------------------------------------
def both_walks(monkeypatch, run):
    out = []
    for rows in ("1", "0"):
        monkeypatch.setenv("NRTGPU_MS_WALK_ROWS", rows)
        out.append(run())
    return out


def test_ab_leaves_that_differ(dev_lib, monkeypatch, differ):
    ctx = api.GpuContext(device_id=0, max_batch=16)
    try:
        with_rows, without = both_walks(monkeypatch, lambda: run_differ(ctx, differ))
        for s in with_rows:
            for i, (a, b) in enumerate(zip(with_rows[s], without[s])):
                same_arrays(f"ab_differ_{s}_{i}", a, b)
    finally:
        ctx.close()


@pytest.mark.parametrize("scatter", ["0", "1"], ids=["docid_order", "scattered"])
def test_ab_many_parts(dev_lib, monkeypatch, many_parts, scatter):
    monkeypatch.setenv("NRTGPU_MS_SCATTER", scatter)
    ctx = api.GpuContext(device_id=0, max_batch=128)
    try:
        for mode in ("batch", "single"):
            with_rows, without = both_walks(monkeypatch, lambda: run_many_parts(ctx, many_parts[0], mode))
            for s in with_rows:
                for i, (a, b) in enumerate(zip(with_rows[s], without[s])):
                    same_arrays(f"ab_parts_{scatter}_{mode}_{s}_{i}", a, b)
    finally:
        ctx.close()


@pytest.mark.parametrize("packed", [False, True], ids=["two_columns", "packed"])
def test_ab_query_shapes(dev_lib, monkeypatch, shaped, packed):
    ctx = api.GpuContext(device_id=0, max_batch=16, flags=_lib.NRTGPU_FLAG_PACKED_POSTINGS if packed else 0)
    try:
        with_rows, without = both_walks(monkeypatch, lambda: run_shaped(ctx, shaped))
        for part_a, part_b in zip(with_rows, without):
            for i, (a, b) in enumerate(zip(part_a, part_b)):
                same_arrays(f"ab_shapes_{packed}_{shaped[2][i][0]}", a, b)
    finally:
        ctx.close()
