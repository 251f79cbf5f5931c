"""An overflow compaction keeps the keys that can still matter (maxscore.hip: ms_compact): those that reach the largest bound the
workgroup holds -- the k-th key, the guess the selection yields, the theta it came with, the query's theta_g -- not the k best.
The rule differs from "keep the k best" only where an item overflows its candidate buffer (2304 slots) with a bound above the
k-th key in hand, and a dropped key can only be missed at a LATER compaction or in the item's epilogue: inputs that overflow at
least twice with a guess in between.

Corpora: 60 k docs in one segment; the same docs cut into segments of 30 k / 20 k / 10 k (parts change); 1 M docs in one segment.
A doc window is 65,536 docs, so the 60 k corpora are ONE window per segment: every window is begun before the first overflow, the
workgroup counts its share of the query's windows as 1 and makes no guess (ms_compact: r = 0) -- there the two rules differ by
nothing, and the queries check the overflow path itself (measured: 2 - 3 overflow meetings per query at numHits 1000, 0 guesses).
A searcher's slices do not cut a query into items either -- its cost does: the two-slice queries check the relation per slice.
Guesses between two overflows need windows that are begun one after another: the 1 M corpus (16 windows for 12 waves; measured
at numHits 1000 with one item per query: 4 - 5 overflow meetings, a guess in all or all but one of them).  The TWO-ITEM queries,
where theta_g feeds the filter, are the 1 M corpus under target_items = 2 (measured: 5 - 6 overflow meetings over the two items
against 6 - 8 under the old rule, a guess in each).  Guesses rarely FAIL on these corpora whatever the margin: the share errs
high (a window begun counts as walked), so the guess errs low.  The re-run path is therefore driven the way test_maxscore_gpu.py
drives it -- 49 windows walked in docid order, the live docs at the front, so that a workgroup has seen the hits when it still
expects more -- at a margin of 0.25, and with every live doc in the FIRST window: with the first 30 % live the overflow that could
fail falls where the workgroup holds about as many of the final top-k as its guess's rank (measured: 0 - 2 re-runs of 6 queries,
run to run), with one live window the second overflow comes when a third to two thirds of the hits are seen by a workgroup that
expects a quarter (measured: 6 re-runs of 6 queries under either rule, eight runs of eight;
test_failed_guesses_are_run_again_under_both_rules).

numHits 1 and 10 are run and compared like the others, but cannot overflow twice: after the first overflow theta is the best (10th
best) of at least 2304 docs, and of the at most 46,600 matching docs that follow about k x ln(48,900 / 2304) = 3 (31) beat it -- far
from the 2300 that a second overflow takes.  The not-vacuous assertions are made for numHits 1000 and 1024.

Answers are compared with the oracle's exhaustive ones, exactly (docids, ranks, score bits, relation; totalHits a lower bound above
max(threshold, numHits)), per slice where the searcher is sliced.  Needs a real MI355X."""
import dataclasses

import numpy as np
import pytest

from nrtsearch_amd import _lib, api, synth

pytestmark = pytest.mark.gpu

RANKS = [1, 2, 3, 5, 8]                           # dense terms: every second to every ninth doc
QUERIES = [[1, 2, 3], [2, 5, 8], [1, 2, 3, 5, 8]]
KS = (1, 10, 1000, 1024)
THR = 10                                          # totalHitsThreshold: the items run in Prune mode from their first doc
MSM_QUERY, MSM = [1, 2, 3, 5, 8], 2               # the clause-counting instantiation (SHAPES = 1)
CAND_CAP = 2304                                   # plan.h: kMsCandCap
MARGINS = (None, 0.0, 0.25)                       # the default margin (5), speculation off, guesses that fail
TWO_SLICES = (35_000, 2)                          # 30 k + 20 k | 10 k: two items per query, theta_g feeds the filter


def recut(corpus, sizes):
    """The single-segment corpus cut into segments of the given sizes (the same docs, docids and statistics)."""
    (seg,) = corpus.segments
    assert sum(sizes) == seg.max_doc
    out, base = [], 0
    for size in sizes:
        docs, freqs, counts = [], [], []
        for t in seg.term_ids:
            d, f = seg.postings(int(t))
            lo, hi = np.searchsorted(d, [base, base + size])
            docs.append((d[lo:hi] - base).astype(np.int32))
            freqs.append(f[lo:hi])
            counts.append(hi - lo)
        out.append(synth.SegmentData(max_doc=int(size), doc_base=int(base), norms=seg.norms[base: base + size].copy(), term_ids=seg.term_ids.copy(),
                                     offsets=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64),
                                     docids=np.ascontiguousarray(np.concatenate(docs), dtype=np.int32),
                                     freqs=np.ascontiguousarray(np.concatenate(freqs), dtype=np.int32), live_bits=None))
        base += size
    return dataclasses.replace(corpus, segments=out)


def bq(terms, msm=0):
    return api.BooleanQuery(tuple(api.TermQuery(0, int(t)) for t in terms), msm)


def check(name, got, exp, k):
    edocs, escores, etotal, egte = exp
    assert got.docs.tolist() == edocs.tolist(), f"{name}: docids/ranks differ"
    assert got.scores.view(np.uint32).tolist() == escores.view(np.uint32).tolist(), f"{name}: score bits differ"
    assert got.relation_gte == egte, f"{name}: relation"
    if egte:
        assert max(THR, k) < got.total_hits <= etotal, f"{name}: lower bound {got.total_hits} not in ({max(THR, k)}, {etotal}]"
    else:
        assert got.total_hits == etotal, f"{name}: totalHits {got.total_hits} != {etotal}"


def cases_of(slicing):
    """(name, terms, msm, k, slicing): every query at every numHits, the counting query, and -- on the segmented corpus -- a query whose
    searcher has two slices."""
    out = [(f"{'_'.join(map(str, t))}_k{k}", t, 0, k, None) for t in QUERIES for k in KS]
    out.append((f"msm{MSM}_k1000", MSM_QUERY, MSM, 1000, None))
    if slicing is not None:
        out += [(f"two_slices_{'_'.join(map(str, t))}_k{k}", t, 0, k, slicing) for t in (QUERIES[0], QUERIES[2]) for k in (10, 1000)]
    return out


def expected(oracle, which, corpus, slicing):
    cases = cases_of(slicing)
    exp = {}
    for name, terms, msm, k, sl in cases:
        exp[name] = oracle.search_bm25(corpus, terms, k, total_hits_threshold=THR, min_should_match=msm, slicing=sl)
        total = oracle.search_bm25(corpus, terms, k, total_hits_threshold=2**31 - 1, min_should_match=msm, slicing=sl)[2]
        assert total >= 3 * CAND_CAP, f"{name}: {total} docs match, the buffer overflows at most {total // CAND_CAP} times"
    return which, corpus, cases, exp


@pytest.fixture(scope="module")
def big(oracle):
    """(name, corpus, cases, the oracle's exhaustive answer per case) of the 1 M corpus: computed once, shared, never changed."""
    return expected(oracle, "1_segment_1m", synth.build_corpus(1_000_000, RANKS, n_segments=1), None)


@pytest.fixture(scope="module", params=["1_segment_60k", "3_segments_30k_20k_10k", "1_segment_1m"])
def case(request, oracle):
    """... and of every corpus."""
    if request.param == "1_segment_1m":
        return request.getfixturevalue("big")
    corpus = synth.build_corpus(60_000, RANKS, n_segments=1)
    slicing = None
    if request.param.startswith("3_"):
        corpus, slicing = recut(corpus, [30_000, 20_000, 10_000]), TWO_SLICES
        assert len(oracle.corpus_slices(corpus, slicing)) == 2
    return expected(oracle, request.param, corpus, slicing)


def run_cases(ctx, ix, cases, exp, tag):
    """Every case in one call per slicing (a searcher's slicing is its context's when it is made)."""
    leaves, stats = ix
    out = {}
    for sl in sorted({c[4] for c in cases}, key=lambda s: s is not None):
        sel = [c for c in cases if c[4] == sl]
        ctx.set_slicing(*sl) if sl is not None else ctx.set_slicing()
        try:
            sr = api.GpuIndexSearcher(ctx, leaves, stats)
            got = sr.search_batch([bq(t, msm) for _, t, msm, _, _ in sel], [api.TopScoreDocCollectorManager(k, None, THR) for _, _, _, k, _ in sel])
        finally:
            ctx.set_slicing()
        for (name, _, _, k, _), g in zip(sel, got):
            check(f"{tag}_{name}", g, exp[name], k)
            out[name] = (g.docs.tolist(), g.scores.view(np.uint32).tolist(), g.relation_gte)
    return out


def open_index(ctx, corpus):
    leaves = [api.GpuSegment.from_data(ctx, s) for s in corpus.segments]
    return leaves, (leaves, api.IndexStatistics.from_corpus(corpus))


def test_every_margin_returns_the_exhaustive_answer(case):
    """The product library: the default margin, speculation off, and a margin at which guesses fail and the queries are run again --
    the oracle's answer each time, hence identical answers."""
    which, corpus, cases, exp = case
    ctx = api.GpuContext(device_id=0, max_batch=64)
    leaves, sr = open_index(ctx, corpus)
    try:
        outs = []
        for margin in MARGINS:
            if margin is not None:
                ctx.set_speculation(margin)
            outs.append(run_cases(ctx, sr, cases, exp, f"margin_{margin}"))
            c = ctx.spec_counters()
            print(which, "margin", margin, c)
            assert not c["switched_off"], c
            if margin == 0.0:
                assert c["reruns"] == 0, c
        assert outs[0] == outs[1] == outs[2]
    finally:
        for l in leaves:
            l.release()
        ctx.close()


def both_rules(monkeypatch, ctx, ix, which, deep, exp, two_items):
    """Every deep case, one query per call so that the counts are one query's, under the new and the old compaction rule and at each
    margin: identical answers (the oracle's), overflows that make the comparison mean something, and guesses where they can be."""
    for margin in (None, 0.25, 0.0):
        if margin is not None:
            ctx.set_speculation(margin)
        for c in deep:
            name = c[0]
            counts = {}
            for rule in ("1", "0"):
                monkeypatch.setenv("NRTGPU_MS_KEEP_LIVE", rule)
                ctx.reset_stats()
                before = ctx.spec_counters()["reruns"]
                counts[rule] = (run_cases(ctx, ix, [c], exp, f"rule_{rule}_margin_{margin}"), ctx.maxscore_meetings(),
                                ctx.spec_counters()["reruns"] - before, int(ctx.stats()["maxscore_items"]))
            (new, m_new, re_new, it_new), (old, m_old, re_old, it_old) = counts["1"], counts["0"]
            print(which, name, "items" if not two_items else "two items:", it_new, "margin", margin, "keep live:", m_new, "reruns", re_new, "| keep k:", m_old, "reruns", re_old)
            assert new == old, f"{name}: the two compaction rules disagree"
            for m, re, items in ((m_new, re_new, it_new), (m_old, re_old, it_old)):
                # (sums over the query's walks -- a query run again walks twice.  One item per walk: two overflows in each; two items:
                #  more overflows than items, so one of them overflowed twice)
                if two_items:
                    assert items >= 2 and items % 2 == 0, f"{name}: {items} items"
                    assert m["overflow_meetings"] > max(items, 2 * (1 + re)), f"{name}: {m}, {items} items -- no item overflowed twice"
                else:
                    assert 1 <= items <= 1 + re, f"{name}: {items} items"
                    assert m["overflow_meetings"] >= 2 * (1 + re), f"{name}: {m}, {re} re-runs -- an item that did not overflow twice"
            # a guess: where the workgroup's share of the query's windows is below 1 when it overflows (windows begun one after
            # another, or a second item), with speculation on
            if margin != 0.0 and which == "1_segment_1m":
                assert m_new["meeting_guesses"] + m_new["wave_estimates"] >= 1, f"{name}: {m_new} -- no guess"
                assert m_old["meeting_guesses"] + m_old["wave_estimates"] >= 1, f"{name}: {m_old} -- no guess"
            if margin == 0.0:
                assert m_new["meeting_guesses"] == 0 and m_new["wave_estimates"] == 0, m_new


def test_the_items_overflow_twice_with_a_guess_and_both_rules_agree(dev_lib, monkeypatch, case):
    """The instrumented instantiation of the development library: at numHits 1000 and 1024 every query's item meets for at least two
    overflows, and -- on the corpus of many windows -- a meeting publishes a guess.  NRTGPU_MS_KEEP_LIVE=0 brings back the old rule
    (the k best stay): the same answers, key for key.  One item per query here (target_items = 1)."""
    which, corpus, cases, exp = case
    monkeypatch.setenv("NRTGPU_MS_SCATTER", "0")
    ctx = api.GpuContext(device_id=0, max_batch=64, target_items=1, flags=_lib.NRTGPU_FLAG_PROFILE)
    leaves, ix = open_index(ctx, corpus)
    try:
        both_rules(monkeypatch, ctx, ix, which, [c for c in cases if c[3] >= 1000], exp, False)
        # the shallow queries under both rules as well (one call each)
        shallow = [c for c in cases if c[3] < 1000]
        ctx.set_speculation(5.0)
        monkeypatch.setenv("NRTGPU_MS_KEEP_LIVE", "1")
        a = run_cases(ctx, ix, shallow, exp, "shallow_new")
        monkeypatch.setenv("NRTGPU_MS_KEEP_LIVE", "0")
        assert a == run_cases(ctx, ix, shallow, exp, "shallow_old")
    finally:
        for l in leaves:
            l.release()
        ctx.close()


def test_two_items_of_a_query_share_theta_through_the_filter(dev_lib, monkeypatch, big):
    """A query cut into TWO items (target_items = 2: two doc ranges of the 1 M corpus; a searcher's slices do not cut a query, a
    query's cost does): each item's share of the query's windows stays below 1, its compactions filter by what the other has
    published in theta_g, and the answers are the oracle's under both rules."""
    which, corpus, cases, exp = big   # (the 60 k corpora are below the cost of one item: nothing to cut)
    monkeypatch.setenv("NRTGPU_MS_SCATTER", "0")
    ctx = api.GpuContext(device_id=0, max_batch=64, target_items=2, flags=_lib.NRTGPU_FLAG_PROFILE)
    leaves, ix = open_index(ctx, corpus)
    try:
        both_rules(monkeypatch, ctx, ix, which, [c for c in cases if c[3] == 1000], exp, True)
    finally:
        for l in leaves:
            l.release()
        ctx.close()


def test_failed_guesses_are_run_again_under_both_rules(dev_lib, monkeypatch, oracle):
    """Guesses that fail (margin 0.25; docs not spread like a sample: every live doc in the first of 49 doc windows, windows in docid
    order): the merge catches them, the queries are run again, and the answers are the oracle's under either compaction rule -- a
    key dropped below a guess that then failed is found again by the re-run."""
    monkeypatch.setenv("NRTGPU_MS_SCATTER", "0")
    corpus = synth.build_corpus(3_200_000, RANKS, n_segments=1)   # 49 doc windows, one item (+ helpers)
    seg = corpus.segments[0]
    live = np.zeros((seg.max_doc + 63) // 64, dtype=np.uint64)
    live[: 65_536 // 64] = np.uint64(0xFFFFFFFFFFFFFFFF)   # (33 k - 53 k hits per query: the buffer overflows at about 2.3 k and 20 k of them)
    seg.live_bits = live
    exp = {(i, k): oracle.search_bm25(corpus, t, k, total_hits_threshold=THR) for i, t in enumerate(QUERIES) for k in (1000, 1024)}
    ctx = api.GpuContext(device_id=0, max_batch=64, flags=_lib.NRTGPU_FLAG_PROFILE)
    leaves = [api.GpuSegment.from_data(ctx, s) for s in corpus.segments]
    sr = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics.from_corpus(corpus))
    try:
        leaves[0].set_live_docs(live)
        answers = {}
        for rule in ("1", "0"):
            monkeypatch.setenv("NRTGPU_MS_KEEP_LIVE", rule)
            ctx.set_speculation(0.25)    # (resets the counters)
            ctx.reset_stats()
            got = sr.search_batch([bq(t) for t in QUERIES for _ in (1000, 1024)],
                                  [api.TopScoreDocCollectorManager(k, None, THR) for _ in QUERIES for k in (1000, 1024)])
            it = iter(got)
            for i in range(len(QUERIES)):
                for k in (1000, 1024):
                    g = next(it)
                    check(f"skewed_rule_{rule}_{i}_{k}", g, exp[(i, k)], k)
                    answers[(rule, i, k)] = (g.docs.tolist(), g.scores.view(np.uint32).tolist())
            c, m = ctx.spec_counters(), ctx.maxscore_meetings()
            print("skewed, keep live" if rule == "1" else "skewed, keep k", c, m)
            assert c["reruns"] >= 1, c
            assert m["overflow_meetings"] >= 2 * len(got) and m["meeting_guesses"] + m["wave_estimates"] >= 1, m
        assert all(answers[("1", i, k)] == answers[("0", i, k)] for i in range(len(QUERIES)) for k in (1000, 1024))
    finally:
        for l in leaves:
            l.release()
        ctx.close()
