"""The MaxScore walk completes a surviving doc in a query's later clauses through one of three doc -> posting lookup paths
(plan.h: kLook*; maxscore.hip, "the later clauses of the surviving docs"): records per 32 docs, lookup cells + a lock-step
binary search, or the tile-granular cell table + the same search.  Which term gets which is the seal's decision (segment.cpp:
build_term_aux: policy, nrtgpu_config.lookup_budget_pct), and on test-sized corpora the default never runs out of budget: a
dense term is never searched, a sparse one never has records.  Here every term of a hand-built corpus (tests/_lookup_cases.py)
goes through every structure, with two posting columns and packed, and the answers must be the oracle's bit for bit --
"slower, same results" (include/nrtgpu.h) -- and those of a context that never prunes.

Each case first asks the development library what the terms were given (nrtgpu_debug_term_lookup) and holds the segments' device
bytes to the structures' bytes: a knob that silently does nothing fails before any search runs.  That the lookups ran is the
instrumented kernel's count (nrtgpu_get_maxscore_profile [6]).  tests/test_lookup_policy_host.py pins the same assignments
without a GPU."""
import dataclasses
import math

import numpy as np
import pytest

from nrtsearch_amd import _lib, api, synth
from oracle import oracle

from tests import _lookup_cases as lc
from tests.test_parity_gpu import Index, assert_same

pytestmark = pytest.mark.gpu
THR = 10            # total_hits_threshold: the pruned route, whatever the query
FILTER_ID, MUST_NOT_ID = 1, 2
SHAPES = ("sum", "msm2", "msm3", "dismax0", "dismax03", "must", "filter", "must_not", "after")
SCAN_SHAPES = ("sum", "msm2", "msm3", "dismax0", "filter", "must_not", "after")   # what a context that never prunes serves too


@dataclasses.dataclass
class Spec:
    name: str
    shape: str
    terms: list
    boosts: list
    k: int
    must: list = None          # per clause, MUST first (as the mirror hands them over)


def query_specs(corpus):
    """33 queries: every term of the corpus three times as a clause that is NOT the heaviest -- the walk streams the heaviest
    clause first and looks the surviving docs up in the others, so a sparse term (a large idf) is only ever looked up when a
    boost lifts a denser clause above it.  2 - 8 clauses, k in {1, 10, 100}, every shape about four times."""
    n = corpus.doc_count
    idf = {t: math.log(1.0 + (n - df + 0.5) / (df + 0.5)) for t, df in corpus.doc_freq.items()}
    rng = np.random.Generator(np.random.PCG64(4242))
    out = []
    for i, target in enumerate(sorted(lc.NAMES)):
        for v in range(3):
            n_clauses = 2 + (3 * i + v) % 7
            others = [t for t in sorted(lc.NAMES) if t != target]
            terms = [target] + [int(t) for t in rng.choice(others, size=n_clauses - 1, replace=False)]
            heavy = 1 + v % (n_clauses - 1)
            boosts = [1.0] * n_clauses
            boosts[heavy] = float(math.ceil(1.25 * max(idf[t] for t in terms) / idf[terms[heavy]]))
            if n_clauses > 3:
                boosts[n_clauses - 1 if heavy != n_clauses - 1 else 1] = 0.5
            assert all(boosts[heavy] * idf[terms[heavy]] > b * idf[t] for j, (t, b) in enumerate(zip(terms, boosts)) if j != heavy)
            shape = SHAPES[(i + 4 * v) % len(SHAPES)]
            if shape == "msm3" and n_clauses < 3:
                shape = "msm2"
            must = None
            if shape == "must":       # one MUST clause -- the looked-up term itself every other time -- next to SHOULD clauses
                m = 0 if v % 2 else heavy
                order = [m] + [j for j in range(n_clauses) if j != m]
                terms, boosts = [terms[j] for j in order], [boosts[j] for j in order]
                must = [True] + [False] * (n_clauses - 1)
            out.append(Spec(f"{lc.NAMES[target]}_{v}_{shape}", shape, terms, boosts, (1, 10, 100)[(i + v) % 3], must))
    return out


def clause(t, b):
    return api.BoostQuery(api.TermQuery(0, t), b) if b != 1.0 else api.TermQuery(0, t)


def build_queries(corpus, masks):
    """-> [(spec, query, manager, the oracle's answer)] for one version of the corpus (its liveDocs count)."""
    out = []
    for s in query_specs(corpus):
        cl = tuple(clause(t, b) for t, b in zip(s.terms, s.boosts))
        kw = dict(boosts=s.boosts, total_hits_threshold=THR)
        if s.shape in ("sum", "after"):
            q = api.BooleanQuery(cl)
        elif s.shape in ("msm2", "msm3"):
            q = api.BooleanQuery(cl, int(s.shape[3]))
            kw["min_should_match"] = int(s.shape[3])
        elif s.shape in ("dismax0", "dismax03"):
            tie = 0.0 if s.shape == "dismax0" else float(np.float32(0.3))
            q = api.DisjunctionMaxQuery(cl, tie)
            kw["dismax"] = tie
        elif s.shape == "must":
            q = api.BooleanQuery(cl[1:], 0, (), (), cl[:1])
            kw["must"] = s.must
        elif s.shape == "filter":
            q = api.BooleanQuery(cl, 1, (api.MaskFilter(FILTER_ID),))
            kw["min_should_match"] = 1
            kw["accept"] = [synth.accept_words(seg, masks[FILTER_ID][si], None) for si, seg in enumerate(corpus.segments)]
        else:
            q = api.BooleanQuery(cl, 0, (), (api.MaskFilter(MUST_NOT_ID),))
            kw["accept"] = [synth.accept_words(seg, None, masks[MUST_NOT_ID][si]) for si, seg in enumerate(corpus.segments)]
        after = None
        if s.shape == "after":      # searchAfter from a mid-list hit of the first page
            first = oracle.search_bm25(corpus, s.terms, s.k, **kw)
            assert len(first[0])
            after = (int(first[0][len(first[0]) // 2]), float(first[1][len(first[0]) // 2]))
            kw["after"] = after
        mgr = api.TopScoreDocCollectorManager(s.k, api.ScoreDoc(*after) if after else None, THR)
        out.append((s, q, mgr, oracle.search_bm25(corpus, s.terms, s.k, **kw)))
    return out


@pytest.fixture(scope="module")
def data():
    """Built once: the corpus, its 5 %-deleted version, two masks, the queries with the oracle's answers for both versions; and what
    the cases share across the module -- per layout the device bytes without any structure and the answers of a context that never
    prunes (plain numbers: every handle is closed by the test that made it)."""
    plain = lc.build_corpus()
    deleted = lc.build_corpus(delete_fraction=0.05)
    masks = {FILTER_ID: [synth.random_mask(s.max_doc, 0.4, 71 + i) for i, s in enumerate(plain.segments)],
             MUST_NOT_ID: [synth.random_mask(s.max_doc, 0.3, 91 + i) for i, s in enumerate(plain.segments)]}
    return dict(plain=plain, deleted=deleted, masks=masks, q_plain=build_queries(plain, masks), q_deleted=build_queries(deleted, masks),
                base_bytes={}, no_prune={})


def set_masks(leaves, masks):
    for mid, per_seg in masks.items():
        for leaf, m in zip(leaves, per_seg):
            leaf.set_mask(mid, m)


def run(tag, searcher, queries, no_prune=None):
    """Two batches; every answer against the oracle's, and (the shapes the exhaustive scan serves) against the unpruned context's."""
    half = (len(queries) + 1) // 2
    got = []
    for part in (queries[:half], queries[half:]):
        got += searcher.search_batch([q for _, q, _, _ in part], [m for _, _, m, _ in part])
    for (s, _, _, exp), g in zip(queries, got):
        assert_same(f"{tag}_{s.name}", g, exp, s.k, THR)
        if no_prune is not None and s.shape in SCAN_SHAPES:
            docs, bits = no_prune[s.name]
            assert g.docs.tolist() == docs and g.scores.view(np.uint32).tolist() == bits, f"{tag}_{s.name}: differs from the unpruned context"
    return got


@pytest.mark.parametrize("case", lc.MATRIX, ids=lambda c: c.name)
def test_every_lookup_structure_gives_the_oracles_answers(case, dev_lib, monkeypatch, data):
    monkeypatch.setenv("NRTGPU_LOOK_POLICY", case.policy)      # read by the development build at every seal
    monkeypatch.delenv("NRTGPU_PACKED_POSTINGS", raising=False)
    monkeypatch.delenv("NRTGPU_TEST_LOOKUP_BUDGET_PCT", raising=False)
    flags = _lib.NRTGPU_FLAG_PACKED_POSTINGS if case.packed else 0
    plain, deleted, masks = data["plain"], data["deleted"], data["masks"]
    made_ctx, made_leaves = [], []

    def context(extra=0, pct=case.pct):
        made_ctx.append(api.GpuContext(0, 64, flags=flags | extra, lookup_budget_pct=pct))
        return made_ctx[-1]

    def index(ctx, corpus):
        ix = Index(ctx, corpus)
        made_leaves.extend(ix.leaves)
        set_masks(ix.leaves, masks)
        return ix

    try:
        # ---- shared across the cases of a layout: bytes without structures, the unpruned answers
        if case.packed not in data["base_bytes"]:
            bare = Index(context(pct=-1), plain)
            made_leaves.extend(bare.leaves)
            assert all(leaf.debug_term_lookup(0, int(t))[0] == lc.NONE for leaf, seg in zip(bare.leaves, plain.segments) for t in seg.term_ids)
            data["base_bytes"][case.packed] = [leaf.device_bytes for leaf in bare.leaves]
            scan = index(context(_lib.NRTGPU_FLAG_NO_PRUNE), plain)
            part = [x for x in data["q_plain"] if x[0].shape in SCAN_SHAPES]
            got = scan.searcher.search_batch([q for _, q, _, _ in part], [m for _, _, m, _ in part])
            for (s, _, _, exp), g in zip(part, got):
                assert_same(f"{case.name}_noprune_{s.name}", g, exp, s.k, THR)
            data["no_prune"][case.packed] = {s.name: (g.docs.tolist(), g.scores.view(np.uint32).tolist()) for (s, _, _, _), g in zip(part, got)}
            assert made_ctx[-1].stats()["maxscore_launches"] == 0
        no_prune = data["no_prune"][case.packed]

        # ---- what the terms were given, before any search
        ctx = context()
        ix = Index(ctx, plain)
        made_leaves.extend(ix.leaves)
        exp = lc.expected_for(case, plain)
        for si, (leaf, seg) in enumerate(zip(ix.leaves, plain.segments)):
            got = {int(t): leaf.debug_term_lookup(0, int(t)) for t in seg.term_ids}
            for t, want in lc.PINNED[case.name][si].items():
                assert got[t] == want, (case.name, seg.max_doc, lc.NAMES[t], got[t], want)
            assert got == exp[si], (case.name, seg.max_doc, {lc.NAMES[t]: (got[t], exp[si][t]) for t in got if got[t] != exp[si][t]})
            look = sum(b for _, _, b in exp[si].values())
            assert leaf.device_bytes - data["base_bytes"][case.packed][si] == look + (64 if look else 0), (case.name, seg.max_doc)
        set_masks(ix.leaves, masks)

        # ---- the answers
        ctx.reset_stats()
        run(case.name, ix.searcher, data["q_plain"], no_prune)
        st = ctx.stats()
        assert st["maxscore_launches"] > 0 and st["maxscore_items"] >= len(data["q_plain"]) and st["scan_items"] == 0, st   # every query walked
        # deletes, three ways: folded into the posting columns (a packed context keeps them a mask), never folded, a fork's own
        run(case.name + "_folded", index(ctx, deleted).searcher, data["q_deleted"])
        run(case.name + "_nofold", index(context(_lib.NRTGPU_FLAG_NO_LIVE_FOLD), deleted).searcher, data["q_deleted"])
        forks = [leaf.fork(seg.live_bits) for leaf, seg in zip(ix.leaves, deleted.segments)]
        made_leaves.extend(forks)
        set_masks(forks, masks)
        run(case.name + "_fork", api.GpuIndexSearcher(ctx, forks, api.IndexStatistics.from_corpus(deleted)), data["q_deleted"])

        # ---- the later-clause lookups ran (the instrumented kernel: same results)
        prof = context(_lib.NRTGPU_FLAG_PROFILE)
        px = index(prof, plain)
        assert [leaf.debug_term_lookup(0, lc.DENSE) for leaf in px.leaves] == [e[lc.DENSE] for e in exp]
        prof.reset_stats()
        run(case.name + "_profile", px.searcher, data["q_plain"], no_prune)
        lookups = prof.maxscore_profile()["lookups"]
        print(f"LOOKUP_CASE {case.name} lookups {int(lookups)}")
        assert lookups > 0
    finally:
        for leaf in made_leaves:
            leaf.release()
        for c in made_ctx:
            c.close()
