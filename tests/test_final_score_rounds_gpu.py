"""The edges of the rounds both final-score kernels run (funcscore.hip, multimatch.hip; finalscore.hiph), at both workgroup shapes --
12 waves and 3072 candidate slots (function score), 8 waves and 2048 (multi-match): one leaf, one field, one term that EVERY doc
holds, so the sub-tiles and the candidates of a round are known from max_doc alone (theta starts at 0: every doc is a candidate):

  max_doc 1, 1023, 1024, 1025   fewer sub-tiles than waves; a sub-tile with a short last word; exactly one; one doc into a second
  max_doc 8 * 1024 + 1          a second round in which a single wave works, at 8 waves
  max_doc 12 * 1024 + 1         the same at 12 waves
  k = 1024 at the two largest   the first round brings more candidates than either buffer holds: wave by wave through topk_compact

Every case through search_function_score_batch (no functions; one weight function over every third doc) and through
search_multi_match_batch (one group, both shapes), against tests/_function_score_ref.py and tests/_multi_match_ref.py: docids,
float32 score bits, total hits and the relation, bit for bit.  And a term no leaf holds: zero items, no launch.  Needs a real MI355X."""
import numpy as np
import pytest

from nrtsearch_amd import api, synth
from oracle import oracle

from tests import _function_score_ref as fs_ref
from tests import _multi_match_ref as mm_ref
from tests.test_parity_gpu import assert_same

pytestmark = pytest.mark.gpu
TERM, TERM_NOWHERE, MASK = 1, 99, 7
SIZES = (1, 1023, 1024, 1025, 8 * 1024 + 1, 12 * 1024 + 1)
KS = (1, 1024)
WEIGHT = ((MASK, 2.5),)
GROUPS = [[(0, TERM, 1.0)]]


@pytest.fixture(scope="module", autouse=True)
def two_column_postings():
    """The routes refuse packed postings: these contexts keep the two-column layout also where the whole suite runs with
    NRTGPU_PACKED_POSTINGS=1, which packs every api.GpuContext."""
    mp = pytest.MonkeyPatch()
    mp.delenv("NRTGPU_PACKED_POSTINGS", raising=False)
    yield
    mp.undo()


@pytest.fixture(scope="module")
def ctx(two_column_postings):
    c = api.GpuContext(device_id=0, max_batch=16)
    yield c
    c.close()


def corpus_of(max_doc):
    """One leaf whose every doc holds TERM; freqs (a few above 12: escape codes) and lengths from a fixed seed, so scores differ."""
    rng = np.random.default_rng(1000 + max_doc)
    lengths = np.clip(np.rint(np.exp(rng.normal(np.log(80.0), 0.6, size=max_doc))), 4, 4000).astype(np.int64)
    freqs = np.minimum(rng.geometric(0.45, size=max_doc), 20).astype(np.int32)
    seg = synth.SegmentData(max_doc=max_doc, doc_base=0, norms=synth.int_to_byte4(lengths), term_ids=np.array([TERM], np.int64),
                            offsets=np.array([0, max_doc], np.int64), docids=np.arange(max_doc, dtype=np.int32), freqs=freqs)
    return synth.Corpus(n_docs=max_doc, doc_count=max_doc, sum_total_term_freq=int(lengths.sum()), segments=[seg], doc_freq={TERM: max_doc})


class Ix:
    def __init__(self, ctx, corpus):
        self.leaves, stats = mm_ref.upload(api, ctx, [corpus])
        self.masks = {(0, MASK): mm_ref.words_of(np.arange(corpus.n_docs) % 3 == 0)}
        self.leaves[0].set_mask(MASK, self.masks[(0, MASK)])
        self.searcher = api.GpuIndexSearcher(ctx, self.leaves, stats)

    def function_score(self, term, cases):
        qs = [api.FunctionScoreQuery(api.TermQuery(0, term), tuple(api.WeightFunction(float(w), int(m)) for m, w in fn), "multiply", "multiply",
                                     0.0, False) for fn, _ in cases]
        return self.searcher.search_function_score_batch(qs, [api.TopScoreDocCollectorManager(k) for _, k in cases])

    def multi_match(self, term, cases):
        qs = [mm_ref.to_query(api, [[(0, term, 1.0)]], shape, "should", 0, 0.3) for shape, _ in cases]
        return self.searcher.search_multi_match_batch(qs, [api.TopScoreDocCollectorManager(k) for _, k in cases])

    def close(self):
        for leaf in self.leaves:
            leaf.release()


def same(name, got, exp, k):
    assert_same(name, got, exp, k, 1000)
    assert got.total_hits == exp[2], f"{name}: total_hits {got.total_hits}, the reference counts {exp[2]}"


@pytest.mark.parametrize("max_doc", SIZES)
def test_rounds_at_both_workgroup_shapes(ctx, max_doc):
    corpus = corpus_of(max_doc)
    x = Ix(ctx, corpus)
    try:
        cases = [(fn, k) for k in KS for fn in ((), WEIGHT)]
        for (fn, k), td in zip(cases, x.function_score(TERM, cases)):
            exp = fs_ref.search(oracle, corpus, [TERM], k, fn, "multiply", "multiply", masks=x.masks)
            assert exp[2] == max_doc
            same(f"function_score_{max_doc}_{k}_{len(fn)}", td, exp, k)
        d = api.GpuContext.last_diagnostics()
        assert d["items_maxscore"] == 0 and d["items_scan"] == len(cases)   # one item per query: the rounds are one workgroup's
        cases = [(shape, k) for k in KS for shape in ("cross_fields", "best_fields")]
        for (shape, k), td in zip(cases, x.multi_match(TERM, cases)):
            exp = mm_ref.search(oracle, [corpus], GROUPS, shape, k, tie_breaker=0.3)
            assert exp[2] == max_doc
            same(f"multi_match_{max_doc}_{k}_{shape}", td, exp, k)
        d = api.GpuContext.last_diagnostics()
        assert d["items_maxscore"] == 0 and d["items_scan"] == len(cases)
    finally:
        x.close()


def test_a_term_no_leaf_holds_launches_nothing(ctx):
    x = Ix(ctx, corpus_of(1025))
    try:
        for route, run, cases in (("function_score", x.function_score, [((), 10), (WEIGHT, 1024)]),
                                  ("multi_match", x.multi_match, [("cross_fields", 10), ("best_fields", 1024)])):
            before = ctx.stats()
            got = run(TERM_NOWHERE, cases)
            for td in got:
                assert len(td.docs) == 0 and len(td.scores) == 0 and td.total_hits == 0 and not td.relation_gte, route
            assert api.GpuContext.last_diagnostics()["items_scan"] == 0, route
            after = ctx.stats()
            assert after["batches"] == before["batches"] + 1 and after["queries"] == before["queries"] + len(cases), route
            assert after["scan_launches"] == before["scan_launches"] and after["scan_items"] == before["scan_items"], route
    finally:
        x.close()
