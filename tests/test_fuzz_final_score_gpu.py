"""A seeded differential fuzz of the four routes on csrc/finalscore.hiph's skeleton -- function score, multi-match, function score
over multi-match, a text query beside knn clauses -- through the C ABI on the device, against the four NumPy references.  Per
round tests/_final_score_cases.py (fuzz_round) draws an index -- 1-12 leaves, 1-4 fields, deletes, leaves without liveDocs, four
masks, the context's slicing and target_items -- and two batches of 1-16 requests per entry, every knob of a request mixed inside
a batch: shapes, operators, minima, tie breakers, boosts, functions and modes, masks, cursors, min_score, knn lists.  Here are the
upload, the calls and the comparisons: docids, float32 score bits, count and relation, exactly.  The generator draws supported
shapes only: the predicate must say so for EVERY request, none is skipped.  NRT_FINAL_FUZZ_ROUNDS scales it (default 8).  A failure
names round, batch and index: fc.fuzz_round(BASE, round_)[1][batch][1][index] is the case.  Needs a real MI355X."""
import os

import pytest

from nrtsearch_amd import api

from tests import _final_score_cases as fc
from tests import test_final_score_edges_gpu as edges   # open_context, upload, supported, run, check, release

pytestmark = pytest.mark.gpu
# The seed of round r is PCG64(BASE + r).  BASE is chosen so that the default rounds hold the floors of
# tests/test_final_score_cases_host.py (candidate-buffer overflows, cursors inside runs of equal final scores, empty hit sets,
# min_scores that cut, more than 8 slices, items of 4 leaves, 4 fields, 24 clauses, 8 functions, omitted leaves, the four kinds of
# listed docs): conditions on the inputs, checked there without a device.
BASE = 100
ROUNDS = int(os.environ.get("NRT_FINAL_FUZZ_ROUNDS", "8"))


@pytest.fixture(scope="module", autouse=True)
def two_column_postings():
    """The routes refuse packed postings: these contexts keep the two-column layout whatever the suite runs under."""
    mp = pytest.MonkeyPatch()
    mp.delenv("NRTGPU_PACKED_POSTINGS", raising=False)
    yield
    mp.undo()


@pytest.mark.parametrize("round_", range(ROUNDS))
def test_fuzz_final_score_routes(round_):
    m, batches = fc.fuzz_round(BASE, round_)
    ctx = edges.open_context(m)
    leaves = []
    try:
        leaves, searcher = edges.upload(ctx, m)
        for bi, (entry, reqs) in enumerate(batches):
            names = [f"round {round_} (leaves {m.sizes}, {len(m.fields)} fields, slicing {m.slicing}, target_items {m.target_items}), batch {bi} ({entry}), "
                     f"index {i}: {fc.describe(r)}" for i, r in enumerate(reqs)]
            for name, r in zip(names, reqs):
                assert edges.supported(searcher, m, r) is True, name
            got = edges.run(searcher, m, entry, reqs)
            d = api.GpuContext.last_diagnostics()
            assert d["items_maxscore"] == 0 and d["items_scan"] >= sum(1 for r in reqs if m.kept_leaves(r)), names[0]
            for name, r, g in zip(names, reqs, got):
                edges.check(name, m, r, g)
    finally:
        edges.release(leaves)
        ctx.close()
