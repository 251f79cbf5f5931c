"""A second seeded differential fuzz of nrtgpu_search_bm25_batch against the oracle, beside tests/test_fuzz_gpu.py (which stays as it
is): the knobs that one never draws.  Per round tests/_bm25_cases.py (fuzz_round) builds an index of 1-12 explicit leaves (1 doc ...
65 537 docs, deletes, leaves without liveDocs, leaves that lack some of the terms) and a context -- the searcher's slicing (one
slice, 2 ... 12 of them: the per-slice hit slots, the item cut at the ninth slice, slice_relation_kernel's loop, MaxScore's count
mode), target_items, the lookup budget, packed or plain postings, and a flag set that includes NRTGPU_FLAG_NO_PRUNE (every shape
through the scan's count-carrying variant), NO_MASK_VARIANT and NO_PREFETCH -- and three batches of requests, every shape mixed
inside a batch.  Docids, float32 score bits, the relation and the count as tests/test_bm25_edges_gpu.check holds them.  The
generator draws supported shapes only: the predicate must say so for EVERY request, none is skipped.  NRT_BM25_FUZZ_ROUNDS scales
it (default 8).  A failure names the round, the leaves, the slicing, the flags and the request; bc.fuzz_round(BASE, round_)[2][batch]
[index] is the case.  Needs a real MI355X."""
import os

import pytest

from nrtsearch_amd import api

from tests import _bm25_cases as bc
from tests import test_bm25_edges_gpu as edges   # open_context, upload, run, check, assert_routes, release

pytestmark = pytest.mark.gpu
# The seed of round r is PCG64(BASE + r).  BASE is chosen so that the default rounds hold the floors of
# tests/test_bm25_cases_host.py (both relations; requests in D on either route, but no more than one in ten; nine slices and more
# under both slicings that can give them, on either route; every flag set, both posting layouts): conditions on the inputs, checked
# there without a device.
BASE = 604
ROUNDS = int(os.environ.get("NRT_BM25_FUZZ_ROUNDS", "8"))


@pytest.mark.parametrize("round_", range(ROUNDS))
def test_fuzz_bm25_routes(round_):
    m, knobs, batches = bc.fuzz_round(BASE, round_)
    ctx = edges.open_context(m, knobs.flags, knobs.packed, knobs.budget_pct)
    leaves = []
    try:
        leaves, searcher = edges.upload(ctx, m)
        for bi, reqs in enumerate(batches):
            names = [f"round {round_} (leaves {m.sizes}, slicing {m.slicing}: {len(m.slices)} slices, target_items {m.target_items}, flags {knobs.flags}, "
                     f"{'packed' if knobs.packed else 'plain'}, lookup budget {knobs.budget_pct}), batch {bi}, index {i}: {bc.describe(r)}" for i, r in enumerate(reqs)]
            for name, r in zip(names, reqs):
                assert searcher.supported(bc.query_of(r), bc.manager_of(r)) is True, name
            got = edges.run(searcher, reqs)
            edges.assert_routes(names[0], knobs.flags, api.GpuContext.last_diagnostics(), reqs, m)
            for name, r, g in zip(names, reqs, got):
                edges.check(name, m, r, g)
    finally:
        edges.release(leaves)
        ctx.close()
