"""A seeded differential fuzz of the column routes -- sort by field, terms counts and doc-set requests over single-valued and
multi-valued columns -- through the C ABI on the device, against the four NumPy references.  Per round tests/_column_cases.py
(fuzz_round) draws an index -- 1-4 leaves, deletes, masks, the context's slicing / target_items / flags, fourteen columns -- and four
batches of 1-16 requests per entry, every knob of a request mixed inside a batch; here are the upload, the calls and the
comparisons: exact equality of every output field.  The generator draws supported shapes only: the predicate must say so for
EVERY request, none is skipped.  NRT_COLUMN_FUZZ_ROUNDS scales it (default 8).  A failure names round, batch and index:
cc.fuzz_round(BASE, round_)[1][batch][1][index] is the case.  Needs a real MI355X."""
import os

import pytest

from nrtsearch_amd import _lib, api

from tests import _column_cases as cc
from tests import test_column_edges_gpu as edges   # upload, run, supported, check
from tests import test_docset_gpu as dg

pytestmark = pytest.mark.gpu
# The seed of round r is PCG64(BASE + r).  BASE is chosen so that the default rounds hold the floors of
# tests/test_column_cases_host.py (candidate-buffer overflows over full-range keys, cursors inside runs, overflowed counts, empty
# hit sets, four range clauses, mixed arities, queries cut into items): conditions on the inputs, checked there without a device.
BASE = 7180
ROUNDS = int(os.environ.get("NRT_COLUMN_FUZZ_ROUNDS", "8"))


@pytest.fixture(scope="module", autouse=True)
def two_column_postings():
    """The text routes over a column refuse packed postings: only the flagged rounds pack, and say so themselves."""
    mp = pytest.MonkeyPatch()
    mp.delenv("NRTGPU_PACKED_POSTINGS", raising=False)
    yield
    mp.undo()


@pytest.mark.parametrize("round_", range(ROUNDS))
def test_fuzz_column_routes(round_):
    m, batches = cc.fuzz_round(BASE, round_)
    ctx = api.GpuContext(device_id=0, max_batch=16, target_items=m.target_items, flags=m.flags)
    leaves = []
    try:
        if m.slicing != cc.DEFAULT_SLICING:
            ctx.set_slicing(*m.slicing)
        leaves, searcher = edges.upload(ctx, m)
        assert (round_ % 4 == 3) == (m.flags != 0) and all(e.startswith("docset") for e, _ in batches) == (m.flags != 0)
        for bi, (entry, reqs) in enumerate(batches):
            names = [f"round {round_} (leaves {m.sizes}, slicing {m.slicing}, target_items {m.target_items}, flags {m.flags}), batch {bi} ({entry}), "
                     f"index {i}: {cc.describe(r)}" for i, r in enumerate(reqs)]
            for name, r in zip(names, reqs):
                assert edges.supported(searcher, m, r) is True, name
            got = edges.run(searcher, m, entry, reqs)
            d = api.GpuContext.last_diagnostics()
            assert d["items_maxscore"] == 0, names[0]
            if entry.startswith("docset"):   # every query of the call walks every sub-tile, cut as the planner's rule says
                assert d["items_scan"] >= len(reqs) * min(m.docset_items(len(reqs)), 2), names[0]
            for name, r, g in zip(names, reqs, got):
                edges.check(name, m, r, g)
        if m.flags:   # the two text entries refuse these contexts
            text = [cc.Req("sorted", clauses=(2,), column=("s", "int", "wide")), cc.Req("count", clauses=(2,), column=("m", "int", "wide"))]
            for r in text:
                assert edges.supported(searcher, m, r) is False
                with pytest.raises(_lib.NrtGpuError) as e:
                    edges.run(searcher, m, r.entry, [r])
                assert e.value.code == _lib.NRTGPU_ERR_UNSUPPORTED
    finally:
        dg.release(leaves)
        ctx.close()
