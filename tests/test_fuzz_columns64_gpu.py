"""A seeded differential fuzz of the routes over 64-bit doc value columns -- sorted searches over a text query and over a doc set,
masks built from the columns, range counts over both kinds of hit set -- through the C ABI on the device, against the NumPy
references.  Per round tests/_column64_cases.py (fuzz_round) draws an index -- 1-4 leaves, deletes, masks, the context's slicing /
target_items / flags, nine 64-bit columns and three 32-bit ones for the doc sets' range clauses -- and four batches of 1-16 requests
per entry, every knob of a request mixed inside a batch; here are the upload, the calls and the comparisons: exact equality of
every output field.  The generator draws supported shapes only: the predicate must say so for EVERY request, none is skipped.
NRT_COLUMN64_FUZZ_ROUNDS scales it (default 8).  A failure names round, batch and index:
c64.fuzz_round(BASE, round_)[1][batch][1][index] is the case.  Needs a real MI355X."""
import os

import pytest

from nrtsearch_amd import _lib, api

from tests import _column64_cases as c64
from tests import _column_cases as cc
from tests import test_column64_edges_gpu as edges   # upload, run, supported, check, check_mask
from tests import test_field_sort64_gpu as s64

pytestmark = pytest.mark.gpu
# The seed of round r is PCG64(BASE + r).  BASE is chosen so that the default rounds hold the floors of
# tests/test_column64_cases_host.py (candidate-buffer overflows on both sorted entries, cursors inside runs and outside the window,
# sentinel and in-window missing values, empty hit sets, multi-valued range clauses, batches that mix long and double sorts, doc-set
# queries cut into items): conditions on the inputs, checked there without a device.  That is how it was chosen: bases were to be tried
# from 6400 on until one held every floor, and 6400 does (census: tests/test_column64_cases_host.py: take_census(BASE)).
BASE = 6400
ROUNDS = int(os.environ.get("NRT_COLUMN64_FUZZ_ROUNDS", "8"))


@pytest.fixture(scope="module", autouse=True)
def two_column_postings():
    """The text routes over a column refuse packed postings: only the flagged rounds pack, and say so themselves."""
    mp = pytest.MonkeyPatch()
    mp.delenv("NRTGPU_PACKED_POSTINGS", raising=False)
    yield
    mp.undo()


@pytest.mark.parametrize("round_", range(ROUNDS))
def test_fuzz_column64_routes(round_):
    m, batches = c64.fuzz_round(BASE, round_)
    ctx = api.GpuContext(device_id=0, max_batch=16, target_items=m.target_items, flags=m.flags)
    leaves = []
    try:
        if m.slicing != cc.DEFAULT_SLICING:
            ctx.set_slicing(*m.slicing)
        leaves, searcher = edges.upload(ctx, m)
        assert (round_ % 4 == 3) == (m.flags != 0) and all(e.startswith("docset") for e, _ in batches) == (m.flags != 0)
        for bi, (entry, reqs) in enumerate(batches):
            names = [f"round {round_} (leaves {m.sizes}, slicing {m.slicing}, target_items {m.target_items}, flags {m.flags}), batch {bi} ({entry}), "
                     f"index {i}: {c64.describe(r)}; replay: c64.fuzz_round({BASE}, {round_})[1][{bi}][1][{i}]" for i, r in enumerate(reqs)]
            if entry == "mask64":
                for name, r in zip(names, reqs):
                    edges.check_mask(name, m, r, leaves)
                continue
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
            text = [c64.Req("sorted64", clauses=(2,), column=("s", "long", "best")),
                    c64.Req("ranges64", clauses=(2,), column=("s", "double", "pos"), count_ranges=((c64.KIND_MIN["double"], c64.KIND_MAX["double"]),))]
            for r in text:
                assert edges.supported(searcher, m, r) is False
                with pytest.raises(_lib.NrtGpuError) as e:
                    edges.run(searcher, m, r.entry, [r])
                assert e.value.code == _lib.NRTGPU_ERR_UNSUPPORTED
    finally:
        s64.release(leaves)
        ctx.close()
