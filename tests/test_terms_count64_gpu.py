"""The terms aggregation over 64-bit columns (nrtgpu_count_terms64_batch, nrtgpu_count_docset_terms64_batch) through the C ABI on the
device, against tests/_terms_count64_ref.py.  Every comparison is exact equality: the buckets' 64 value bits and their order, the
counts, total_hits, hits_with_value, overflowed.  The indexes and the fuzz are tests/_terms_count64_cases.py's.  Needs a real MI355X."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from nrtsearch_amd import _lib, api

from tests import _field_sort64_ref as f64
from tests import _field_sort_ref as fs
from tests import _terms_count64_cases as cases
from tests.test_terms_count64_host import FUZZ_BASE, FUZZ_ROUNDS

pytestmark = pytest.mark.gpu
UNS, INV = _lib.NRTGPU_ERR_UNSUPPORTED, _lib.NRTGPU_ERR_INVALID_ARG
Req = cases.Req
LDS_PROBE = 8   # steps of a probe in the workgroup's table (include/nrtgpu.h: nrtgpu_terms_home_slots64): 9 values on one home slot exhaust it


@pytest.fixture(scope="module", autouse=True)
def two_column_postings():
    """The text route refuses packed postings: these contexts keep the two-column layout also where the whole suite runs with
    NRTGPU_PACKED_POSTINGS=1."""
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


def more_columns(g, si):
    """field 40: a 64-bit column under different kinds on leaves 0 and 1"""
    g.add_doc_values64(40, "long" if si != 1 else "double", np.zeros(g.max_doc, dtype=np.uint64))


@pytest.fixture(scope="module")
def a(ctx):
    ix = cases.index_a()
    leaves, searcher = cases.upload(ctx, ix, more=more_columns)
    yield ix, searcher
    release(leaves)


def run_and_check(ix, searcher, reqs, what):
    got = cases.run(searcher, ix, reqs)
    assert api.GpuContext.last_diagnostics()["items_maxscore"] == 0
    for i, (r, g) in enumerate(zip(reqs, got)):
        cases.check(f"{what} [{i}] {cases.describe(r)}", r.column[0], g, ix.expected(r))
    return got


# ---- index A: every column under every hit set of both forms -------------------------------------------------------------------
@pytest.mark.parametrize("docset", [False, True])
def test_every_column_under_every_hit_set(a, docset):
    ix, searcher = a
    reqs = [Req(key, 1024, **s) for key in ix.columns for s in cases.shapes(docset)]
    got = run_and_check(ix, searcher, reqs, "index A")
    assert api.GpuContext.last_diagnostics()["items_scan"] >= len(reqs) // 2
    assert sum(1 for g in got if len(g.counts) > 600) >= 4 and all(not g.overflowed and g.total_hits > 0 for g in got)
    assert any(ix.unvalued(r) > 0 for r in reqs)
    for r in reqs[:: 7]:
        assert cases.supported(searcher, ix, r) is True


@pytest.mark.parametrize("docset", [False, True])
def test_the_edge_buckets_come_back_as_listed(a, docset):
    """INT64_MIN and INT64_MAX are both there and ordered; the zeros are two buckets; the NaNs -- three payloads, both signs -- are
    one bucket, last, reported canonical."""
    ix, searcher = a
    shape = dict(docset=True) if docset else dict(clauses=(1, 2, 3))
    lg, db = run_and_check(ix, searcher, [Req(("long", "edge"), 16, **shape), Req(("double", "edge"), 7, **shape)], "edge")
    assert lg.values.tolist() == [f64.INT64_MIN, f64.INT64_MIN + 1, -1, 0, 1, f64.INT64_MAX - 1, f64.INT64_MAX] and lg.values.dtype == np.int64
    assert db.value_bits.tolist() == cases.DOUBLE_EDGE.tolist() + [f64.CANONICAL_NAN] and db.values.dtype == np.float64
    assert db.value_bits.tolist()[1:3] == [0x8000000000000000, 0] and np.isnan(db.values[-1]) and db.values[-2] == np.inf
    nan_docs = sum(int(np.isin(col[1], cases.u64(cases.NANS)).sum()) for col in ix.columns[("double", "edge")] if col is not None)
    assert 0 < db.counts[-1] <= nan_docs and min(lg.counts) >= 1


@pytest.mark.parametrize("docset", [False, True])
def test_the_reserved_code(a, docset):
    """Long.MIN_VALUE's code is the word that marks an empty key slot, Long.MAX_VALUE's the all-ones word: both are buckets like any
    other, and each claims exactly one."""
    ix, searcher = a
    shape = dict(docset=True) if docset else dict(clauses=(1,))
    for end, value in (("min", f64.INT64_MIN), ("max", f64.INT64_MAX)):
        only, three_fit, three_over = run_and_check(ix, searcher, [Req(("long", end + "_only"), 1, **shape), Req(("long", end + "3"), 3, **shape),
                                                                     Req(("long", end + "3"), 2, **shape)], end)
        assert not only.overflowed and only.values.tolist() == [value] and only.counts[0] == only.hits_with_value > 100
        assert not three_fit.overflowed and sorted(three_fit.values.tolist()) == sorted([value, -7, cases.EPOCH])
        assert three_over.overflowed and three_over.hits_with_value == -1 and three_over.total_hits == three_fit.total_hits
        for r in (Req(("long", end + "_only"), 1, **shape), Req(("long", end + "3"), 2, **shape)):   # and alone
            run_and_check(ix, searcher, [r], end + " alone")


@pytest.mark.parametrize("docset", [False, True])
def test_overflow_is_exactly_more_than_max_buckets(a, docset):
    """max_buckets = distinct, distinct - 1 and distinct + 1: overflow exactly at distinct - 1 -- alone, and as queries of a batch that
    mixes LONG and DOUBLE columns and whose other queries stay exact."""
    ix, searcher = a
    shape = dict(docset=True, filters=(5,)) if docset else dict(clauses=(1, 2, 3), need=2)
    reqs, expect = [], []
    for kind in ("long", "double"):
        for name in ("const", "two", "many"):
            n = ix.distinct(Req((kind, name), 1, **shape))
            assert n == {"const": 1, "two": 2}.get(name, n) and (name != "many" or n > 300)
            for b, over in ((n, 0), (n - 1, 1), (n + 1, 0)):
                if b >= 1:
                    reqs.append(Req((kind, name), b, **shape))
                    expect.append(over)
    for r, over in zip(reqs, expect):
        got = run_and_check(ix, searcher, [r], "alone")[0]
        assert int(got.overflowed) == over, cases.describe(r)
    order = np.random.default_rng(3).permutation(len(reqs)).tolist()   # kinds and outcomes interleaved
    got = run_and_check(ix, searcher, [reqs[i] for i in order], "batch")
    assert [int(g.overflowed) for g in got] == [expect[i] for i in order] and 0 < sum(expect) < len(expect)


# ---- index B: one item, more distinct values than the workgroup's table takes within its probe bound -----------------------------------
@pytest.fixture(scope="module")
def b(ctx):
    n = 13_000
    corpus = fs.make_corpus([n], {1: 0.6}, seed=8)
    perm = np.random.default_rng(9).permutation(n).astype(np.uint64)
    columns = {("long", "high"): [(None, (perm << np.uint64(32)) + np.uint64(5))], ("long", "low"): [(None, (np.uint64(5) << np.uint64(32)) + perm)]}
    ix = cases.Index(corpus, columns, {}, [None], [None])
    leaves, searcher = cases.upload(ctx, ix)
    yield ix, searcher
    release(leaves)


@pytest.mark.parametrize("name", ["high", "low"])
def test_more_distinct_values_than_the_workgroup_table_takes(b, name):
    """~7800 distinct values that differ in one half only: exact at max_buckets 8192 (values go straight to the query's table), and
    overflowed at 4, where the probe of the query's table runs its whole bound."""
    ix, searcher = b
    fit, tiny = Req(("long", name), 8192), Req(("long", name), 4)
    exp = ix.expected(fit)
    assert 7500 < exp[2] <= 8192 and exp[5] == 0 and exp[1].max() == 1
    got = run_and_check(ix, searcher, [fit], name)[0]
    assert api.GpuContext.last_diagnostics()["items_scan"] == 1 and set(got.counts.tolist()) == {1}
    got = run_and_check(ix, searcher, [tiny], name)[0]
    assert got.overflowed and got.hits_with_value == -1 and got.total_hits > 7500
    both = run_and_check(ix, searcher, [tiny, fit], name)
    assert [int(g.overflowed) for g in both] == [1, 0]
    both = run_and_check(ix, searcher, [dataclasses.replace(fit, docset=True, max_buckets=16384), dataclasses.replace(tiny, docset=True)], name)
    assert [int(g.overflowed) for g in both] == [0, 1] and len(both[0].counts) == 13_000


# ---- crafted collisions: a probe chain longer than the workgroup's bound, a full chain in the query's table --------------------------------
def test_crafted_collisions(ctx):
    """12 longs with ONE home slot in the workgroup's table -- more than its probe takes (9 would do): the last ones are handed to the
    query's table while the first eight arrive there with the flush -- and 6 with one home slot in a query's table of max_buckets 8
    (16 slots): a chain of 6.  A 1024-doc leaf whose hits hold exactly these values, with unequal multiplicities."""
    lds12, v = [], cases.EPOCH
    want = api.terms_home_slots64("long", cases.EPOCH, 16)[0]
    while len(lds12) < 12:
        if api.terms_home_slots64("long", v, 16)[0] == want:
            lds12.append(v)
        v += 1
    tab6, v = [], -5
    want = api.terms_home_slots64("long", (-5) & (2**64 - 1), 8)[1]
    while len(tab6) < 6:
        if api.terms_home_slots64("long", v & (2**64 - 1), 8)[1] == want:
            tab6.append(v)
        v += 2**33 + 1
    assert LDS_PROBE < len(lds12) and len(set(lds12)) == 12 and len(set(tab6)) == 6
    n = 1024
    corpus = fs.make_corpus([n], {1: 1.0}, seed=12)

    def spread(values):   # value j on about (j + 1) / sum of the docs
        w = np.arange(1, len(values) + 1, dtype=np.float64)
        return cases.u64(values)[np.random.default_rng(13).choice(len(values), size=n, p=w / w.sum())]

    columns = {("long", "lds12"): [(None, spread(lds12))], ("long", "tab6"): [(None, spread(tab6))]}
    ix = cases.Index(corpus, columns, {}, [None], [None])
    leaves, searcher = cases.upload(ctx, ix)
    try:
        for docset in (False, True):
            got = run_and_check(ix, searcher, [Req(("long", "lds12"), 16, docset=docset), Req(("long", "tab6"), 8, docset=docset),
                                               Req(("long", "lds12"), 12, docset=docset), Req(("long", "tab6"), 6, docset=docset),
                                               Req(("long", "lds12"), 11, docset=docset), Req(("long", "tab6"), 5, docset=docset)], "collisions")
            assert got[0].values.tolist() == sorted(lds12) and got[1].values.tolist() == sorted(tab6)
            assert len(set(got[0].counts.tolist())) > 6 and sum(got[0].counts.tolist()) == n == sum(got[1].counts.tolist())
            assert [int(g.overflowed) for g in got] == [0, 0, 0, 0, 1, 1]
    finally:
        release(leaves)


# ---- one query cut into several items: the counts of one value arrive from more than one workgroup -------------------------------------
def test_several_items_share_the_query_table(ctx):
    n = 300_000
    corpus = fs.make_corpus([n], {1: 1.0}, seed=10)
    mod5 = (np.arange(n) % 5).astype(np.int64)
    mod5[mod5 == 3] = f64.INT64_MIN          # one residue is the reserved code: its counter is shared by the items too
    columns = {("long", "mod5"): [(None, mod5.view(np.uint64))], ("long", "every"): [(None, np.arange(n, dtype=np.int64).view(np.uint64))]}
    ix = cases.Index(corpus, columns, {}, [None], [None])
    leaves, searcher = cases.upload(ctx, ix)
    try:
        for docset in (False, True):
            got = run_and_check(ix, searcher, [Req(("long", "mod5"), 16, docset=docset), Req(("long", "every"), 65536, docset=docset)], "items")
            assert api.GpuContext.last_diagnostics()["items_scan"] >= 4
            assert got[0].counts.tolist() == [n // 5] * 5 and got[0].total_hits == n and got[0].values[0] == f64.INT64_MIN
            assert got[1].overflowed and got[1].total_hits == n      # 300 000 distinct values under the largest bound
    finally:
        release(leaves)


# ---- sub-tile edges ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025])
def test_sub_tile_edges(ctx, n):
    """Single leaves around the 64-doc word and the 1024-doc sub-tile; the column on every doc (no `has` words) or on all but the last.
    The first and the last doc hold Long.MIN_VALUE, whose code is what the column's padding reads as: a padded slot that counted
    would show in its bucket."""
    corpus = fs.make_corpus([n], {1: 1.0, 2: 0.5}, seed=40 + n)
    columns = {}
    for kind in ("long", "double"):
        pool = cases.POOLS[(kind, "edge")]
        full = pool[np.arange(n) % len(pool)].copy()
        if kind == "long":
            full[0] = full[-1] = cases.u64([f64.INT64_MIN])[0]
        columns[(kind, "full")] = [(None, full)]
        columns[(kind, "nolast")] = [(np.arange(n - 1, dtype=np.int32), full[: n - 1])]
    ix = cases.Index(corpus, columns, {}, [None], [None])
    leaves, searcher = cases.upload(ctx, ix)
    try:
        for docset in (False, True):
            reqs = [Req(key, 16, docset=docset, clauses=c) for key in columns for c in ((1,), (2,))[: 1 if docset or n == 1 else 2]]
            got = run_and_check(ix, searcher, reqs, f"{n} docs")
            assert got[0].total_hits == n and got[0].hits_with_value == n
            nolast = [g for r, g in zip(reqs, got) if r.column[1] == "nolast" and r.clauses == (1,)]
            assert all(g.total_hits == n and g.hits_with_value == n - 1 for g in nolast)
    finally:
        release(leaves)


# ---- the two widths meet, the refusals ----------------------------------------------------------------------------------------------------
def _raw(searcher, ix, r, field=None, capacity=None, null_arrays=False, mgr=None):
    """the batch entry's status and reason for one request; the predicate must agree (it has no output to judge)"""
    L = _lib.load()
    col = api.TermsCollector(ix.field[r.column] if field is None else field, 10, True, r.column[0])
    cap = max(r.max_buckets, 1) if capacity is None else capacity
    bits, counts = np.zeros(max(cap, 1), np.uint64), np.zeros(max(cap, 1), np.int32)
    out = _lib.TermCounts64()
    out.capacity = cap
    if not null_arrays:
        out.value_bits = C.cast(bits.ctypes.data, C.POINTER(C.c_uint64))
        out.counts = C.cast(counts.ctypes.data, C.POINTER(C.c_int32))
    h, segs, bases, nl = searcher.ctx._h, searcher._segs, searcher._bases, len(searcher.leaves)
    if r.docset:
        tc, _ = api._terms64([col], r.max_buckets, 1)
        ds, keep = api._marshal_docsets([cases.query_of(r)], [mgr or api.TopScoreDocCollectorManager(1)])
        rc = L.nrtgpu_count_docset_terms64_batch(h, segs, bases, nl, ds, tc, 1, C.byref(out))
        text = L.nrtgpu_last_error().decode()
        rc2 = L.nrtgpu_count_docset_terms64_supported(h, segs, nl, ds, tc)
        del keep
    else:
        m, tc, _ = api._marshal_terms64(searcher, [cases.query_of(r)], [col], r.max_buckets, None if mgr is None else [mgr])
        rc = L.nrtgpu_count_terms64_batch(h, segs, bases, nl, m.queries, tc, 1, C.byref(out))
        text = L.nrtgpu_last_error().decode()
        rc2 = L.nrtgpu_count_terms64_supported(h, segs, nl, m.queries, tc)
    if capacity is None and not null_arrays:
        assert rc2 == rc, f"the predicate ({rc2}) and the call ({rc}) disagree: {text}"
    return rc, text


@pytest.mark.parametrize("docset", [False, True])
def test_refusals(a, docset):
    ix, searcher = a
    shape = dict(docset=True) if docset else dict(clauses=(1, 2, 3))
    entry32 = "nrtgpu_count_docset_terms_batch" if docset else "nrtgpu_count_terms_batch"
    r = Req(("long", "two"), 16, **shape)
    for name, code, kw, rr, says in (
            ("an int column", UNS, dict(field=cases.R_SINGLE_FIELD), r, entry32),
            ("a multi-valued column", UNS, dict(field=cases.R_MULTI_FIELD), r, entry32),
            ("a multi-valued column is called one", UNS, dict(field=cases.R_MULTI_FIELD), r, "multi-valued"),
            ("resident on no leaf", UNS, dict(field=55), r, "55"),
            ("kinds differ", INV, dict(field=40), r, "kinds"),
            ("max_buckets 0", INV, {}, dataclasses.replace(r, max_buckets=0), "max_buckets"),
            ("max_buckets 65537", INV, {}, dataclasses.replace(r, max_buckets=65537), "max_buckets"),
            ("max_buckets 0 over no column", INV, dict(field=55), dataclasses.replace(r, max_buckets=0), "max_buckets"),
            ("capacity below max_buckets", INV, dict(capacity=15), r, "capacity"),
            ("NULL output arrays", INV, dict(null_arrays=True), r, "NULL"),
            ("numHits 0", INV, dict(mgr=api.TopScoreDocCollectorManager(0)), r, ""),
            ("a mask that is not resident", UNS, {}, dataclasses.replace(r, filters=(77,)), "77")):
        rc, text = _raw(searcher, ix, rr, **kw)
        assert rc == code and says in text and "query 0" in text, (name, rc, text)
    # INVALID_ARG of a later query comes before UNSUPPORTED of an earlier one
    fn = api.count_docset_terms64_batch if docset else api.count_terms64_batch
    q = cases.query_of(r)
    with pytest.raises(_lib.NrtGpuError) as e:
        fn(searcher, [q, q], [api.TermsCollector(cases.R_SINGLE_FIELD, 10, True, "long"), ix.collector(r)], [16, 0])
    assert e.value.code == INV and "query 1" in str(e.value)
    with pytest.raises(_lib.NrtGpuError) as e:
        fn(searcher, [q, q], [ix.collector(r), api.TermsCollector(cases.R_SINGLE_FIELD, 10, True, "long")], [16, 16])
    assert e.value.code == UNS and "query 1" in str(e.value) and entry32 in str(e.value)
    with pytest.raises(api.UnsupportedQuery):
        fn(searcher, [q], [api.TermsCollector(ix.field[r.column], 10, True, "int")], 16)
    # the 32-bit entries over a 64-bit column keep refusing, and now name the entry that builds the buckets
    fn32 = api.count_docset_terms_batch if docset else api.count_terms_batch
    with pytest.raises(_lib.NrtGpuError) as e:
        fn32(searcher, [q], [api.TermsCollector(ix.field[r.column], 10)], 16)
    assert e.value.code == UNS and "64-bit buckets are not built" in str(e.value) and entry32.replace("terms_", "terms64_") in str(e.value)
    # NULL arguments with a context
    L, t, o = _lib.load(), _lib.TermsCount(), _lib.TermCounts64()
    h, segs, bases = searcher.ctx._h, searcher._segs, searcher._bases
    batch, pred = (L.nrtgpu_count_docset_terms64_batch, L.nrtgpu_count_docset_terms64_supported) if docset else (L.nrtgpu_count_terms64_batch, L.nrtgpu_count_terms64_supported)
    one = C.byref(_lib.DocsetQuery()) if docset else C.byref(_lib.Bm25Query())
    assert batch(h, segs, bases, 3, None, C.byref(t), 1, C.byref(o)) == INV
    assert batch(h, segs, bases, 3, one, None, 1, C.byref(o)) == INV
    assert batch(h, segs, bases, 3, one, C.byref(t), 1, None) == INV
    assert pred(h, segs, 3, None, C.byref(t)) == INV and pred(h, segs, 3, one, None) == INV
    # and the route still answers
    run_and_check(ix, searcher, [r], "after the refusals")


def test_the_workspace_bound(ctx):
    """A table slot is 12 bytes: 171 tables of 2^17 slots exceed the call's 22 369 621; 170 fit and run."""
    corpus = fs.make_corpus([200], {1: 0.5}, seed=13)
    values = cases.u64([cases.EPOCH + (i % 3) * 2**33 for i in range(200)])
    ix = cases.Index(corpus, {("long", "three"): [(None, values)]}, {}, [None], [None])
    leaves, searcher = cases.upload(ctx, ix)
    try:
        r = Req(("long", "three"), 65536)
        assert _lib.NRTGPU_TERMS64_MAX_CALL_SLOTS == 22369621 and 170 * 2**17 <= 22369621 < 171 * 2**17
        for rr in (r, dataclasses.replace(r, docset=True)):
            with pytest.raises(_lib.NrtGpuError) as e:
                cases.run(searcher, ix, [rr] * 171)
            assert e.value.code == INV and "22369621" in str(e.value) and "query 170" in str(e.value)
            assert cases.supported(searcher, ix, rr) is True   # (the bound is the call's, not the query's)
        got = cases.run(searcher, ix, [r] * 170)
        for g in got[:: 34]:
            cases.check("170 tables of 2^17 slots", "long", g, ix.expected(r))
    finally:
        release(leaves)


@pytest.mark.parametrize("flag", [_lib.NRTGPU_FLAG_PACKED_POSTINGS, _lib.NRTGPU_FLAG_NO_FIXED_POINT])
def test_contexts_the_text_form_refuses_and_the_doc_set_form_runs_under(flag):
    corpus = fs.make_corpus([700, 300], {1: 0.5}, seed=14, delete_fraction=0.1)
    rng = np.random.default_rng(15)
    columns = {("long", "edge"): [(None, rng.choice(cases.LONG_EDGE, size=700)), None], ("double", "edge"): [(None, rng.choice(cases.POOLS[("double", "edge")], size=700)), None]}
    ix = cases.Index(corpus, columns, {}, [None, None], [None, None])
    c = api.GpuContext(device_id=0, max_batch=16, flags=flag)
    leaves = []
    try:
        leaves, searcher = cases.upload(c, ix)
        for key in columns:
            r = Req(key, 16)
            assert cases.supported(searcher, ix, r) is False
            with pytest.raises(_lib.NrtGpuError) as e:
                cases.run(searcher, ix, [r])
            assert e.value.code == UNS
            assert cases.supported(searcher, ix, dataclasses.replace(r, docset=True)) is True
        run_and_check(ix, searcher, [Req(key, 16, docset=True) for key in columns], "under the flag")
    finally:
        release(leaves)
        c.close()


# ---- the seeded fuzz -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("round_", range(FUZZ_ROUNDS))
def test_fuzz(round_):
    """tests/_terms_count64_cases.py: fuzz_round; tests/test_terms_count64_host.py checks that every round holds an overflowed query,
    an exact one with two buckets and a hit without a value.  The generator draws supported shapes only: none is skipped.  A
    failure names round, batch and index: cases.fuzz_round(FUZZ_BASE, round_)[1][batch][index] is the case."""
    ix, batches = cases.fuzz_round(FUZZ_BASE, round_)
    c = api.GpuContext(device_id=0, max_batch=16, target_items=ix.target_items)
    leaves = []
    try:
        if ix.slicing is not None:
            c.set_slicing(*ix.slicing)
        leaves, searcher = cases.upload(c, ix)
        for bi, reqs in enumerate(batches):
            for r in reqs[:: 5]:
                assert cases.supported(searcher, ix, r) is True, cases.describe(r)
            run_and_check(ix, searcher, reqs, f"round {round_} (leaves {ix.sizes}, slicing {ix.slicing}, target_items {ix.target_items}) batch {bi}")
    finally:
        release(leaves)
        c.close()
