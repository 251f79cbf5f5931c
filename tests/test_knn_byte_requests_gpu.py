"""knn requests over a BYTE (int8) vector field with a k, boost, pre-filter and threshold EACH that share a pass over the rows
(nrtgpu_knn_search_bytes_requests, nrtgpu_knn_search_bytes_coalesced, nrtgpu_knn_exact_bytes_coalesced) against the
numpy brute force of tests/_byte_knn_ref.py: exact integers, the header's table with one fp32 rounding per operation, * float32(boost),
sorted by (score desc, doc asc).  Docids and score BITS, no tolerance: a member of a mixed panel gets what nrtgpu_knn_search_bytes
gives it alone.  int8 rows make tied scores common, so the docid order among ties is checked by the same assertions.  Thresholds come
from the reference's own list for that query under that filter (its 60th score), so the cut falls inside the top 100 -- often on a
tie -- and is decided on result bits."""
import functools
import threading
import time

import numpy as np
import pytest

from nrtsearch_amd import _lib, api
from tests._byte_knn_ref import (KINDS, M1, M7, M25, M25B, M0, SIMS, Leaf, check_hits, expected, mixed_index, mixed_requests,
                                 reference_lists, threshold_of)

pytestmark = pytest.mark.gpu
FIELD = 3


def _filters(kinds):
    return [api.MaskFilter(kd) if kd is not None else None for kd in kinds]


@functools.lru_cache(maxsize=None)
def _index(dim):
    return mixed_index(dim)


@pytest.fixture(scope="module")
def searchers():
    """dim -> (context, searcher over mixed_index(dim)); one context, every index uploaded once."""
    made = {}
    ctx = api.GpuContext(device_id=0, max_batch=64)

    def get(dim):
        if dim not in made:
            gl = [lf.upload(ctx, FIELD, api) for lf in _index(dim)[0]]
            made[dim] = (api.GpuIndexSearcher(ctx, gl, api.IndexStatistics()), gl)
        return ctx, made[dim][0]

    yield get
    for _, gl in made.values():
        for g in gl:
            g.release()
    ctx.close()


_REFS = {}


def mixed_reference(dim, sim_name):
    """The 70 requests of the mixed panel and their reference lists: computed once per (dim, similarity) and left unchanged."""
    if (dim, sim_name) not in _REFS:
        leaves, queries = _index(dim)
        kinds, ks, boosts, thr_kinds = mixed_requests(len(queries))
        full = reference_lists(sim_name, queries, leaves, kinds)
        mins = [threshold_of(full[q], thr_kinds[q]) for q in range(len(queries))]
        _REFS[(dim, sim_name)] = (kinds, ks, boosts, mins, full)
    return _REFS[(dim, sim_name)]


@pytest.mark.parametrize("sim_name", list(SIMS))
@pytest.mark.parametrize("dim", [24, 100, 320])
def test_mixed_panel_matches_the_brute_force(searchers, dim, sim_name):
    """70 requests = a pass of 64 (four panels of 16: P = 4) and a pass of 6 (P = 1); every filter kind, k, boost and threshold kind
    inside each 16-query panel of the 64.  dim 24 / 100 / 320: one padded step, two steps, five steps -- ring depths 1, 2 and 5."""
    ctx, sr = searchers(dim)
    leaves, queries = _index(dim)
    kinds, ks, boosts, mins, full = mixed_reference(dim, sim_name)
    ctx.reset_stats()
    got = sr.knn_search_bytes_requests(FIELD, sim_name, queries, ks, boosts, _filters(kinds), mins)
    st = ctx.stats()
    assert st["knn_panels"] == 2 and st["knn_sketch_launches"] == 0 and st["knn_second_passes"] == 0, st
    assert st["knn_rows"] == 2 * (4000 + 2500 + 900), st
    n_empty = 0
    for q in range(len(queries)):
        exp = expected(full[q], ks[q], boosts[q], mins[q])
        check_hits(got[q], exp, (q, kinds[q], ks[q], boosts[q], mins[q]))
        n_empty += not exp
        if kinds[q] is not None:
            for d in got[q].docs.tolist():
                lf = max((l for l in leaves if l.base <= d), key=lambda l: l.base)
                assert lf.masks[kinds[q]][d - lf.base], (q, d)
    assert 0 < n_empty < len(queries)


def test_a_member_gets_what_knn_search_bytes_gives_it_alone(searchers):
    """The contract itself, on a few members of the mixed panel: the same docids, score bits and total_hits as the single call."""
    ctx, sr = searchers(100)
    _, queries = _index(100)
    kinds, ks, boosts, mins, _ = mixed_reference(100, "cosine")
    got = sr.knn_search_bytes_requests(FIELD, "cosine", queries[:20], ks[:20], boosts[:20], _filters(kinds[:20]), mins[:20])
    for q in range(20):
        (want,) = sr.knn_search_bytes(FIELD, "cosine", queries[q], ks[q], boost=boosts[q],
                                      filter=api.MaskFilter(kinds[q]) if kinds[q] is not None else None, min_score=mins[q])
        assert got[q].docs.tolist() == want.docs.tolist() and got[q].total_hits == want.total_hits, q
        assert got[q].scores.view(np.uint32).tolist() == want.scores.view(np.uint32).tolist(), q


def test_equal_requests_take_knn_search_bytes_own_path():
    """All requests equal: nrtgpu_knn_search_bytes' bits and its route -- with the gather knob open and the 1 % filter knn_rows counts
    the accepted rows only; two different filters under the same setting pass over all 7400 rows."""
    leaves, queries = _index(100)
    ctx = api.GpuContext(device_id=0, max_batch=64)
    gl = [lf.upload(ctx, FIELD, api) for lf in leaves]
    try:
        sr = api.GpuIndexSearcher(ctx, gl, api.IndexStatistics())
        qs, n = queries[:5], 5
        full = reference_lists("cosine", qs, leaves, [M1] * n)
        thr = float(full[0][len(full[0]) // 2][0])
        n_accepted = sum(int(lf.accept_rows(M1).sum()) for lf in leaves if lf.rows is not None)
        assert 0 < n_accepted < 200
        for gather in (0, 1000):
            ctx.set_knn_gather(gather)
            ctx.reset_stats()
            want = sr.knn_search_bytes(FIELD, "cosine", qs, 10, boost=2.0, filter=api.MaskFilter(M1), min_score=thr)
            st_want = ctx.stats()
            ctx.reset_stats()
            got = sr.knn_search_bytes_requests(FIELD, "cosine", qs, [10] * n, [2.0] * n, [api.MaskFilter(M1)] * n, [thr] * n)
            st = ctx.stats()
            assert st["knn_panels"] == 1 and st["knn_rows"] == (n_accepted if gather else 7400), (gather, st)
            assert [st[c] for c in ("knn_panels", "knn_rows", "knn_score_launches")] == \
                [st_want[c] for c in ("knn_panels", "knn_rows", "knn_score_launches")], (gather, st, st_want)
            for q in range(n):
                assert got[q].docs.tolist() == want[q].docs.tolist() and got[q].total_hits == want[q].total_hits
                assert got[q].scores.view(np.uint32).tolist() == want[q].scores.view(np.uint32).tolist()
                check_hits(got[q], expected(full[q], 10, 2.0, thr), (gather, q))
        # (the knob is still open) two filters in one pass: all rows are passed over
        kinds = [M1, M7, M1, M7, M1]
        full2 = reference_lists("cosine", qs, leaves, kinds)
        ctx.reset_stats()
        got = sr.knn_search_bytes_requests(FIELD, "cosine", qs, [10] * n, None, _filters(kinds), None)
        st = ctx.stats()
        assert st["knn_panels"] == 1 and st["knn_rows"] == 4000 + 2500 + 900, st
        for q in range(n):
            check_hits(got[q], expected(full2[q], 10, 1.0, 0.0), q)
    finally:
        for g in gl:
            g.release()
        ctx.close()


def test_a_member_without_a_theta_next_to_members_with_one():
    """One member's filter accepts 40 rows (< k) among the first 70 000 and 5 000 further on: its theta stays unknown through the first
    round while the others' tighten, so it keeps a slot per row in the long round next to queries that only append what beats their
    theta.  The second leaf's long round (400 000 rows) exceeds a candidate list (2^18): the overflow is flagged and the WHOLE panel
    is redone in bounded rounds -- all 40 answers must be exact."""
    rng = np.random.default_rng(77)
    dim, k, nq, sel = 16, 64, 40, 17
    n0, n1 = 300_000, 400_000
    l0 = Leaf(0, n0, rng.integers(-128, 128, size=(n0, dim), dtype=np.int8))
    l1 = Leaf(n0, n1, rng.integers(-128, 128, size=(n1, dim), dtype=np.int8))
    m0 = np.zeros(n0, bool)
    m0[5:45] = True                                                        # 40 rows < k among the first 70 000 ...
    m0[rng.choice(np.arange(70_000, n0), size=2000, replace=False)] = True    # ... and 5 000 further on, over both leaves
    m1 = np.zeros(n1, bool)
    m1[rng.choice(n1, size=3000, replace=False)] = True
    l0.masks[M1], l1.masks[M1] = m0, m1
    queries = rng.integers(-128, 128, size=(nq, dim), dtype=np.int8)
    kinds = [M1 if q == sel else None for q in range(nq)]
    full = reference_lists("max_inner_product", queries, [l0, l1], kinds, depth=k)
    ctx = api.GpuContext(device_id=0, max_batch=64)
    gl = [l0.upload(ctx, FIELD, api), l1.upload(ctx, FIELD, api)]
    try:
        sr = api.GpuIndexSearcher(ctx, gl, api.IndexStatistics())
        got = sr.knn_search_bytes_requests(FIELD, "max_inner_product", queries, [k] * nq, None, _filters(kinds), None)
        for q in range(nq):
            check_hits(got[q], expected(full[q], k, 1.0, 0.0), q)
        assert len(got[sel].docs) == k and all((m0[d] if d < n0 else m1[d - n0]) for d in got[sel].docs.tolist())
    finally:
        for g in gl:
            g.release()
        ctx.close()


def test_a_full_workgroup_queue_writes_rows_through_the_members_own_accept_set():
    """The straight-to-list branch of a FULL workgroup queue must read the member's own accept set.

    launch_knn_bytes' arithmetic (knn_bytes.hip) at dim 16 with more than 16 members: one step, four panels, so the panel takes
    1 x 4 x 1024 = 4096 bytes and the queue behind it min(4096, (160 KiB - 1536 - 4096 - 16) / 8) = 4096 entries per workgroup.
    The rounds (KnnRun::tile_rounds): the first is 65 536 rows, every row in a slot; the second is min(15 x 65 536, the rest).
    With N = 65 536 + 262 144 rows the second round is 262 144 rows on min(262 144 / 256, CUs) workgroups: on the 256 CUs of an
    MI355X 1024 rows each (more with fewer CUs; 863 with 304).  The rows are in rising order of their score for the one query vector
    all members share (max_inner_product with a vector of ones: the score is the row's sum + 1, in plateaus of about 80 rows), so
    after the first round every accepted row of a later plateau beats theta: with 24 members and a 50 % filter each a workgroup
    queues about 1024 x 24 x 0.5 = 12 288 entries -- three times its queue.  What does not fit goes straight to the member's list,
    about 131 072 keys per member: below a list's 2^18, so nothing is redone.  Every member has its OWN random 50 % mask: a row
    tested against another member's set, or the leaf's liveDocs, would put foreign docs into the top k."""
    rng = np.random.default_rng(9)
    dim, k, members, n = 16, 10, 24, 65_536 + 262_144
    sums = -2048 + (np.arange(n, dtype=np.int64) * 4080) // n           # non-decreasing, within what 16 int8 can sum to
    rows = (sums // dim)[:, None] + (np.arange(dim)[None, :] < (sums % dim)[:, None])
    assert rows.min() >= -128 and rows.max() <= 127 and (rows.sum(1) == sums).all()
    lf = Leaf(0, n, rows.astype(np.int8))
    for m in range(members):
        lf.masks[100 + m] = rng.random(n) < 0.5
    queries = np.ones((members, dim), np.int8)
    kinds = [100 + m for m in range(members)]
    full = reference_lists("max_inner_product", queries, [lf], kinds, depth=k)
    assert len({tuple(d for _, d in full[m]) for m in range(members)}) > members // 2   # the members' answers differ
    ctx = api.GpuContext(device_id=0, max_batch=64, collect_timing=True)   # (timing: the statistics count the scoring launches)
    g = lf.upload(ctx, FIELD, api)
    try:
        sr = api.GpuIndexSearcher(ctx, [g], api.IndexStatistics())
        ctx.reset_stats()
        got = sr.knn_search_bytes_requests(FIELD, "max_inner_product", queries, [k] * members, None, _filters(kinds), None)
        st = ctx.stats()
        assert st["knn_panels"] == 1 and st["knn_score_launches"] == 2 and st["knn_rows"] == n, st   # two rounds, nothing redone
        for m in range(members):
            check_hits(got[m], expected(full[m], k, 1.0, 0.0), m)
            assert all(lf.masks[kinds[m]][d] for d in got[m].docs.tolist())
    finally:
        g.release()
        ctx.close()


def _park(ctx, which, threads, done, want_pending=None):
    """Start `threads`; wait until coalescer `which` reports want_pending parked callers (None: until all have returned -- a held
    leader leaves by itself once a whole panel of 64 waits)."""
    for t in threads:
        t.start()
    t_end = time.monotonic() + 60.0
    while time.monotonic() < t_end:
        if want_pending is not None and ctx.debug_coalescer_pending(which) >= want_pending:
            return True
        if want_pending is None and done() >= len(threads):
            return True
        time.sleep(0.001)
    return False


def test_coalesced_callers_with_their_own_filters_share_one_panel(dev_lib):
    """nrtgpu_knn_search_bytes_coalesced: 64 callers parked behind nrtgpu_debug_hold_coalescers, each with its own query, one of 6
    filters, its own k, boost and threshold, leave as ONE panel and each gets the brute force's bits; a caller whose deadline
    expires while parked is told NRTGPU_ERR_TIMEOUT and its mate is answered.  nrtgpu_knn_exact_bytes_coalesced: 64 callers, one
    boost, mixed k, one panel.  A float-entry caller and a byte-entry caller parked together never share a panel."""
    rng = np.random.default_rng(616)
    dim, n, n_callers = 64, 20_000, 64
    lf = Leaf(0, n, rng.integers(-128, 128, size=(n, dim), dtype=np.int8), live=rng.random(n) > 0.05)
    lf.masks = {M25: rng.random(n) < 0.25, M1: rng.random(n) < 0.01, M7: np.zeros(n, bool), M0: np.zeros(n, bool), M25B: rng.random(n) < 0.25}
    lf.masks[M7][rng.choice(np.flatnonzero(lf.live), size=7, replace=False)] = True
    queries = rng.integers(-128, 128, size=(n_callers, dim), dtype=np.int8)
    kinds = [KINDS[q % 6] for q in range(n_callers)]
    ks = [int(x) for x in rng.choice([1, 10, 37, 100], size=n_callers)]
    boosts = [float(x) for x in rng.choice([0.5, 1.0, 2.0], size=n_callers)]
    full = reference_lists("cosine", queries, [lf], kinds)
    mins = [threshold_of(full[q], q % 3) for q in range(n_callers)]
    full_exact = reference_lists("l2_norm", queries, [lf], [None] * n_callers)
    n_live = int(lf.live.sum())
    c = api.GpuContext(device_id=0, max_batch=64)
    g = lf.upload(c, FIELD, api)
    gf = api.GpuSegment(c, 64, 0)   # a float field, for the float entry's caller
    gf.add_vectors(FIELD, np.ones((64, 16), np.float32))
    gf.seal()
    sr = api.GpuIndexSearcher(c, [g], api.IndexStatistics())
    srf = api.GpuIndexSearcher(c, [gf], api.IndexStatistics())
    results, errors = {}, {}

    def call(i):
        return sr.knn_search_bytes_coalesced(FIELD, "cosine", queries[i], ks[i], boost=boosts[i],
                                             filter=api.MaskFilter(kinds[i]) if kinds[i] is not None else None, min_score=mins[i])

    def caller(i, rep, deadline=None, fn=call):
        try:
            if deadline is not None:
                api.GpuContext.set_thread_deadline(deadline)
            results[(i, rep)] = fn(i)
        except api.NrtGpuError as e:
            errors[(i, rep)] = e

    def check(i, rep):
        check_hits(results[(i, rep)], expected(full[i], ks[i], boosts[i], mins[i]), (i, rep, kinds[i], ks[i], boosts[i], mins[i]))

    try:
        check_hits(call(1), expected(full[1], ks[1], boosts[1], mins[1]), "a lone caller runs at once")
        # 64 callers, 6 filters: one panel
        c.reset_stats()
        c.debug_hold_coalescers(True)
        try:
            ok = _park(c, 3, [threading.Thread(target=caller, args=(i, 0)) for i in range(n_callers)], lambda: len(results) + len(errors))
        finally:
            c.debug_hold_coalescers(False)
        assert ok and not errors, errors
        st = c.stats()
        assert st["knn_panels"] == 1 and st["knn_sketch_launches"] == 0 and st["knn_second_passes"] == 0, st
        for i in range(n_callers):
            check(i, 0)
        # requests that cannot be answered fail alone, at once, while another waits; a caller whose deadline passes in the queue
        # (behind a leader that is held): TIMEOUT for it alone
        results.clear()
        c.debug_hold_coalescers(True)
        try:
            leader = threading.Thread(target=caller, args=(0, 1))
            assert _park(c, 3, [leader], None, want_pending=1)
            for bad, code, says in ((lambda: sr.knn_search_bytes_coalesced(FIELD, "cosine", queries[0], 10, filter=api.MaskFilter(77)), _lib.NRTGPU_ERR_UNSUPPORTED, "query 0:"),
                                    (lambda: sr.knn_search_bytes_coalesced(FIELD, "cosine", np.ones(24, np.int8), 10), _lib.NRTGPU_ERR_INVALID_ARG, "dimension"),
                                    (lambda: sr.knn_search_bytes_coalesced(FIELD, "cosine", np.zeros(dim, np.int8), 10), _lib.NRTGPU_ERR_INVALID_ARG, "query 0:"),
                                    (lambda: sr.knn_search_bytes_coalesced(FIELD, "cosine", queries[0], 0), _lib.NRTGPU_ERR_INVALID_ARG, "query 0:"),
                                    (lambda: sr.knn_exact_bytes_coalesced(FIELD, "cosine", np.zeros(dim, np.int8), 10), _lib.NRTGPU_ERR_INVALID_ARG, "query 0:")):
                with pytest.raises(api.NrtGpuError) as e:
                    bad()
                assert e.value.code == code and says in str(e.value), e.value
            assert c.debug_coalescer_pending(3) == 1
            late = threading.Thread(target=caller, args=(2, 1, 0.02))
            assert _park(c, 3, [late], None, want_pending=2)
            time.sleep(0.03)
        finally:
            c.debug_hold_coalescers(False)
        leader.join()
        late.join()
        check(0, 1)
        assert errors[(2, 1)].code == _lib.NRTGPU_ERR_TIMEOUT and "waited for a panel" in str(errors[(2, 1)]), errors
        errors.clear()
        # the exact entry: 64 callers, one boost, mixed k -- one panel, every caller the first k of its own
        results.clear()
        c.reset_stats()
        c.debug_hold_coalescers(True)
        try:
            exact = lambda i: sr.knn_exact_bytes_coalesced(FIELD, "l2_norm", queries[i], ks[i], boost=2.0)   # noqa: E731
            ok = _park(c, 4, [threading.Thread(target=caller, args=(i, 2, None, exact)) for i in range(n_callers)], lambda: len(results) + len(errors))
        finally:
            c.debug_hold_coalescers(False)
        assert ok and not errors, errors
        assert c.stats()["knn_panels"] == 1, c.stats()
        for i in range(n_callers):
            r, exp = results[(i, 2)], expected(full_exact[i], ks[i], 2.0, 0.0)
            assert r.docs.tolist() == [d for _, d in exp] and r.total_hits == n_live, i
            assert r.scores.view(np.uint32).tolist() == np.array([s for s, _ in exp], np.float32).view(np.uint32).tolist(), i
        # a float-entry caller and a byte-entry caller parked together: two queues, two panels
        results.clear()
        c.reset_stats()
        c.debug_hold_coalescers(True)
        try:
            fl = threading.Thread(target=caller, args=(0, 3, None, lambda i: srf.knn_search_coalesced(FIELD, "l2_norm", np.ones(16, np.float32), 5)))
            by = threading.Thread(target=caller, args=(1, 3))
            assert _park(c, 2, [fl], None, want_pending=1) and _park(c, 3, [by], None, want_pending=1)
            assert [c.debug_coalescer_pending(w) for w in (0, 1, 2, 3, 4)] == [0, 0, 1, 1, 0]
        finally:
            c.debug_hold_coalescers(False)
        fl.join()
        by.join()
        assert not errors, errors
        assert c.stats()["knn_panels"] == 2, c.stats()
        check(1, 3)
        assert len(results[(0, 3)].docs) == 5
        assert [c.debug_coalescer_pending(w) for w in (0, 1, 2, 3, 4)] == [0, 0, 0, 0, 0]
    finally:
        c.debug_hold_coalescers(False)
        g.release()
        gf.release()
        c.close()


def test_a_bad_request_refuses_the_whole_call_and_names_itself(searchers):
    ctx, sr = searchers(100)
    _, queries = _index(100)
    qs, n = queries[:4], 4
    ctx.reset_stats()
    inv, uns = _lib.NRTGPU_ERR_INVALID_ARG, _lib.NRTGPU_ERR_UNSUPPORTED

    def refused(code, names, queries=qs, sim="cosine", **kw):
        args = dict(ks=[10] * n, boosts=None, filters=None, min_scores=None)
        args.update(kw)
        with pytest.raises(api.NrtGpuError) as e:
            sr.knn_search_bytes_requests(FIELD, sim, queries, args["ks"], args["boosts"], args["filters"], args["min_scores"])
        assert e.value.code == code, (kw, e.value)
        if names is not None:
            assert f"query {names}:" in str(e.value), (kw, e.value)

    refused(inv, 2, ks=[10, 10, 0, 10])
    refused(inv, 3, ks=[10, 10, 10, -5])
    refused(uns, 1, ks=[10, _lib.NRTGPU_MAX_K + 1, 10, 10])
    refused(inv, 0, min_scores=[-0.5, 0, 0, 0])
    refused(inv, 3, min_scores=[0, 0, 0, float("nan")])
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        refused(inv, 1, boosts=[1.0, bad, 1.0, 1.0])
    refused(uns, 2, filters=[None, api.MaskFilter(M25), api.MaskFilter(77), None])
    zero = qs.copy()
    zero[2] = 0
    refused(inv, 2, queries=zero)                      # a zero query under cosine
    refused(inv, None, queries=np.ones((n, 24), np.int8))   # a dimension other than the field's
    L = _lib.load()
    outs, _, _ = api._topdocs_outputs(n, 10)
    ks = np.full(n, 10, np.int32)
    neg = np.array([0, M25, 0, -3], np.int32)
    call = lambda dim, ks_p, masks_p: L.nrtgpu_knn_search_bytes_requests(ctx._h, sr._segs, sr._bases, len(sr.leaves), FIELD, 0, qs.ctypes.data,  # noqa: E731
                                                                          n, dim, ks_p, None, masks_p, None, outs)
    assert call(100, ks.ctypes.data, neg.ctypes.data) == inv and b"query 3:" in L.nrtgpu_last_error()
    assert call(100, None, None) == inv            # ks == NULL
    assert call(4096, ks.ctypes.data, None) == uns
    # a float field: refused, and the error names the element type
    gf = api.GpuSegment(ctx, 64, 0)
    gf.add_vectors(FIELD, np.ones((64, 16), np.float32))
    gf.seal()
    try:
        srf = api.GpuIndexSearcher(ctx, [gf], api.IndexStatistics())
        for bad in (lambda: srf.knn_search_bytes_requests(FIELD, "cosine", np.ones((2, 16), np.int8), [3, 4]),
                    lambda: srf.knn_search_bytes_coalesced(FIELD, "cosine", np.ones(16, np.int8), 3),
                    lambda: srf.knn_exact_bytes_coalesced(FIELD, "cosine", np.ones(16, np.int8), 3)):
            with pytest.raises(api.NrtGpuError) as e:
                bad()
            assert e.value.code == inv and "float" in str(e.value), e.value
    finally:
        gf.release()
    assert ctx.stats()["knn_panels"] == 0          # nothing was launched
    assert len(sr.knn_search_bytes_requests(FIELD, "l2_norm", zero, [10, 10, 10, 7])[2].docs) == 10   # (a zero query is refused under cosine only)
    # NULL boosts / filters / thresholds: all 1, none, none
    want = sr.knn_search_bytes(FIELD, "cosine", qs, 10)
    got = sr.knn_search_bytes_requests(FIELD, "cosine", qs, [10, 10, 10, 7])
    for q in range(n):
        kq = 7 if q == 3 else 10
        assert got[q].docs.tolist() == want[q].docs.tolist()[:kq]
        assert got[q].scores.view(np.uint32).tolist() == want[q].scores.view(np.uint32).tolist()[:kq]
