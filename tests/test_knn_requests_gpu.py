"""knn requests with a k, boost, pre-filter and threshold EACH that share a pass over the rows (nrtgpu_knn_search_requests,
nrtgpu_knn_search_coalesced) against the CPU oracle: oracle.knn_exact with the request's accept set (liveDocs & its
mask) as live_words per leaf, the leaves' lists merged by (score desc, doc asc).  Docids and score BITS, no tolerance: a member of
a mixed panel gets what nrtgpu_knn_search gives it alone.  Thresholds come from the reference's own list for that query under that
filter (its 60th score), so the cut falls inside the top 100 and is decided on result bits."""
import functools
import threading
import time

import numpy as np
import pytest

from nrtsearch_amd import _lib, api

pytestmark = pytest.mark.gpu
FIELD = 3
SIMS = {"cosine": 0, "dot_product": 1, "l2_norm": 2, "max_inner_product": 3}
# mask ids per leaf: 25 %, 1 %, one that accepts 7 rows in total, an empty one, a second 25 %; None = no filter
M25, M1, M7, M0, M25B = 3, 4, 5, 6, 7
KINDS = (M25, M1, M7, M0, M25B, None)


def _words(bits):
    padded = np.zeros(((len(bits) + 63) // 64) * 64, dtype=bool)
    padded[: len(bits)] = bits
    return np.packbits(padded.reshape(-1, 64), axis=1, bitorder="little").view(np.uint64).reshape(-1)


class Leaf:
    """One leaf on the host: rows, ord -> doc, liveDocs, masks (all over docs)."""

    def __init__(self, base, max_doc, vecs, o2d=None, live=None):
        self.base, self.max_doc, self.vecs, self.o2d, self.live = base, max_doc, vecs, o2d, live
        self.masks = {}

    def accept_rows(self, mask_id):
        """liveDocs & mask, per ROW (the oracle's live_words: row r = doc r of its matrix)."""
        acc = np.ones(self.max_doc, bool) if self.live is None else self.live.copy()
        if mask_id is not None:
            acc &= self.masks[mask_id]
        return acc if self.o2d is None else acc[self.o2d]

    def upload(self, ctx):
        g = api.GpuSegment(ctx, self.max_doc, self.base)
        if self.vecs is None:   # the leaf lacks the field (it holds another one)
            g.add_vectors(FIELD + 6, np.ones((4, 16), np.float32), np.arange(4, dtype=np.int32))
        else:
            g.add_vectors(FIELD, self.vecs, self.o2d)
        g.seal()
        if self.live is not None:
            g.set_live_docs(_words(self.live))
        for mid, m in self.masks.items():
            g.set_mask(mid, _words(m))
        return g


def reference_lists(oracle, sim, queries, leaves, kinds, depth=100):
    """Per query the oracle's top `depth` (unboosted score, global doc) under its own filter: queries that share a filter kind go
    through the oracle together, per leaf; the leaves' lists merged by (score desc, doc asc)."""
    out = [None] * len(queries)
    for kind in set(kinds):
        idx = [i for i, kd in enumerate(kinds) if kd == kind]
        merged = [[] for _ in idx]
        for lf in leaves:
            if lf.vecs is None:
                continue
            rows, scores, cnt = oracle.knn_exact(sim, queries[idx], lf.vecs, depth, live_words=_words(lf.accept_rows(kind)), n_threads=8)
            for j in range(len(idx)):
                for r, s in zip(rows[j][: cnt[j]].tolist(), scores[j][: cnt[j]]):
                    merged[j].append((np.float32(s), lf.base + (int(lf.o2d[r]) if lf.o2d is not None else r)))
        for j, i in enumerate(idx):
            merged[j].sort(key=lambda t: (-float(t[0]), t[1]))
            out[i] = merged[j][:depth]
    return out


def expected(full, k, boost, min_score):
    return [(np.float32(s) * np.float32(boost), d) for s, d in full if s >= np.float32(min_score)][:k]


def check_hits(got, exp, what):
    assert got.docs.tolist() == [d for _, d in exp], what
    assert got.scores.view(np.uint32).tolist() == np.array([s for s, _ in exp], dtype=np.float32).view(np.uint32).tolist(), what
    assert got.total_hits == len(got.docs) and not got.relation_gte, what


def threshold_of(full, kind):
    """0: none; 1: the reference's 60th score (a shorter list: its middle); 2: above the best score -- an empty answer."""
    if kind == 0:
        return 0.0
    if kind == 2:
        return float(full[0][0]) * 2.0 + 1.0 if full else 1.0
    if not full:
        return 0.5
    return float(full[60][0]) if len(full) > 60 else float(full[len(full) // 2][0])


@functools.lru_cache(maxsize=None)
def mixed_index(dim):
    """4000 / 2500 / 900 rows with a sparse ord -> doc map and deletes, and a leaf that lacks the field; the five masks on each."""
    rng = np.random.default_rng(1000 + dim)
    leaves, base = [], 0
    for si, n in enumerate((4000, 2500, 0, 900)):
        if n == 0:
            lf = Leaf(base, 500, None)
        else:
            max_doc = 2 * n if si == 1 else n
            o2d = np.sort(rng.choice(max_doc, size=n, replace=False)).astype(np.int32) if si == 1 else None
            live = rng.random(max_doc) > 0.1 if si in (0, 3) else None
            lf = Leaf(base, max_doc, rng.standard_normal((n, dim)).astype(np.float32), o2d, live)
        lf.masks = {M25: rng.random(lf.max_doc) < 0.25, M1: rng.random(lf.max_doc) < 0.01, M7: np.zeros(lf.max_doc, bool),
                    M0: np.zeros(lf.max_doc, bool), M25B: rng.random(lf.max_doc) < 0.25}
        leaves.append(lf)
        base += lf.max_doc
    for lf, n7 in zip((leaves[0], leaves[1], leaves[3]), (3, 3, 1)):   # 7 accepted rows in total: live docs that have a vector
        docs = np.arange(lf.max_doc) if lf.o2d is None else lf.o2d
        ok = docs[lf.live[docs]] if lf.live is not None else docs
        lf.masks[M7][rng.choice(ok, size=n7, replace=False)] = True
    assert sum(int(lf.accept_rows(M7).sum()) for lf in leaves if lf.vecs is not None) == 7
    queries = rng.standard_normal((70, dim)).astype(np.float32)
    return leaves, queries


@pytest.fixture(scope="module")
def searchers():
    """(context flags, dim) -> (context, searcher over mixed_index(dim)), uploaded once."""
    made, ctxs = {}, {}

    def get(flags, dim):
        if (flags, dim) not in made:
            if flags not in ctxs:
                ctxs[flags] = api.GpuContext(device_id=0, max_batch=64, flags=flags)
            gl = [lf.upload(ctxs[flags]) for lf in mixed_index(dim)[0]]
            made[(flags, dim)] = (ctxs[flags], api.GpuIndexSearcher(ctxs[flags], gl, api.IndexStatistics()), gl)
        return made[(flags, dim)][:2]

    yield get
    for _, _, gl in made.values():
        for g in gl:
            g.release()
    for c in ctxs.values():
        c.close()


_REFS = {}


def mixed_reference(oracle, dim, sim_name):
    """The 70 requests of the mixed panel and their reference lists: computed once per (dim, similarity), shared by both routes."""
    if (dim, sim_name) not in _REFS:
        leaves, queries = mixed_index(dim)
        nq = len(queries)
        kinds = [KINDS[(q + q // 32) % 6] for q in range(nq)]   # queries 0..31 and 32..63 each see all six
        ks = [(1, 10, 37, 100)[(q // 3 + q) % 4] for q in range(nq)]
        boosts = [(0.5, 1.0, 2.0)[(q // 5) % 3] for q in range(nq)]
        full = reference_lists(oracle, SIMS[sim_name], queries, leaves, kinds)
        mins = [threshold_of(full[q], (q // 2) % 3) for q in range(nq)]
        for half in (range(0, 32), range(32, 64)):
            assert {kinds[q] for q in half} == set(KINDS)
        _REFS[(dim, sim_name)] = (kinds, ks, boosts, mins, full)
    return _REFS[(dim, sim_name)]


@pytest.mark.parametrize("sim_name", ["cosine", "l2_norm", "max_inner_product"])
@pytest.mark.parametrize("dim", [64, 24])
@pytest.mark.parametrize("flags", [0, _lib.NRTGPU_FLAG_NO_VECTOR_SKETCH], ids=["sketch", "fp32"])
def test_mixed_panel_matches_the_oracle(searchers, oracle, flags, dim, sim_name):
    """70 requests = a pass of 64 (two halves of 32 on paired workgroups in the fp32 kernel) and one of 6, every filter kind, k,
    boost and threshold kind in each half."""
    ctx, sr = searchers(flags, dim)
    leaves, queries = mixed_index(dim)
    kinds, ks, boosts, mins, full = mixed_reference(oracle, dim, sim_name)
    ctx.reset_stats()
    got = sr.knn_search_requests(FIELD, sim_name, queries, ks, boosts, [api.MaskFilter(kd) if kd is not None else None for kd in kinds], mins)
    st = ctx.stats()
    assert st["knn_panels"] == 2 and (st["knn_sketch_launches"] == 0) == bool(flags), st
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


def test_equal_requests_take_knn_searchs_own_path(oracle):
    """All requests equal: nrtgpu_knn_search's bits and its route -- with the gather knob open and a 1 % filter no sketch launch;
    two different filters under the same setting: the full pass."""
    leaves, queries = mixed_index(64)
    ctx = api.GpuContext(device_id=0, max_batch=64)
    gl = [lf.upload(ctx) for lf in leaves]
    try:
        sr = api.GpuIndexSearcher(ctx, gl, api.IndexStatistics())
        qs, n = queries[:5], 5
        full = reference_lists(oracle, 0, qs, leaves, [M1] * n)
        thr = float(full[0][len(full[0]) // 2][0])
        for gather in (0, 1000):
            ctx.set_knn_gather(gather)
            want = sr.knn_search(FIELD, "cosine", qs, 10, boost=2.0, filter=api.MaskFilter(M1), min_score=thr)
            ctx.reset_stats()
            got = sr.knn_search_requests(FIELD, "cosine", qs, [10] * n, [2.0] * n, [api.MaskFilter(M1)] * n, [thr] * n)
            st = ctx.stats()
            assert (st["knn_sketch_launches"] == 0) == (gather != 0) and st["knn_panels"] == 1, (gather, st)
            for q in range(n):
                assert got[q].docs.tolist() == want[q].docs.tolist() and got[q].total_hits == want[q].total_hits
                assert got[q].scores.view(np.uint32).tolist() == want[q].scores.view(np.uint32).tolist()
                check_hits(got[q], expected(full[q], 10, 2.0, thr), (gather, q))
        # (the knob is still open) two filters in one pass: all rows are passed over, from the sketch
        kinds = [M1, M7, M1, M7, M1]
        full2 = reference_lists(oracle, 0, qs, leaves, kinds)
        ctx.reset_stats()
        got = sr.knn_search_requests(FIELD, "cosine", qs, [10] * n, None, [api.MaskFilter(kd) for kd in kinds], None)
        st = ctx.stats()
        assert st["knn_sketch_launches"] >= 1 and st["knn_panels"] == 1 and st["knn_rows"] == 4000 + 2500 + 900, st
        for q in range(n):
            check_hits(got[q], expected(full2[q], 10, 1.0, 0.0), q)
    finally:
        for g in gl:
            g.release()
        ctx.close()


@pytest.mark.parametrize("n", [300_000, 400_000])
def test_a_selective_filter_next_to_unfiltered_queries(oracle, n):
    """One member's filter accepts fewer than k rows among the first 65536: its theta stays unknown while the others' tighten, it
    keeps a slot per row in the long rounds next to queries that only append what beats their theta.  At 400 000 rows the long
    round is longer than a candidate list (2^18): the overflow is flagged and the WHOLE panel is redone in bounded rounds -- the
    other 39 must still get their exact answers."""
    rng = np.random.default_rng(21 + n)
    dim, k, nq, sel = 16, 64, 40, 17
    vecs = rng.standard_normal((n, dim)).astype(np.float32)
    lf = Leaf(0, n, vecs)
    m = np.zeros(n, bool)
    m[5:45] = True                                                   # 40 rows < k among the first 70 000 ...
    m[rng.choice(np.arange(70_000, n), size=5000, replace=False)] = True   # ... 5 000 further on
    lf.masks[M1] = m
    queries = rng.standard_normal((nq, dim)).astype(np.float32)
    kinds = [M1 if q == sel else None for q in range(nq)]
    full = reference_lists(oracle, 3, queries, [lf], kinds, depth=k)
    ctx = api.GpuContext(device_id=0, max_batch=64)
    g = lf.upload(ctx)
    try:
        sr = api.GpuIndexSearcher(ctx, [g], api.IndexStatistics())
        got = sr.knn_search_requests(FIELD, "max_inner_product", queries, [k] * nq, None, [api.MaskFilter(kd) if kd else None for kd in kinds], None)
        for q in range(nq):
            check_hits(got[q], expected(full[q], k, 1.0, 0.0), q)
        assert all(m[d] for d in got[sel].docs.tolist()) and len(got[sel].docs) == k
    finally:
        g.release()
        ctx.close()


def test_uncertified_members_take_the_second_pass_with_their_own_filter_and_threshold(oracle):
    """Near-duplicates of a large norm defeat the certificate (l2_norm: the estimate of |q - v|^2 is all rounding): the second pass
    restarts every uncertified member from ITS threshold and filter."""
    rng = np.random.default_rng(404)
    dim, n, k, nq = 32, 20_000, 25, 8
    centre = (rng.standard_normal(dim) * 3.0 + 17.5).astype(np.float32)           # |centre| ~ 100
    assert 80.0 < float(np.linalg.norm(centre)) < 125.0
    vecs = (centre + rng.standard_normal((n, dim)).astype(np.float32) * np.float32(1e-3)).astype(np.float32)
    lf = Leaf(0, n, vecs)
    lf.masks[M25] = rng.random(n) < 0.25
    queries = (centre + rng.standard_normal((nq, dim)).astype(np.float32) * np.float32(1e-3)).astype(np.float32)
    kinds = [M25 if q % 2 == 0 else None for q in range(nq)]     # half filtered at 25 % ...
    full = reference_lists(oracle, 2, queries, [lf], kinds)
    mins = [0.0 if q % 2 == 0 else threshold_of(full[q], 1) for q in range(nq)]   # ... half with a threshold
    ctx = api.GpuContext(device_id=0, max_batch=64)
    g = lf.upload(ctx)
    try:
        sr = api.GpuIndexSearcher(ctx, [g], api.IndexStatistics())
        ctx.reset_stats()
        got = sr.knn_search_requests(FIELD, "l2_norm", queries, [k] * nq, None, [api.MaskFilter(kd) if kd else None for kd in kinds], mins)
        for q in range(nq):
            check_hits(got[q], expected(full[q], k, 1.0, mins[q]), q)
        assert ctx.stats()["knn_second_passes"] >= 1
    finally:
        g.release()
        ctx.close()


def _park(ctx, threads, done, want_pending=None):
    """Start `threads`; wait until the knn request coalescer reports want_pending parked callers (None: until all have returned --
    a held leader leaves by itself once a whole panel of 64 waits)."""
    for t in threads:
        t.start()
    t_end = time.monotonic() + 60.0
    while time.monotonic() < t_end:
        if want_pending is not None and ctx.debug_coalescer_pending(2) >= want_pending:
            return True
        if want_pending is None and done() >= len(threads):
            return True
        time.sleep(0.001)
    return False


def test_coalesced_callers_with_their_own_filters_share_one_panel(dev_lib, oracle):
    """nrtgpu_knn_search_coalesced: 64 callers parked behind nrtgpu_debug_hold_coalescers, each with its own query, one of 6
    filters, its own k, boost and threshold, leave as ONE panel (through nrtgpu_knn_search that number cannot be below the number of
    distinct filters) and each gets the oracle's bits.  Panels are asserted by construction: a held leader leaves with 64 waiting,
    never with fewer."""
    rng = np.random.default_rng(515)
    dim, n, n_callers = 64, 40_000, 64
    lf = Leaf(0, n, rng.standard_normal((n, dim)).astype(np.float32), live=rng.random(n) > 0.05)
    lf.masks = {M25: rng.random(n) < 0.25, M1: rng.random(n) < 0.01, M7: np.zeros(n, bool), M0: np.zeros(n, bool), M25B: rng.random(n) < 0.25}
    lf.masks[M7][rng.choice(np.flatnonzero(lf.live), size=7, replace=False)] = True
    queries = rng.standard_normal((n_callers + 16, dim)).astype(np.float32)
    kinds = [KINDS[q % 6] for q in range(n_callers)] + [KINDS[q % 3] for q in range(16)]
    sims = ["cosine"] * n_callers + ["l2_norm"] * 16
    ks = [int(x) for x in rng.choice([1, 10, 37, 100], size=n_callers + 16)]
    boosts = [float(x) for x in rng.choice([0.5, 1.0, 2.0], size=n_callers + 16)]
    full = reference_lists(oracle, 0, queries[:n_callers], [lf], kinds[:n_callers]) + \
        reference_lists(oracle, 2, queries[n_callers:], [lf], kinds[n_callers:])
    mins = [threshold_of(full[q], q % 3) for q in range(n_callers + 16)]
    c = api.GpuContext(device_id=0, max_batch=64)
    g = lf.upload(c)
    sr = api.GpuIndexSearcher(c, [g], api.IndexStatistics())
    results, errors = {}, {}

    def call(i):
        return sr.knn_search_coalesced(FIELD, sims[i], queries[i], ks[i], boost=boosts[i],
                                       filter=api.MaskFilter(kinds[i]) if kinds[i] is not None else None, min_score=mins[i])

    def caller(i, rep, deadline=None):
        try:
            if deadline is not None:
                api.GpuContext.set_thread_deadline(deadline)
            results[(i, rep)] = call(i)
        except api.NrtGpuError as e:
            errors[(i, rep)] = e

    def check(i, rep):
        check_hits(results[(i, rep)], expected(full[i], ks[i], boosts[i], mins[i]), (i, rep, kinds[i], ks[i], boosts[i], mins[i]))

    try:
        check_hits(call(1), expected(full[1], ks[1], boosts[1], mins[1]), "a lone caller runs at once")
        # 64 callers, 6 filters: one panel
        for rep in range(2):
            c.reset_stats()
            c.debug_hold_coalescers(True)
            try:
                ok = _park(c, [threading.Thread(target=caller, args=(i, rep)) for i in range(n_callers)], lambda: len(results) + len(errors) - rep * n_callers)
            finally:
                c.debug_hold_coalescers(False)
            assert ok and not errors, errors
            assert c.stats()["knn_panels"] == 1, (rep, c.stats())
            for i in range(n_callers):
                check(i, rep)
        # 16 callers of another similarity first, then the 64: the 16 leave together when 64 wait, the 64 when they are all there
        results.clear()
        c.reset_stats()
        c.debug_hold_coalescers(True)
        try:
            first = [threading.Thread(target=caller, args=(i, 2)) for i in range(n_callers, n_callers + 16)]
            assert _park(c, first, None, want_pending=16)
            # requests that cannot be answered fail alone, at once, while the others wait
            with pytest.raises(api.NrtGpuError) as e:
                sr.knn_search_coalesced(FIELD, "l2_norm", queries[0], 10, filter=api.MaskFilter(77))
            assert e.value.code == _lib.NRTGPU_ERR_UNSUPPORTED
            with pytest.raises(api.NrtGpuError) as e:
                sr.knn_search_coalesced(FIELD, "l2_norm", np.ones(24, np.float32), 10)
            assert e.value.code == _lib.NRTGPU_ERR_INVALID_ARG
            assert c.debug_coalescer_pending(2) == 16
            rest = [threading.Thread(target=caller, args=(i, 2)) for i in range(n_callers)]
            ok = _park(c, rest, lambda: len(results) + len(errors) - 16)
        finally:
            c.debug_hold_coalescers(False)
        for t in first + rest:
            t.join()
        assert ok and not errors, errors
        assert c.stats()["knn_panels"] == 2, c.stats()
        for i in range(n_callers + 16):
            check(i, 2)
        # a caller whose deadline passes in the queue (behind a leader that is held): TIMEOUT for it alone
        results.clear()
        c.debug_hold_coalescers(True)
        try:
            leader = threading.Thread(target=caller, args=(0, 3))
            assert _park(c, [leader], None, want_pending=1)
            late = threading.Thread(target=caller, args=(2, 3, 0.02))
            assert _park(c, [late], None, want_pending=2)
            time.sleep(0.03)
        finally:
            c.debug_hold_coalescers(False)
        leader.join()
        late.join()
        check(0, 3)
        assert errors[(2, 3)].code == _lib.NRTGPU_ERR_TIMEOUT and "waited for a panel" in str(errors[(2, 3)]), errors
        assert [c.debug_coalescer_pending(w) for w in (0, 1, 2)] == [0, 0, 0]
    finally:
        c.debug_hold_coalescers(False)
        g.release()
        c.close()


def test_a_bad_request_refuses_the_whole_call_and_names_itself(searchers, oracle):
    ctx, sr = searchers(0, 64)
    _, queries = mixed_index(64)
    qs, n = queries[:4], 4
    ctx.reset_stats()
    inv, uns = _lib.NRTGPU_ERR_INVALID_ARG, _lib.NRTGPU_ERR_UNSUPPORTED

    def refused(code, names, **kw):
        args = dict(ks=[10] * n, boosts=None, filters=None, min_scores=None)
        args.update(kw)
        with pytest.raises(api.NrtGpuError) as e:
            sr.knn_search_requests(FIELD, "cosine", qs, args["ks"], args["boosts"], args["filters"], args["min_scores"])
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
    L = _lib.load()
    outs, _, _ = api._topdocs_outputs(n, 10)
    ks = np.full(n, 10, np.int32)
    neg = np.array([0, M25, 0, -3], np.int32)
    call = lambda dim, ks_p, masks_p: L.nrtgpu_knn_search_requests(ctx._h, sr._segs, sr._bases, len(sr.leaves), FIELD, 0, qs.ctypes.data, n, dim,  # noqa: E731
                                                                    ks_p, None, masks_p, None, outs)
    assert call(64, ks.ctypes.data, neg.ctypes.data) == inv and b"query 3:" in L.nrtgpu_last_error()
    assert call(64, None, None) == inv            # ks == NULL
    assert call(24, ks.ctypes.data, None) == inv  # a dimension other than the field's
    assert call(4096, ks.ctypes.data, None) == uns
    assert ctx.stats()["knn_panels"] == 0         # nothing was launched
    # NULL boosts / filters / thresholds: all 1, none, none
    want = sr.knn_search(FIELD, "cosine", qs, 10)
    got = sr.knn_search_requests(FIELD, "cosine", qs, [10, 10, 10, 7])
    for q in range(n):
        kq = 7 if q == 3 else 10
        assert got[q].docs.tolist() == want[q].docs.tolist()[:kq]
        assert got[q].scores.view(np.uint32).tolist() == want[q].scores.view(np.uint32).tolist()[:kq]


def test_a_byte_field_is_refused(searchers):
    ctx, _ = searchers(0, 64)
    g = api.GpuSegment(ctx, 64, 0)
    g.add_byte_vectors(FIELD, np.ones((64, 16), np.int8))
    g.seal()
    try:
        sr = api.GpuIndexSearcher(ctx, [g], api.IndexStatistics())
        for call in (lambda: sr.knn_search_requests(FIELD, "cosine", np.ones((2, 16), np.float32), [3, 4]),
                     lambda: sr.knn_search_coalesced(FIELD, "cosine", np.ones(16, np.float32), 3)):
            with pytest.raises(api.NrtGpuError) as e:
                call()
            assert e.value.code == _lib.NRTGPU_ERR_INVALID_ARG and "byte" in str(e.value)
    finally:
        g.release()
