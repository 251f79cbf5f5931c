"""BM25 recall + rescore over a BYTE (int8) vector field on the device: nrtgpu_search_hybrid_bytes_batch (fused) against
nrtgpu_search_bm25_batch + nrtgpu_rescore_byte_vectors (two calls), both against a numpy restatement of QueryRescore over the
byte scorer that does not call the code under test, and the second-pass scores against nrtgpu_knn_exact_bytes.

Every comparison is BIT equality on docids and on scores.view(uint32), no hit left out: dot, |q|^2 and |v|^2 are integers (int64
here), the unboosted score is nrtgpu_byte_vector_score (pinned bit for bit by tests/test_byte_vectors_host.py), and every float
step behind it is one IEEE operation: f32(score) * f32(boost), the combine in float64 cast to float32, a sort on (-score, doc).

The index is tests/test_hybrid_gpu.py's shape (three leaves of a synthetic corpus) with one byte field per dimension:
  leaf 0: a row per doc up to n_vec, n_vec % 16 == 7 (the last tile is partial; the docs behind n_vec have no vector)
  leaf 1: a sparse ord -> doc map (60 % of the docs)
  leaf 2: no vector field at all (its hits keep queryWeight * first)
Rows: a zero row every 97 (cosine scores it 0); dimension 2048: rows of all -128 and all 127; dimension 3: four distinct rows, so
that with queryWeight = 0 most combined scores tie and the docid decides."""
import ctypes as C

import numpy as np
import pytest

from nrtsearch_amd import _lib, api, synth

pytestmark = pytest.mark.gpu
SIMS = {"cosine": 0, "dot_product": 1, "l2_norm": 2, "max_inner_product": 3}
DIMS = [3, 64, 100, 768, 2048]
FIELD = {d: 10 + i for i, d in enumerate(DIMS)}
f32, f64 = np.float32, np.float64
FEW = np.array([[1, 2, 3], [-3, 0, 5], [127, -128, 0], [0, 0, 0]], dtype=np.int8)


def _rows(rng, n, dim):
    if dim == 3:
        return FEW[rng.integers(0, len(FEW), size=n)]
    v = rng.integers(-128, 128, size=(n, dim), dtype=np.int8)
    v[::97] = 0
    if dim == 2048:
        v[5::50] = -128
        v[6::50] = 127
    return v


def _queries(rng, n, dim):
    if dim == 3:
        return np.array([[1, 1, 1], [-128, 127, 5], [0, 0, 1], [3, 0, -5], [127, 127, 127]], dtype=np.int8)[np.arange(n) % 5]
    q = rng.integers(-128, 128, size=(n, dim), dtype=np.int8)
    if dim == 2048:
        q[0], q[1] = -128, 127
    return q


def _index(n_docs, ranks, max_batch=64):
    rng = np.random.default_rng(21)
    corpus = synth.build_corpus(n_docs, ranks, n_segments=3)
    ctx = api.GpuContext(0, max_batch=max_batch)
    leaves, rows = [], {d: [] for d in DIMS}      # rows[dim][leaf] = (int8[n_vec, dim], ord_to_doc or None) or None
    for si, seg in enumerate(corpus.segments):
        g = api.GpuSegment(ctx, seg.max_doc, seg.doc_base)
        g.add_field_norms(0, seg.norms)
        g.add_terms(0, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
        have = np.flatnonzero(rng.random(seg.max_doc) < 0.6).astype(np.int32)
        for d in DIMS:
            if si == 0:
                n_vec = ((seg.max_doc - 16) // 16) * 16 + 7
                v = _rows(rng, n_vec, d)
                g.add_byte_vectors(FIELD[d], v)
                rows[d].append((v, None))
            elif si == 1:
                v = _rows(rng, len(have), d)
                g.add_byte_vectors(FIELD[d], v, have)
                rows[d].append((v, have))
            else:
                rows[d].append(None)
        g.seal()
        leaves.append(g)
    sr = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics.from_corpus(corpus))
    return dict(corpus=corpus, ctx=ctx, leaves=leaves, rows=rows, sr=sr, rng=rng, bases=[s.doc_base for s in corpus.segments])


def _close(h):
    for g in h["leaves"]:
        g.release()
    h["ctx"].close()


@pytest.fixture(scope="module")
def big():
    h = _index(60_000, [1, 3, 8, 20, 60, 300, 2000])
    yield h
    _close(h)


@pytest.fixture(scope="module")
def small():
    h = _index(1000, [1, 3, 8, 20])       # fewer than NRTGPU_MAX_K rows: nrtgpu_knn_exact_bytes can return every one of them
    yield h
    _close(h)


def _bq(terms):
    return api.BooleanQuery(tuple(api.TermQuery(0, int(t)) for t in terms))


def _row_of(h, dim, doc):
    """The doc's row of the field (int8[dim]) or None, and whether it lies in a partial last tile: the host's own tables."""
    si = max(i for i, b in enumerate(h["bases"]) if b <= doc)
    entry = h["rows"][dim][si]
    if entry is None:
        return None, False
    v, o2d = entry
    local = doc - h["bases"][si]
    if o2d is None:
        r = local if local < len(v) else -1
    else:
        r = int(np.searchsorted(o2d, local))
        r = r if r < len(o2d) and o2d[r] == local else -1
    if r < 0:
        return None, False
    return v[r], len(v) % 16 != 0 and r >= (len(v) & ~15)


def _c_score(sim, dim, dot, nq, nv):
    out = C.c_float()
    rc = _lib.load().nrtgpu_byte_vector_score(int(sim), int(dim), int(dot), int(nq), int(nv), C.byref(out))
    assert rc == 0, (sim, dim, dot, nq, nv)
    return f32(out.value)


def _second(h, dim, sim, q, doc, boost):
    """f32(unboosted score) * f32(boost), or None for a doc without a vector; the three integers in int64."""
    v, partial = _row_of(h, dim, doc)
    if v is None:
        return None, False
    qi, vi = q.astype(np.int64), v.astype(np.int64)
    return f32(_c_score(sim, dim, (qi * vi).sum(), (qi * qi).sum(), (vi * vi).sum()) * f32(boost)), partial


def _restated(h, first, dim, sim, q, window, qw, rw, boost):
    """QueryRescore over the first pass's hits: (docs, score bits) and what the hits covered."""
    exp, seen = [], dict(partial=0, no_vector=0, zero_row=0)
    for doc, f in zip(first.docs.tolist(), first.scores):
        second, partial = _second(h, dim, sim, q, doc, boost)
        if second is None:
            comb = f32(f64(qw) * f64(f))
            seen["no_vector"] += 1
        else:
            comb = f32(f64(qw) * f64(f) + f64(rw) * f64(second))
            seen["partial"] += partial
            seen["zero_row"] += not _row_of(h, dim, doc)[0].any()
        exp.append((comb, doc))
    exp.sort(key=lambda t: (-float(t[0]), t[1]))
    exp = exp[:window]
    return [d for _, d in exp], np.array([s for s, _ in exp], dtype=np.float32).view(np.uint32).tolist(), seen


TERM_SETS = [[1, 20, 300], [3, 8, 60, 2000], [2000], [1, 3, 8, 20, 60], [300, 2000]]
# (recall, window, queryWeight, rescoreWeight, boost) by dimension: window < n, window == recall, window > n, qw = 0
SHAPES = {3: (1000, 300, 0.0, 1.0, 1.0), 64: (64, 10, 1.0, 1.0, 1.0), 100: (200, 300, 0.5, 4.0, 2.0), 768: (1000, 100, 1.0, 2.5, 0.37),
          2048: (300, 300, 0.25, 3.0, 1.0)}


def _check(h, sr, sim_name, dim, term_sets, totals):
    sim = SIMS[sim_name]
    recall, window, qw, rw, boost = SHAPES[dim]
    qs = [_bq(t) for t in term_sets]
    mg = [api.TopScoreDocCollectorManager(recall)] * len(qs)
    qv = _queries(h["rng"], len(qs), dim)
    fused = sr.search_hybrid_bytes_batch(qs, mg, FIELD[dim], sim_name, qv, window, qw, rw, boost)
    assert len(fused) == len(qs)
    for i, q in enumerate(qs):
        first = sr.search(q, mg[i])
        two = sr.rescore_byte_vectors(first, FIELD[dim], sim_name, qv[i], window, qw, rw, boost)
        where = (sim_name, dim, i)
        assert fused[i].docs.tolist() == two.docs.tolist(), where
        assert fused[i].scores.view(np.uint32).tolist() == two.scores.view(np.uint32).tolist(), where
        assert fused[i].total_hits == first.total_hits and fused[i].relation_gte == first.relation_gte, where
        edocs, ebits, seen = _restated(h, first, dim, sim, qv[i], window, qw, rw, boost)
        assert len(edocs) == min(window, len(first.docs)), where
        assert two.docs.tolist() == edocs, where
        assert two.scores.view(np.uint32).tolist() == ebits, where
        for k, v in seen.items():
            totals[k] = totals.get(k, 0) + v
        totals["hits"] = totals.get("hits", 0) + len(first.docs)
        if window > len(first.docs):
            totals["window_above_n"] = totals.get("window_above_n", 0) + 1
        if window < len(first.docs):
            totals["window_below_n"] = totals.get("window_below_n", 0) + 1
        totals["ties"] = totals.get("ties", 0) + (len(ebits) - len(set(ebits)))


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("sim_name", list(SIMS))
def test_fused_equals_two_calls_equals_the_restatement(big, sim_name, dim):
    totals = {}
    _check(big, big["sr"], sim_name, dim, TERM_SETS, totals)
    # the cases the hits must have covered (asserted on the INPUTS, so that a changed corpus cannot hollow the test out)
    assert totals["hits"] > 200 and totals["no_vector"] > 30, totals        # leaf 2, and the docs absent from leaf 1's map
    if dim in (3, 64, 768):
        assert totals.get("window_below_n", 0) >= 1, totals
    if dim in (100, 2048):
        assert totals.get("window_above_n", 0) >= 1, totals
    if dim == 3:
        assert totals["ties"] > 500, totals                                  # qw = 0 over four distinct rows: the docid decides
    if dim in (768, 2048):
        assert totals["zero_row"] >= 1, totals


def test_hits_in_the_last_partial_tile_and_a_fork_with_deletes(big):
    """A reader version of leaf 0 whose live docs are its last 47 docs with a row (the last whole tile and the 7 rows of the partial
    one behind it) and the docs behind n_vec (no vector), searched on its own: every hit is there."""
    g0 = big["leaves"][0]
    seg = big["corpus"].segments[0]
    n_vec = ((seg.max_doc - 16) // 16) * 16 + 7
    live = np.zeros((seg.max_doc + 63) // 64, dtype=np.uint64)
    for d in range(n_vec - 47, seg.max_doc):
        live[d >> 6] |= np.uint64(1) << np.uint64(d & 63)
    fork = g0.fork(live)
    try:
        sr = api.GpuIndexSearcher(big["ctx"], [fork], api.IndexStatistics.from_corpus(big["corpus"]))
        for sim_name, dim in (("cosine", 768), ("l2_norm", 2048), ("dot_product", 100), ("max_inner_product", 3), ("cosine", 64)):
            totals = {}
            _check(big, sr, sim_name, dim, [[1], [1, 3], [1, 3, 8]], totals)
            assert totals["partial"] >= 3 and totals["no_vector"] >= 1, (sim_name, dim, totals)
        first = sr.search(_bq([1]), api.TopScoreDocCollectorManager(1000))
        assert 10 < len(first.docs) <= seg.max_doc - (n_vec - 47) and first.docs.min() >= n_vec - 47, first.docs   # the deletes were applied
    finally:
        fork.release()


@pytest.mark.parametrize("sim_name", list(SIMS))
def test_second_pass_scores_are_knn_exact_bytes_scores(small, sim_name):
    """queryWeight 0, rescoreWeight 1: the combined score IS the second-pass score ((float)(0 * first + (double)second)).  It must
    be the bits nrtgpu_knn_exact_bytes returns for that doc with k >= the field's rows; a hit without a vector scores 0."""
    sr = small["sr"]
    n_rows = sum(len(e[0]) for e in small["rows"][3] if e is not None)
    assert n_rows <= _lib.NRTGPU_MAX_K
    for dim in DIMS:
        boost = 1.0 if dim == 64 else 0.37
        qv = _queries(small["rng"], 2, dim)
        for qi in range(2):
            knn = sr.knn_exact_bytes(FIELD[dim], sim_name, qv[qi:qi + 1], _lib.NRTGPU_MAX_K, boost)[0]
            assert len(knn.docs) == n_rows or (sim_name == "cosine" and 0 < len(knn.docs) < n_rows)   # (a cosine score can be 0)
            by_doc = dict(zip(knn.docs.tolist(), knn.scores.view(np.uint32).tolist()))
            mg = api.TopScoreDocCollectorManager(1000)
            first = sr.search(_bq([1, 3]), mg)
            assert len(first.docs) > 300
            two = sr.rescore_byte_vectors(first, FIELD[dim], sim_name, qv[qi], len(first.docs), 0.0, 1.0, boost)
            fused = sr.search_hybrid_bytes_batch([_bq([1, 3])], [mg], FIELD[dim], sim_name, qv[qi:qi + 1], len(first.docs), 0.0, 1.0, boost)[0]
            assert fused.docs.tolist() == two.docs.tolist() and fused.scores.view(np.uint32).tolist() == two.scores.view(np.uint32).tolist()
            assert sorted(two.docs.tolist()) == sorted(first.docs.tolist())
            with_row = 0
            for doc, bits in zip(two.docs.tolist(), two.scores.view(np.uint32).tolist()):
                assert bits == by_doc.get(doc, 0), (sim_name, dim, qi, doc)
                with_row += doc in by_doc
            assert 100 < with_row < len(first.docs)
        # the whole table of the big index's checks on this one too (other sizes: leaves of 500 / 250 / 250 docs)
        _check(small, sr, sim_name, 768, [[1, 20], [3, 8]], {})


def test_fused_bytes_under_speculative_thresholds_equals_the_unspeculated_answer(dev_lib, monkeypatch):
    """tests/test_hybrid_gpu.py's speculation test with a byte field as the rescorer: a batch over an index whose live docs all sit
    in the first third of the docid range, where speculative thresholds fail -- tagged queries are run again, first pass and byte
    tail, and come out as without speculation: docids and score bits; the counters show the re-runs."""
    monkeypatch.setenv("NRTGPU_MS_SCATTER", "0")   # (development library: windows in docid order -- where this index defeats the guesses)
    rng = np.random.default_rng(5)
    corpus = synth.build_corpus(3_200_000, [1, 2, 5, 9, 20, 60, 150, 400], n_segments=1)
    seg = corpus.segments[0]
    dim, field = 16, 7
    ctx = api.GpuContext(0, max_batch=64)
    g = api.GpuSegment(ctx, seg.max_doc, seg.doc_base)
    g.add_field_norms(0, seg.norms)
    g.add_terms(0, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
    rows = rng.integers(-128, 128, size=(seg.max_doc, dim), dtype=np.int8)
    g.add_byte_vectors(field, rows)
    g.seal()
    live = np.zeros((seg.max_doc + 63) // 64, dtype=np.uint64)
    live[: int(seg.max_doc * 0.3) // 64] = np.uint64(0xFFFFFFFFFFFFFFFF)
    g.set_live_docs(live)
    sr = api.GpuIndexSearcher(ctx, [g], api.IndexStatistics.from_corpus(corpus))
    h = dict(bases=[0], rows={dim: [(rows, None)]})
    try:
        qs = [_bq(t) for t in ([1, 5, 20, 150, 400], [2, 9, 60], [1, 2, 5, 9, 20, 60, 150, 400], [5, 400], [9, 20, 150])]
        mg = [api.TopScoreDocCollectorManager(1000)] * len(qs)
        qv = rng.integers(-128, 128, size=(len(qs), dim), dtype=np.int8)
        ctx.set_speculation(5.0)
        fused = sr.search_hybrid_bytes_batch(qs, mg, field, "cosine", qv, 100, 1.0, 2.0)
        c = ctx.spec_counters()
        assert c["queries"] == len(qs) and c["reruns"] >= 2, c
        ctx.set_speculation(0.0)
        plain = sr.search_hybrid_bytes_batch(qs, mg, field, "cosine", qv, 100, 1.0, 2.0)
        assert ctx.spec_counters()["queries"] == 0
        for i, (a, b) in enumerate(zip(fused, plain)):
            assert a.docs.tolist() == b.docs.tolist() and a.scores.view(np.uint32).tolist() == b.scores.view(np.uint32).tolist()
            assert len(a.docs) == 100 and a.relation_gte == b.relation_gte   # (the counts are lower bounds: what each run happened to evaluate)
            first = sr.search(qs[i], mg[i])
            edocs, ebits, _ = _restated(h, first, dim, 0, qv[i], 100, 1.0, 2.0, 1.0)
            assert a.docs.tolist() == edocs and a.scores.view(np.uint32).tolist() == ebits
    finally:
        g.release()
        ctx.close()
