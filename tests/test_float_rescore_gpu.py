"""BM25 recall + rescore over a FLOAT vector field on the device at every dimension the kernels treat differently:
nrtgpu_search_hybrid_batch (fused: hybrid_rescore_kernel, knn_wave_partials) against nrtgpu_search_bm25_batch +
nrtgpu_rescore_vectors (two calls: rescore_vectors_kernel, knn_wave_score) BIT for bit, and the two-call answer against a float64
restatement of QueryRescore that never calls the code under test (tests/_float_rescore_ref.py: the derived interval; its own
checks run on the host in tests/test_float_rescore_ref_host.py).

The index is tests/test_hybrid_gpu.py's shape (three leaves of a synthetic corpus) with three float fields per dimension in
3 / 64 / 100 / 200 / 260 / 768 / 2048 (resident, padded to a multiple of 16: 16 / 64 / 112 / 208 / 272 / 768 / 2048 -- at 208
only lanes 0-15 of a wave take knn_wave_partials' four-element step, the others only its tail loop; at 272 every lane takes the
step once and lanes 0-15 a tail element behind it; 768 and 2048 run the step 3 and 8 times): "plain" rows for cosine, the same with a zero row every 97 for l2_norm and max_inner_product, unit rows for dot_product.
  leaf 0: a row per doc up to n_vec < max_doc (the docs behind n_vec have no vector)
  leaf 1: a sparse ord -> doc map (60 % of the docs)
  leaf 2: no vector field at all (its hits keep queryWeight * first)
Rows and queries: standard normal with +-3 / +-1.5 at the marker positions; dimension 3: four distinct rows, so that with
queryWeight = 0 most combined scores tie bit for bit and the docid decides."""
import numpy as np
import pytest

from nrtsearch_amd import _lib, api, synth
from tests import _float_rescore_ref as R

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
FIELD = {(kind, d): 10 + len(R.DIMS) * ki + di for ki, kind in enumerate(R.KINDS) for di, d in enumerate(R.DIMS)}


def _index(n_docs, ranks):
    rng = np.random.default_rng(31)
    corpus = synth.build_corpus(n_docs, ranks, n_segments=3)
    ctx = api.GpuContext(0, max_batch=64)
    bases, max_docs = [s.doc_base for s in corpus.segments], [s.max_doc for s in corpus.segments]
    leaves, per_field = [], {key: [] for key in FIELD}
    for si, seg in enumerate(corpus.segments):
        g = api.GpuSegment(ctx, seg.max_doc, seg.doc_base)
        g.add_field_norms(0, seg.norms)
        g.add_terms(0, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
        have = np.flatnonzero(rng.random(seg.max_doc) < 0.6).astype(np.int32)
        for key in FIELD:
            kind, d = key
            if si == 0:
                v = R.make_rows(rng, seg.max_doc * 4 // 5 + 3, d, kind)
                g.add_vectors(FIELD[key], v)
                per_field[key].append((v, None))
            elif si == 1:
                v = R.make_rows(rng, len(have), d, kind)
                g.add_vectors(FIELD[key], v, have)
                per_field[key].append((v, have))
            else:
                per_field[key].append(None)
        g.seal()
        leaves.append(g)
    sr = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics.from_corpus(corpus))
    tables = {key: R.Table(key[1], bases, max_docs, per_field[key]) for key in FIELD}
    return dict(corpus=corpus, ctx=ctx, leaves=leaves, tables=tables, sr=sr, bases=bases, max_docs=max_docs)


@pytest.fixture(scope="module")
def idx():
    h = _index(12_000, [1, 3, 8, 20, 60, 300, 2000])
    yield h
    for g in h["leaves"]:
        g.release()
    h["ctx"].close()


def _bq(terms):
    return api.BooleanQuery(tuple(api.TermQuery(0, int(t)) for t in terms))


def _ranges(table, sim, q, docs, first_scores, qw, rw, boost, terms=None):
    why, rows = table.lookup(docs)
    has = why == R.Table.HAS
    if sim == 0:
        rows = np.where(has[:, None], rows, f32(1))       # (a doc without a vector: a stand-in row, its range is not used)
    second = R.second_pass(sim, q, rows, boost, table.dim, terms)
    return why, R.combined(qw, rw, np.asarray(first_scores, dtype=f32), has, second)


@pytest.mark.parametrize("dim", R.DIMS)
@pytest.mark.parametrize("sim_name", list(R.SIMS))
def test_fused_equals_two_calls_equals_the_restatement(idx, sim_name, dim):
    sr, sim, kind = idx["sr"], R.SIMS[sim_name], R.KIND_OF_SIM[sim_name]
    field, table = FIELD[(kind, dim)], idx["tables"][(kind, dim)]
    recall, window, qw, rw, boost = R.SHAPES[dim]
    qs = [_bq(t) for t in R.TERM_SETS]
    mg = [api.TopScoreDocCollectorManager(recall)] * len(qs)
    qv = R.make_queries(np.random.default_rng([3, sim, dim]), len(qs), dim, kind)
    fused = sr.search_hybrid_batch(qs, mg, field, sim_name, qv, window, qw, rw, boost)
    assert len(fused) == len(qs)
    seen = dict(hits=0, leaf2=0, gap=0, behind=0, ties=0, window_above_n=0, window_below_n=0, full=0, empty=0)
    worst, failures = 0.0, []
    for i, q in enumerate(qs):
        where = (sim_name, dim, i)
        first = sr.search(q, mg[i])
        two = sr.rescore_vectors(first, field, sim_name, qv[i], window, qw, rw, boost)
        # the restatement first: a wrong fused answer is then told from a wrong two-call answer
        why, (ref, lo, hi) = _ranges(table, sim, qv[i], first.docs, first.scores, qw, rw, boost)
        assert len(set(first.docs.tolist())) == len(first.docs)
        worst = max(worst, R.check_answer(first.docs.tolist(), ref, lo, hi, two.docs, two.scores, window, where))
        try:
            R.check_answer(first.docs.tolist(), ref, lo, hi, fused[i].docs, fused[i].scores, window, where + ("fused",))
        except AssertionError as e:
            failures.append(e)
        if fused[i].docs.tolist() != two.docs.tolist() or fused[i].scores.view(np.uint32).tolist() != two.scores.view(np.uint32).tolist():
            failures.append(AssertionError((where, "fused != two calls")))
        assert fused[i].total_hits == first.total_hits and fused[i].relation_gte == first.relation_gte, where
        seen["hits"] += len(first.docs)
        seen["leaf2"] += int((why == R.Table.NO_FIELD).sum())
        seen["gap"] += int((why == R.Table.GAP).sum())
        seen["behind"] += int((why == R.Table.BEHIND).sum())
        bits = two.scores.view(np.uint32).tolist()
        seen["ties"] += len(bits) - len(set(bits))
        seen["window_above_n"] += window > len(first.docs) > 0
        seen["window_below_n"] += window < len(first.docs)
        seen["full"] += len(first.docs) == _lib.NRTGPU_MAX_K
        seen["empty"] += len(first.docs) == 0 and len(two.docs) == 0 and len(fused[i].docs) == 0 and first.total_hits == 0
    print(f"float rescore {sim_name} {dim}: max |got - reference| / half-width = {worst:.3f}; {seen}")
    assert not failures, failures[:3]
    # the cases the hits must have covered (asserted on the INPUTS, so that a changed corpus cannot hollow the test out)
    assert seen["hits"] > 200 and seen["leaf2"] >= 10 and seen["gap"] >= 10 and seen["behind"] >= 5, seen
    assert seen["empty"] == 1, seen                       # the term without postings: an empty first pass, an empty answer
    assert seen["window_above_n"] >= 1, seen              # (the rarest term's few hits lie below every window)
    if dim in (3, 64, 260, 768):
        assert seen["window_below_n"] >= 1, seen
    if dim == 3:
        assert seen["ties"] > 500, seen                   # qw = 0 over four distinct rows: the docid decides
    if dim == 200:
        assert recall == _lib.NRTGPU_MAX_K and seen["full"] >= 1, seen


NS = [0, 1, 3, 4, 5, 129]    # hits of one leaf, that is of one launch of rescore_vectors_kernel (four waves, four hits per block)


@pytest.mark.parametrize("dim", [100, 260])
@pytest.mark.parametrize("sim_name", list(R.SIMS))
def test_rescore_vectors_over_hand_made_hit_lists(idx, sim_name, dim):
    """No BM25: unsorted lists with one doc twice, every count of NS in every kind of leaf, docs behind n_vec and in leaf 1's gaps
    among them; the window above n."""
    sr, sim, kind = idx["sr"], R.SIMS[sim_name], R.KIND_OF_SIM[sim_name]
    field, table = FIELD[(kind, dim)], idx["tables"][(kind, dim)]
    rng = np.random.default_rng([5, sim, dim])
    q = R.make_queries(rng, 1, dim, kind)[0]
    bases, max_docs = idx["bases"], idx["max_docs"]
    n_vec0 = len(table.leaves[0][0])
    cases = [(0, 0, 0)] + [(NS[i], NS[(i + 1) % len(NS)], NS[(i + 2) % len(NS)]) for i in range(len(NS))]
    worst, seen = 0.0, dict(behind=0, gap=0, leaf2=0, twice=0)
    for ci, counts in enumerate(cases):
        docs = []
        for si, c in enumerate(counts):
            pick = rng.choice(max_docs[si], size=c, replace=False) + bases[si]
            if si == 0 and c >= 3:
                pick[-1] = bases[0] + n_vec0 + int(rng.integers(0, max_docs[0] - n_vec0))   # behind n_vec: no vector
                pick[-2] = bases[0] + n_vec0 - 1                                            # the last row
            if c >= 3:
                pick[1] = pick[0]                                                           # one doc twice
                seen["twice"] += 1
            docs += pick.tolist()
        docs = np.array(docs, dtype=np.int32)[rng.permutation(len(docs))]
        first_scores = rng.uniform(0.1, 8.0, size=len(docs)).astype(f32)
        qw, rw, boost = (1.0, 2.5, 0.37) if ci % 2 else (0.5, 4.0, 2.0)
        hits = api.TopDocs(docs, first_scores, len(docs), False)
        got = sr.rescore_vectors(hits, field, sim_name, q, len(docs) + 7, qw, rw, boost)
        why, (ref, lo, hi) = _ranges(table, sim, q, docs, first_scores, qw, rw, boost)
        worst = max(worst, R.check_answer(docs.tolist(), ref, lo, hi, got.docs, got.scores, len(docs) + 7, (sim_name, dim, counts)))
        assert len(got.docs) == sum(counts)
        seen["behind"] += int((why == R.Table.BEHIND).sum())
        seen["gap"] += int((why == R.Table.GAP).sum())
        seen["leaf2"] += int((why == R.Table.NO_FIELD).sum())
    print(f"float rescore (hand-made lists) {sim_name} {dim}: max |got - reference| / half-width = {worst:.3f}; {seen}")
    assert seen["behind"] >= 3 and seen["gap"] >= 10 and seen["leaf2"] >= 10 and seen["twice"] >= 6, seen


@pytest.mark.parametrize("dim", [100, 2048])
@pytest.mark.parametrize("sim_name", list(R.SIMS))
def test_rescored_scores_of_the_exact_searchs_top_20(idx, sim_name, dim):
    """queryWeight 0, rescoreWeight 1: the combined score IS the second-pass score.  nrtgpu_knn_exact returns the oracle's bits (a
    scalar left-to-right sum: dim_resident + 1 roundings per term); the rescorer sums in wave order.  Each must lie in its own
    derived range around the SAME float64 value of that doc; the wave order's range lies inside the scalar sum's."""
    sr, sim, kind = idx["sr"], R.SIMS[sim_name], R.KIND_OF_SIM[sim_name]
    field, table = FIELD[(kind, dim)], idx["tables"][(kind, dim)]
    boost = 0.37 if dim == 100 else 1.0
    q = R.make_queries(np.random.default_rng([9, sim, dim]), 1, dim, kind)[0]
    knn = sr.knn_exact(field, sim_name, q[None, :], 20, boost)[0]
    assert len(knn.docs) == 20 and len(set(knn.docs.tolist())) == 20
    hits = api.TopDocs(knn.docs, np.zeros(20, dtype=f32), 20, False)
    got = sr.rescore_vectors(hits, field, sim_name, q, 20, 0.0, 1.0, boost)
    why, (ref, lo, hi) = _ranges(table, sim, q, knn.docs, hits.scores, 0.0, 1.0, boost)
    assert (why == R.Table.HAS).all()
    R.check_answer(knn.docs.tolist(), ref, lo, hi, got.docs, got.scores, 20, (sim_name, dim))
    _, (sref, slo, shi) = _ranges(table, sim, q, knn.docs, hits.scores, 0.0, 1.0, boost, terms=R.resident(dim) + 1)
    assert np.array_equal(sref, ref)
    ks = knn.scores.astype(f64)
    assert ((slo <= ks) & (ks <= shi)).all(), (sim_name, dim, "knn_exact's score outside the sequential sum's range")
    assert ((slo <= lo) & (hi <= shi)).all()              # (so the rescored scores lie in the range of knn_exact's scores too)
