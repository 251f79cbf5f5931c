"""The exact float vector search on worst-case data (tests/_knn_adversarial.py; tests/test_knn_adversarial_host.py proves on the
CPU that the data is worst-case): the fp16 sketch ranks every decoy above every winner, so all k + max(32, k / 2) nominations
are decoys, the estimate's error sits at 0.5 - 0.93 of the bound E, and only a sound E applied soundly (vectors.cpp: knn_impl;
host_math.h: knn_bound16; plan.h: knn_result_upper / knn_estimate_lower) makes the certification refuse and the second pass
find the winners.  Every case: the oracle's docs, order and score bits; nominations from the sketch; a second pass.  The same
under NRTGPU_FLAG_NO_VECTOR_SKETCH, with identical bits.  A fresh context per search: a sketch that failed lately is skipped
for a few panels (knn_sketch_skip), which would route a case around what it tests.

Mutations of the library (each applied alone and the library rebuilt).  What they do to the emulated search is recorded in
tests/test_knn_adversarial_host.py, which fails under each of them without a GPU; by the same arithmetic, on the device:
  2^-10 -> 2^-11 in knn_bound16            E falls to 0.51 - 0.58 of itself, below need (need / E 0.59 - 0.93): the decoys
                                           certify, and the threshold test's starting theta (min_score - E; the winners' estimates
                                           lie 0.65 - 0.95 E below min_score) passes over the winners.  Every case but
                                           cosine_768 (need / E 0.49)
  score_boost dropped from knn_bound16     E is 4 x too small at boost 4: the decoys certify in test_the_boost_scales_the_bound
                                           [4.0-dot_64, -cosine_64, -mip_64] (l2_norm's bound carries no boost); at boost 0.25
                                           the bound is merely 4 x too wide and the answers stay right -- only the host test's
                                           need / E sees that
  knn_estimate_lower returning s           the second pass's theta and the knn request's starting theta sit above every
                                           winner's estimate: the winners are never nominated.  Every case, the threshold test
                                           included
  knn_result_upper returning m             the k-th decoy's result exceeds the last nomination's estimate: certified.  Every
                                           case but the threshold test (its answer is complete before the certification)
(The table is the emulation's arithmetic.  The mutated libraries were built and run against the host test; they have not been
run on a device.)

Magnitudes at the ends of the float range (the last three tests): for a largest |element| below 2^-113 the sketch's power-of-two
scale is 2^127 or inf and its reciprocal subnormal or 0 -- the sketch would hold inf / NaN and every estimate be NaN or 0, while
the bound stays finite.  host_math.h: knn_sketch_scale refuses such a scale: the field gets no sketch, a query sends its panel to
the fp32 rows; the tests pin that (no sketch launch) next to the oracle's answer.  A field whose |v|^2 overflows never had a
sketch (the seal's sketch_state)."""
import numpy as np
import pytest

from nrtsearch_amd import _lib, api
from tests import _knn_adversarial as ka

pytestmark = pytest.mark.gpu
FLAGS = (0, _lib.NRTGPU_FLAG_NO_VECTOR_SKETCH)
_scores = {}


def oracle_scores(oracle, sim, queries, rows, key):
    """[query][row] -> the oracle's unboosted score, computed once per case."""
    if key not in _scores:
        _scores[key] = np.array([[oracle.vector_score(sim, q, v) for v in rows] for q in queries], dtype=np.float32)
        _scores[key].setflags(write=False)
    return _scores[key]


def expected(scores, docs, k, boost=1.0, live=None, min_score=None):
    """Top k of (score desc, docid asc) over the live rows; min_score applies to the unboosted score, the boost afterwards."""
    keep = np.ones(len(docs), bool) if live is None else live.copy()
    if min_score is not None:
        keep &= scores >= np.float32(min_score)
    s = (scores * np.float32(boost)).astype(np.float32)
    hits = sorted(((float(s[r]), int(docs[r])) for r in np.flatnonzero(keep)), key=lambda t: (-t[0], t[1]))
    return hits[:k]


def check(got, exp, what):
    assert got.docs.tolist() == [d for _, d in exp], what
    assert got.scores.view(np.uint32).tolist() == np.array([s for s, _ in exp], dtype=np.float32).view(np.uint32).tolist(), what


def words(bits):
    padded = np.zeros(((len(bits) + 63) // 64) * 64, dtype=bool)
    padded[: len(bits)] = bits
    return np.packbits(padded.reshape(-1, 64), axis=1, bitorder="little").view(np.uint64).reshape(-1)


def search(flags, leaves, run):
    """leaves: (doc base, rows, ord -> doc or None, live docs or None, mask 1 or None, max_doc).  -> (run(searcher), the stats)."""
    ctx = api.GpuContext(device_id=0, max_batch=64, flags=flags)
    try:
        handles = []
        for base, rows, ord_to_doc, live, mask, max_doc in leaves:
            g = api.GpuSegment(ctx, max_doc, base)
            g.add_vectors(0, rows, ord_to_doc)
            if mask is not None:
                g.set_mask(1, words(mask))
            g.seal()
            if live is not None:
                g.set_live_docs(words(live))
            handles.append(g)
        out = run(api.GpuIndexSearcher(ctx, handles, api.IndexStatistics()))
        st = ctx.stats()
        for g in handles:
            g.release()
        return out, st
    finally:
        ctx.close()


def check_stats(st, flags, second_pass=True, what=""):
    if flags:
        assert st["knn_sketch_launches"] == 0, what
        return
    assert st["knn_sketch_launches"] > 0, (what, st)
    if second_pass:
        assert st["knn_second_passes"] >= 1, (what, st)     # every nomination is a decoy: the certification must refuse


def run_single_leaf(oracle, name, boost=1.0):
    case = ka.build(name, boost)
    sim = ka.SIMS[case.sim_name]
    rows, kind, _ = ka.layout(case)
    queries = ka.panel(case)
    sc = oracle_scores(oracle, sim, queries, rows, name)
    docs = np.arange(len(rows))
    exp = [expected(sc[qi], docs, case.k, boost) for qi in range(2)]
    assert sorted(d for _, d in exp[0]) == np.flatnonzero(kind == 0).tolist()        # the answer is the winners
    answers = []
    for flags in FLAGS:
        got, st = search(flags, [(0, rows, None, None, None, len(rows))], lambda sr: sr.knn_exact(0, case.sim_name, queries, case.k, boost=boost))
        for qi in range(2):
            check(got[qi], exp[qi], (name, flags, qi))
            assert got[qi].total_hits == len(rows)
        check_stats(st, flags, what=name)
        answers.append(got)
    return answers


@pytest.mark.parametrize("name", ka.K10_NAMES)
def test_all_nominations_are_decoys(oracle, name):
    """Four similarities x 64, 100 (resident 112) and 768 dimensions, k = 10, 122 rows, the adversarial query and an ordinary one in
    one panel."""
    run_single_leaf(oracle, name)


def test_k_1(oracle):
    run_single_leaf(oracle, "dot_64_k1")      # 33 nominations


def test_k_700_with_the_nominations_capped_at_1024(oracle):
    run_single_leaf(oracle, "dot_64_k700")    # 700 winners, 1724 decoys; k + k / 2 = 1050 nominations would be needed, 1024 are kept


@pytest.mark.parametrize("boost", [4.0, 0.25])
@pytest.mark.parametrize("name", ["dot_64", "cosine_64", "mip_64", "l2_64"])
def test_the_boost_scales_the_bound(oracle, name, boost):
    """ExactVectorQuery's boost is inside the score, so E (a bound in score units, except l2_norm's) carries it: without it the
    bound is 4 x too small at boost 4."""
    run_single_leaf(oracle, name, boost)


@pytest.mark.parametrize("name", ["dot_64", "mip_64"])
def test_two_leaves_with_different_sketch_scales(oracle, name):
    """The winners' leaf holds one row with an element of 64: its sketch scale is 2^6 below the decoys' leaf's, and the estimates
    of the two leaves must still be comparable (DKnnLeaf.inv_rows_scale) and E hold for both (rows_unit: the larger 1 / scale)."""
    case = ka.build(name)
    sim = ka.SIMS[case.sim_name]
    extra, _ = ka.two_leaf_extra(case)
    rows, kind, _ = ka.layout(case)
    leaf0, leaf1 = rows[kind != 0], np.concatenate([rows[kind == 0], extra])
    queries = ka.panel(case)
    all_rows = np.concatenate([leaf0, leaf1])
    sc = oracle_scores(oracle, sim, queries, all_rows, name + "/two leaves")
    docs = np.arange(len(all_rows))
    exp = [expected(sc[qi], docs, case.k) for qi in range(2)]
    assert sorted(d for _, d in exp[0]) == list(range(len(leaf0), len(leaf0) + case.k))
    for flags in FLAGS:
        got, st = search(flags, [(0, leaf0, None, None, None, len(leaf0)), (len(leaf0), leaf1, None, None, None, len(leaf1))],
                         lambda sr: sr.knn_exact(0, case.sim_name, queries, case.k))
        for qi in range(2):
            check(got[qi], exp[qi], (name, flags, qi))
        check_stats(st, flags, what=name)


def test_sparse_ordinals_and_deleted_decoys(oracle):
    """Rows that are not docids (an ord -> doc map over twice as many docs) and five decoys deleted -- the three the sketch likes
    best among them: they must be neither nominated nor counted."""
    case = ka.build("dot_64")
    rows, kind, ident = ka.layout(case)
    queries = ka.panel(case)
    sc = oracle_scores(oracle, 1, queries, rows, "dot_64")
    ord_to_doc = np.sort(np.random.default_rng(21).choice(2 * len(rows), size=len(rows), replace=False)).astype(np.int32)
    live_rows = ~((kind == 1) & np.isin(ident, ka.DEAD_DECOYS))
    live = np.ones(2 * len(rows), bool)
    live[ord_to_doc[~live_rows]] = False
    exp = [expected(sc[qi], ord_to_doc, case.k, live=live_rows) for qi in range(2)]
    assert sorted(d for _, d in exp[0]) == ord_to_doc[kind == 0].tolist()
    for flags in FLAGS:
        got, st = search(flags, [(0, rows, ord_to_doc, live, None, 2 * len(rows))], lambda sr: sr.knn_exact(0, "dot_product", queries, case.k))
        for qi in range(2):
            check(got[qi], exp[qi], (flags, qi))
            assert got[qi].total_hits == int(live_rows.sum())
        check_stats(st, flags)


@pytest.mark.parametrize("name", ["dot_64", "l2_64", "cosine_64"])
def test_knn_search_with_a_filter_and_a_threshold_between_decoys_and_winners(oracle, name):
    """The knn request path: a pre-filter that drops some decoys and half of the other rows, min_score strictly between the best
    decoy's and the worst winner's result.  The starting theta is knn_estimate_lower(min_score, E): every winner's estimate lies
    well below min_score itself, and exactly the winners come back (k = 20 asks for more than there are).  The answer is
    complete once that theta is right, so no second pass is asserted."""
    case = ka.build(name)
    sim = ka.SIMS[case.sim_name]
    rows, kind, ident = ka.layout(case)
    queries = ka.panel(case)
    sc = oracle_scores(oracle, sim, queries, rows, name)
    lo, hi = sc[0][kind == 1].max(), sc[0][kind == 0].min()
    min_score = np.float32((np.float64(lo) + np.float64(hi)) / 2)
    assert lo < min_score < hi
    mask = ~(((kind == 1) & (ident % 7 == 3)) | ((kind == 2) & (ident % 2 == 1)))
    docs = np.arange(len(rows))
    exp = [expected(sc[qi], docs, 20, boost=2.0, live=mask, min_score=min_score) for qi in range(2)]
    assert sorted(d for _, d in exp[0]) == np.flatnonzero(kind == 0).tolist()
    for flags in FLAGS:
        got, st = search(flags, [(0, rows, None, None, mask, len(rows))],
                         lambda sr: sr.knn_search(0, case.sim_name, queries, 20, boost=2.0, filter=api.MaskFilter(1), min_score=float(min_score)))
        for qi in range(2):
            check(got[qi], exp[qi], (name, flags, qi))
            assert got[qi].total_hits == len(exp[qi])
        check_stats(st, flags, second_pass=False, what=name)


# ---- magnitudes at the ends of the float range --------------------------------------------------------------------------------
SIM_NAMES = ("cosine", "dot_product", "l2_norm", "max_inner_product")


def run_magnitudes(oracle, rows, queries, key, k=10):
    docs = np.arange(len(rows))
    for sim_name in SIM_NAMES:
        sim = ka.SIMS[sim_name]
        sc = oracle_scores(oracle, sim, queries, rows, (key, sim))
        for flags in FLAGS:
            got, st = search(flags, [(0, rows, None, None, None, len(rows))], lambda sr: sr.knn_exact(0, sim_name, queries, k))
            for qi in range(len(queries)):
                check(got[qi], expected(sc[qi], docs, k), (key, sim_name, flags, qi))
            assert st["knn_sketch_launches"] == 0, (key, sim_name, flags)      # no sketch can serve these: the fp32 rows do


def scaled_to(x, absmax):
    return (x * (np.float32(absmax) / np.abs(x).max(axis=-1, keepdims=True))).astype(np.float32)


def test_a_field_whose_largest_element_is_2_to_the_minus_120(oracle):
    rng = np.random.default_rng(120)
    rows = scaled_to(rng.standard_normal((100, 64)), 2.0 ** -120)
    rows[1:] *= rng.random((99, 1)).astype(np.float32)           # (one row holds the field's largest |element|)
    assert np.abs(rows).max() == np.float32(2.0 ** -120)
    run_magnitudes(oracle, rows, rng.standard_normal((3, 64)).astype(np.float32), "tiny field")


def test_a_query_whose_largest_element_is_2_to_the_minus_120(oracle):
    rng = np.random.default_rng(121)
    rows = rng.standard_normal((100, 64)).astype(np.float32)
    queries = np.concatenate([scaled_to(rng.standard_normal((2, 64)), 2.0 ** -120), rng.standard_normal((1, 64)).astype(np.float32)])
    assert np.abs(queries).max(axis=1).tolist() == [2.0 ** -120, 2.0 ** -120, float(np.abs(queries[2]).max())]
    run_magnitudes(oracle, rows, queries, "tiny query")


def test_a_field_whose_squared_norms_overflow(oracle):
    """Largest |element| 2^100: |v|^2 is inf for most rows and the field gets no sketch (segment.cpp: the seal's sketch_state)."""
    rng = np.random.default_rng(122)
    rows = scaled_to(rng.standard_normal((100, 64)), 2.0 ** 100)
    rows[1:] *= (rng.random((99, 1)) * 0.9 + 0.1).astype(np.float32)
    assert np.abs(rows).max() == np.float32(2.0 ** 100)
    run_magnitudes(oracle, rows, rng.standard_normal((3, 64)).astype(np.float32), "huge field")
