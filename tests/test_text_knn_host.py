"""A text query beside knn clauses without a GPU: the arithmetic the kernel compiles (nrtgpu_text_knn_value == plan.h:
text_knn_value) against the NumPy reference (tests/_text_knn_ref.py) bit for bit, the exactness test at its edge, the list checks
that need no device, the struct layouts, and the reference's own hybrid test shape (VectorFieldDefTest.testHybridVectorSearch)
on a synthetic corpus."""
import ctypes as C

import numpy as np
import pytest

from nrtsearch_amd import _lib

from tests import _text_knn_ref as ref

f32, f64 = np.float32, np.float64
TERMS = (1, 2)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def corpus():
    return ref.make_corpus([3000, 1500, 40], [1, 2, 30], delete_fraction=0.01)


def _query(weights=(1.0,), masks=False):
    terms = (_lib.Term * len(weights))()
    for i, w in enumerate(weights):
        terms[i] = _lib.Term(0, 0, i + 1, float(w), 0)
    q = _lib.Bm25Query()
    q.n_terms = len(weights)
    q.terms = terms
    q.k = 10
    q.filter_mask = 3 if masks else 0
    q._keep = terms
    return q


def _clauses(lists, nested=0, n_lists=None, null=False):
    """lists: (docs, scores, boost[, n])."""
    arr = (_lib.DocScores * max(len(lists), 1))()
    keep = []
    for i, l in enumerate(lists):
        docs = None if l[0] is None else np.ascontiguousarray(l[0], dtype=np.int32)
        scores = None if l[1] is None else np.ascontiguousarray(l[1], dtype=np.float32)
        keep += [docs, scores]
        arr[i].docs = None if docs is None else docs.ctypes.data_as(C.POINTER(C.c_int32))
        arr[i].scores = None if scores is None else scores.ctypes.data_as(C.POINTER(C.c_float))
        arr[i].n = l[3] if len(l) > 3 else len(docs)
        arr[i].boost = l[2]
    kc = _lib.KnnClauses()
    kc.lists = None if null else arr
    kc.n_lists = len(lists) if n_lists is None else n_lists
    kc.text_nested = nested
    kc._keep = (arr, keep)
    return kc


def _value(lib, nested, matched, fixed, fx_E, knn_sum):
    out = C.c_float(0)
    rc = lib.nrtgpu_text_knn_value(int(nested), int(matched), int(fixed), int(fx_E), C.c_double(float(knn_sum)), C.byref(out))
    return rc, f32(out.value)


def _scale(lib, oracle, corpus, terms):
    """The query's common fixed-point scale: the largest nrtgpu_fixed_point_scale of its clauses."""
    weights, cache = oracle.bm25_query_stats(corpus, terms)
    max_norm = max(int(np.asarray(s.norms).max()) for s in corpus.segments)
    scales = []
    for w in weights:
        e = C.c_int32(0)
        assert lib.nrtgpu_fixed_point_scale(C.c_float(float(w)), cache.ctypes.data, max_norm, C.byref(e)) == 1
        scales.append(e.value)
    assert max(scales) - min(scales) <= 15
    return max(scales)


def test_struct_sizes():
    assert C.sizeof(_lib.DocScores) == 24
    assert C.sizeof(_lib.KnnClauses) == 16
    assert _lib.NRTGPU_MAX_KNN_LISTS == 8


def test_value_matches_the_reference_in_all_eight_combinations(lib, oracle, corpus):
    fx_E = _scale(lib, oracle, corpus, TERMS)
    matched, text = ref.text_sums(oracle, corpus, TERMS)[0]
    docs = np.nonzero(matched)[0][:200]
    rng = np.random.Generator(np.random.PCG64(5))
    vals = ref.clause_values(rng.random(len(docs)).astype(f32) + f32(0.01), 3.0)
    vals2 = ref.clause_values(rng.random(len(docs)).astype(f32) + f32(0.01), 0.37)
    knn = vals.astype(f64) + vals2.astype(f64)
    checked = 0
    for nested in (0, 1):
        for text_ok in (False, True):
            for listed in (False, True):
                for i, d in enumerate(docs.tolist()):
                    fixed = text[d] * 2.0 ** fx_E
                    assert fixed == int(fixed) and 0 < fixed < 2 ** 52
                    rc, got = _value(lib, nested, text_ok, int(fixed) if text_ok else 0, fx_E, knn[i] if listed else 0.0)
                    if not text_ok and not listed:
                        assert rc == _lib.NRTGPU_ERR_INVALID_ARG   # no hit: no score
                        continue
                    exp = ref.combine(text[d: d + 1], np.array([text_ok]), knn[i: i + 1], np.array([listed]), bool(nested))[0]
                    assert rc == 0 and got.view(np.uint32) == exp.view(np.uint32), (nested, text_ok, listed, d, got, exp)
                    checked += 1
    assert checked == 6 * len(docs)
    # text only is the float nrtgpu_search_bm25 scores; lists only is the float of the double sum
    rc, got = _value(lib, 1, 1, int(text[docs[0]] * 2.0 ** fx_E), fx_E, 0.0)
    assert got == f32(text[docs[0]])
    rc, got = _value(lib, 0, 0, 0, fx_E, knn[0])
    assert got == f32(knn[0])


def test_flat_and_nested_differ_somewhere(lib, oracle, corpus):
    """The two forms are different arithmetic: over the corpus' text sums and a spread of list values the reference alone finds
    pairs where they round apart, and the library gives the reference's bits in both forms there."""
    fx_E = _scale(lib, oracle, corpus, TERMS)
    found = []
    rng = np.random.Generator(np.random.PCG64(11))
    for matched, text in ref.text_sums(oracle, corpus, TERMS):
        docs = np.nonzero(matched)[0]
        knn = ref.clause_values(rng.random(len(docs)).astype(f32) + f32(0.01), 50.0).astype(f64)
        yes = np.ones(len(docs), dtype=bool)
        flat = ref.combine(text[docs], yes, knn, yes, False)
        nest = ref.combine(text[docs], yes, knn, yes, True)
        for i in np.nonzero(flat.view(np.uint32) != nest.view(np.uint32))[0].tolist():
            found.append((text[docs[i]], knn[i], flat[i], nest[i]))
    assert len(found) >= 1, "the reference finds no value pair on which FLAT and NESTED differ"
    for t, ks, flat, nest in found[:50]:
        fixed = int(t * 2.0 ** fx_E)
        assert _value(lib, 0, 1, fixed, fx_E, ks)[1].view(np.uint32) == flat.view(np.uint32)
        assert _value(lib, 1, 1, fixed, fx_E, ks)[1].view(np.uint32) == nest.view(np.uint32)


def test_exactness_at_its_edge(lib):
    """hi = ceil(log2(1 + x)) = 1, lo = floor(log2 x) - 23: x = 2^-29 gives hi - lo == 53 and passes, one binade below fails."""
    q = _query((1.0,))
    assert lib.nrtgpu_text_knn_exact(C.byref(q), C.byref(_clauses([([5], [2.0 ** -29], 1.0)])), 20) == 1
    assert lib.nrtgpu_text_knn_exact(C.byref(q), C.byref(_clauses([([5], [2.0 ** -30], 1.0)])), 20) == 0
    # the boost is part of the value; just below the binade's edge still passes
    assert lib.nrtgpu_text_knn_exact(C.byref(q), C.byref(_clauses([([5], [2.0 ** -28], 0.5)])), 20) == 1
    assert lib.nrtgpu_text_knn_exact(C.byref(q), C.byref(_clauses([([5], [np.nextafter(f32(2.0 ** -29), f32(0))], 1.0)])), 20) == 0
    # the text side's grain can be the smaller one: fx_E = 52 with values around 2 fails on hi = 2
    assert lib.nrtgpu_text_knn_exact(C.byref(q), C.byref(_clauses([([5], [0.75], 1.0)])), 52) == 1
    assert lib.nrtgpu_text_knn_exact(C.byref(q), C.byref(_clauses([([5], [1.5], 1.0)])), 52) == 0
    # every list adds its largest value to hi
    assert lib.nrtgpu_text_knn_exact(C.byref(q), C.byref(_clauses([([5], [0.75], 1.0), ([6], [0.75], 1.0)])), 52) == 0
    # no list entries: the text query alone
    assert lib.nrtgpu_text_knn_exact(C.byref(q), C.byref(_clauses([])), 52) == 1
    assert lib.nrtgpu_text_knn_exact(C.byref(q), C.byref(_clauses([([], [], 1.0)])), 52) == 1


def test_list_checks_need_no_device(lib):
    q = _query((1.0,))
    bad = _lib.NRTGPU_ERR_INVALID_ARG

    def rc(kc, query=q):
        r = lib.nrtgpu_text_knn_exact(C.byref(query), C.byref(kc), 20)
        return r, lib.nrtgpu_last_error().decode()

    cases = {
        "n_lists above the cap": _clauses([([1], [1.0], 1.0)], n_lists=9),
        "n_lists negative": _clauses([([1], [1.0], 1.0)], n_lists=-1),
        "lists NULL": _clauses([([1], [1.0], 1.0)], null=True),
        "n above NRTGPU_MAX_K": _clauses([([1], [1.0], 1.0, 1025)]),
        "n negative": _clauses([([1], [1.0], 1.0, -1)]),
        "docs NULL": _clauses([(None, [1.0], 1.0, 1)]),
        "scores NULL": _clauses([([1], None, 1.0, 1)]),
        "boost 0": _clauses([([1], [1.0], 0.0)]),
        "boost negative": _clauses([([1], [1.0], -2.0)]),
        "boost infinite": _clauses([([1], [1.0], float("inf"))]),
        "boost NaN": _clauses([([1], [1.0], float("nan"))]),
        "score NaN": _clauses([([1, 2], [1.0, float("nan")], 1.0)]),
        "score infinite": _clauses([([1, 2], [float("inf"), 1.0], 1.0)]),
        "a doc twice": _clauses([([7, 3, 7], [1.0, 2.0, 3.0], 1.0)]),
        "text_nested 2": _clauses([([1], [1.0], 1.0)], nested=2),
    }
    for name, kc in cases.items():
        r, msg = rc(kc)
        assert r == bad and msg, name
    r, msg = rc(_clauses([([1], [1.0], 1.0)], nested=0), _query((1.0,), masks=True))
    assert r == bad and "text_nested" in msg
    assert rc(_clauses([([1], [1.0], 1.0)], nested=1), _query((1.0,), masks=True))[0] == 1
    # a clause value the accumulators cannot hold
    for name, kc in {"score 0": _clauses([([1], [0.0], 1.0)]), "score negative": _clauses([([1, 2], [1.0, -0.5], 2.0)]),
                     "value underflows to 0": _clauses([([1], [1e-30], 1e-30)]),
                     "value overflows": _clauses([([1], [1e30], 1e30)])}.items():
        r, msg = rc(kc)
        assert r == _lib.NRTGPU_ERR_UNSUPPORTED and msg, name
    # the same doc in two lists is the point of the thing
    assert rc(_clauses([([7, 3], [1.0, 2.0], 1.0), ([7], [1.0], 1.0)]))[0] == 1
    out = C.c_float(0)
    assert lib.nrtgpu_text_knn_value(2, 1, 5, 0, C.c_double(1.0), C.byref(out)) == bad
    assert lib.nrtgpu_text_knn_value(0, 1, 5, 0, C.c_double(1.0), None) == bad
    assert lib.nrtgpu_text_knn_value(0, 1, 0, 0, C.c_double(1.0), C.byref(out)) == bad
    assert lib.nrtgpu_text_knn_value(0, 1, 5, 0, C.c_double(-1.0), C.byref(out)) == bad


def test_reference_hybrid_test_shape(oracle, corpus):
    """VectorFieldDefTest.testHybridVectorSearch (:844-906) on a synthetic corpus: a term query beside one knn clause with k = 15
    and boost 50, top 30.  The first 15 hits are the listed docs; those holding the term score above the boosted similarity, the
    others exactly the boosted similarity; hits 16-30 hold the term and score below 10."""
    vectors = ref.leaf_vectors(corpus)
    query = np.linspace(-1.0, 1.0, 8).astype(f32)
    term = 2
    ldocs, lscores = ref.knn_list(oracle, corpus, vectors, 0, query, 15, boost=50.0)
    assert len(ldocs) == 15
    docs, scores, total, gte = ref.search(oracle, corpus, [term], 30, lists=[(ldocs, lscores, 1.0)])
    assert len(docs) == 30 and total >= 30
    assert sorted(docs[:15].tolist()) == sorted(ldocs.tolist())
    boosted = dict(zip(ldocs.tolist(), lscores.tolist()))
    holds = {}
    for seg in corpus.segments:
        d, _ = seg.postings(term)
        for x in d.tolist():
            holds[seg.doc_base + x] = True
    n_with = 0
    for d, s in zip(docs[:15].tolist(), scores[:15].tolist()):
        if holds.get(d):
            assert s > boosted[d]
            n_with += 1
        else:
            assert f32(s) == f32(boosted[d])
    assert 0 < n_with < 15, "the corpus must put the term in some of the listed docs and not in others"
    for d, s in zip(docs[15:].tolist(), scores[15:].tolist()):
        assert holds.get(d) and 0 < s < 10 and d not in boosted
    # the same request with the boost left to the clause: the same bits
    unboosted = ref.knn_list(oracle, corpus, vectors, 0, query, 15)
    docs2, scores2, _, _ = ref.search(oracle, corpus, [term], 30, lists=[(unboosted[0], unboosted[1], 50.0)])
    assert docs2.tolist() == docs.tolist() and scores2.view(np.uint32).tolist() == scores.view(np.uint32).tolist()
