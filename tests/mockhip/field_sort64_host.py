"""Run by tests/test_field_sort64_host.py in a subprocess with tests/mockhip preloaded (kernels do nothing): the HOST side of the
64-bit doc value columns -- nrtgpu_segment_add_doc_values64, the sorted entries over such a column (text and doc-set form) with
their predicates, nrtgpu_segment_set_mask_from_values64, and the 32-bit entries meeting a 64-bit column.  Every refusal that needs
a context with its status, the precedence of the statuses, the fit boundary.  One line `name value` per case on stdout; for the
sorted entries the value is `entry-status predicate-status`.  The kernels' results are not looked at."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from nrtsearch_amd import _lib, api   # noqa: E402
from tests import _field_sort_ref as fs   # noqa: E402

L = _lib.load()
COL, COL32, MCOL, EMPTY, DIFF, WIDE, DCOL = 7, 8, 9, 10, 11, 12, 13
INT64_MIN, INT64_MAX = -2**63, 2**63 - 1
top = api.TopScoreDocCollectorManager(10)
T1, T2 = api.TermQuery(0, 1), api.TermQuery(0, 2)
SORT = api.SortField64(COL, "long")
ALL = api.DocSetQuery()


def say(name, text):
    print(name, text, flush=True)


def err():
    return L.nrtgpu_last_error().decode()


corpus = fs.make_corpus([130, 70], {1: 1.0, 2: 0.5}, seed=11, delete_fraction=0.05)
ctx = api.GpuContext(device_id=0, max_batch=64)


def upload(c, seal=True, diff=("long", "double")):
    leaves = []
    for si, seg in enumerate(corpus.segments):
        n = seg.max_doc
        g = api.GpuSegment(c, n, seg.doc_base)
        g.add_field_norms(0, seg.norms)
        g.add_terms(0, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
        if si == 0:
            g.add_doc_values64(COL, "long", 1_700_000_000_000 + np.arange(0, n, 2, dtype=np.int64), np.arange(0, n, 2, dtype=np.int32))
        else:
            g.add_doc_values64(COL, "long", 1_700_000_000_000 + 2**36 - np.arange(n, dtype=np.int64))
        g.add_doc_values(COL32, "int", np.arange(n, dtype=np.int32))
        g.add_doc_values_multi(MCOL, "int", np.arange(2 * n, dtype=np.int32), np.repeat(np.arange(n, dtype=np.int32), 2))
        g.add_doc_values64(EMPTY, "long", np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int32))
        g.add_doc_values64(DIFF, diff[si], np.zeros(n, dtype=np.uint64))
        wide = np.zeros(n, dtype=np.int64)
        wide[0], wide[1] = INT64_MIN, INT64_MAX
        g.add_doc_values64(WIDE, "long", wide)
        g.add_doc_values64(DCOL, "double", 1.5 + np.arange(n, dtype=np.float64))
        if seal:
            g.seal()
            g.set_mask(5, np.full((n + 63) // 64, 2**64 - 1, dtype=np.uint64))
        leaves.append(g)
    return leaves


# ---- the column ---------------------------------------------------------------------------------------------------------------------
N = 2500
g = api.GpuSegment(ctx, N, 0)
v = np.arange(N, dtype=np.int64)
docs = np.arange(0, 200, 2, dtype=np.int32)


def add(field, kind, n, d, vals):
    return L.nrtgpu_segment_add_doc_values64(g._h, field, kind, n, None if d is None else d.ctypes.data, None if vals is None else vals.ctypes.data)


say("add_kind_0", add(7, 0, N, None, v))
say("add_kind_4", add(7, 4, N, None, v))
say("add_n_negative", add(7, 2, -1, None, v))
say("add_n_too_many", add(7, 2, N + 1, None, np.arange(N + 1, dtype=np.int64)))
say("add_null_docs_short", add(7, 2, 100, None, v))
say("add_null_values", add(7, 2, 100, docs, None))
say("add_docs_descending", add(7, 2, 100, docs[::-1].copy(), v))
say("add_docs_out_of_range", add(7, 2, 100, np.where(docs == 198, N, docs).astype(np.int32), v))
before = g.device_bytes
say("add_ok_sparse", add(7, 2, 100, docs, v))
say("device_bytes_counts_8_per_doc", int(g.device_bytes - before >= 8 * N + N // 8))
say("add_second_64", add(7, 3, N, None, v))
say("add_second_32", L.nrtgpu_segment_add_doc_values(g._h, 7, 0, N, None, np.arange(N, dtype=np.int32).ctypes.data))
say("add_second_multi", L.nrtgpu_segment_add_doc_values_multi(g._h, 7, 0, 0, None, None))
g.add_doc_values(8, "int", np.arange(N, dtype=np.int32))
say("add_64_on_a_32_field", add(8, 2, N, None, v))
say("add_empty_column", add(9, 2, 0, docs, None))
g.seal()
say("add_after_seal", add(10, 2, N, None, v))
g.release()

# ---- the sorted entries -------------------------------------------------------------------------------------------------------------
leaves = upload(ctx)
sr = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics.from_corpus(corpus))


def text(s, queries, sorts, managers=None, afters=None, tweak=None, which=0):
    n = len(queries)
    managers = managers or [top] * n
    m, fsr = api._marshal_sorted64(s, queries, managers, sorts, afters)
    if tweak:
        tweak(m.queries, fsr)
    h = api._Outputs64(managers)
    rc2 = L.nrtgpu_sorted64_supported(s.ctx._h, s._segs, len(s.leaves), C.byref(m.queries[which]), C.byref(fsr[which]))
    rc = L.nrtgpu_search_sorted64_batch(s.ctx._h, s._segs, s._bases, len(s.leaves), m.queries, fsr, n, h.outs)
    return rc, rc2


def docset(s, docsets, sorts, managers=None, afters=None, tweak=None, which=0):
    n = len(docsets)
    managers = managers or [top] * n
    ds, keep = api._marshal_docsets(docsets, managers)
    fsr = api._field_sorts64(sorts, afters, n)
    if tweak:
        tweak(ds, fsr)
    h = api._Outputs64(managers)
    rc2 = L.nrtgpu_docset_sorted64_supported(s.ctx._h, s._segs, len(s.leaves), C.byref(ds[which]), C.byref(fsr[which]))
    rc = L.nrtgpu_search_docset_sorted64_batch(s.ctx._h, s._segs, s._bases, len(s.leaves), ds, fsr, n, h.outs)
    return rc, rc2


def pair(r):
    return f"{r[0]} {r[1]}"


def set_sort(**kw):
    def tweak(_, fsr):
        for k, val in kw.items():
            setattr(fsr[0], k, val)
    return tweak


OR = api.BooleanQuery((T1, T2))
say("text_runs", pair(text(sr, [OR, T1], [SORT, api.SortField64(DCOL, "double", True, float("nan"))])))
say("docset_runs", pair(docset(sr, [ALL, api.DocSetQuery((api.MaskFilter(5),))], [SORT, api.SortField64(DCOL, "double", True, float("inf"))])))
say("text_runs_without_a_value_anywhere", pair(text(sr, [OR], [api.SortField64(EMPTY, "long", False, INT64_MAX)])))
say("reverse_2", pair(text(sr, [OR], [SORT], tweak=set_sort(reverse=2))))
say("has_after_2", pair(text(sr, [OR], [SORT], tweak=set_sort(has_after=2))))
say("after_doc_negative", pair(text(sr, [OR], [SORT], tweak=set_sort(has_after=1, after_doc=-1))))
say("query_has_after", pair(text(sr, [OR], [SORT], [api.TopScoreDocCollectorManager(10, api.ScoreDoc(3, 1.0))])))
say("num_hits_0", pair(text(sr, [OR], [SORT], [api.TopScoreDocCollectorManager(0)])))
say("kinds_differ", pair(text(sr, [OR], [api.SortField64(DIFF, "long")])))
say("kinds_differ_names_them", int("kinds" in err() and "query 0" in err()))
say("no_column", pair(text(sr, [OR], [api.SortField64(55, "long")])))
say("narrow_column", pair(text(sr, [OR], [api.SortField64(COL32, "long")])))
say("narrow_names_the_32_bit_entry", int("nrtgpu_search_sorted_batch" in err() and "query 0" in err()))
say("multi_column", pair(text(sr, [OR], [api.SortField64(MCOL, "long")])))
say("dismax", pair(text(sr, [api.DisjunctionMaxQuery((T1, T2))], [SORT])))
say("must_next_to_should", pair(text(sr, [api.BooleanQuery((T2,), 0, (), (), (T1,))], [SORT])))
say("min_competitive", pair(text(sr, [OR], [SORT], [api.TopScoreDocCollectorManager(10, None, 1000, 0.5)])))
say("filter_mask_not_resident", pair(text(sr, [api.BooleanQuery((T1,), 1, (api.MaskFilter(77),))], [SORT])))
say("does_not_fit", pair(text(sr, [OR], [api.SortField64(WIDE, "long")])))
say("does_not_fit_says", int("query 0" in err() and f"field {WIDE}" in err() and "span needs 65 bits, 8-bit docids leave 56" in err()))
say("invalid_in_query_1_before_unsupported_in_query_0",
    text(sr, [OR, OR], [api.SortField64(55, "long"), SORT], tweak=lambda q, fsr: setattr(fsr[1], "reverse", 2))[0])

say("docset_reverse_2", pair(docset(sr, [ALL], [SORT], tweak=set_sort(reverse=2))))
say("docset_k_0", pair(docset(sr, [ALL], [SORT], [api.TopScoreDocCollectorManager(0)])))
say("docset_no_column", pair(docset(sr, [ALL], [api.SortField64(55, "long")])))
say("docset_narrow_column", pair(docset(sr, [ALL], [api.SortField64(COL32, "long")])))
say("docset_narrow_names_the_32_bit_entry", int("nrtgpu_search_docset_sorted_batch" in err()))
say("docset_range_32_beside", pair(docset(sr, [api.DocSetQuery(ranges=(api.RangeClause(COL32, "int", 3, 90), api.RangeClause(MCOL, "int", 0, 50)))], [SORT])))


def range_over(field):
    def tweak(ds, _):
        rc = (_lib.RangeClause * 1)(_lib.RangeClause(field, 0, 5, 0))
        tweak.keep = rc
        ds[0].ranges, ds[0].n_ranges = rc, 1
    return tweak


say("docset_range_over_the_64_bit_column", pair(docset(sr, [ALL], [SORT], tweak=range_over(COL))))
say("docset_mask_not_resident", pair(docset(sr, [api.DocSetQuery((api.MaskFilter(77),))], [SORT])))
say("docset_does_not_fit", pair(docset(sr, [ALL], [api.SortField64(WIDE, "long")])))
say("docset_kinds_differ", pair(docset(sr, [ALL], [api.SortField64(DIFF, "long")])))

# ---- the 32-bit entries over a 64-bit column
SORT32 = api.SortField(COL, "int")
m, fsr = api._marshal_sorted(sr, [OR], [top], [SORT32], None)
h = api._text_outputs(1, [top])
rc = L.nrtgpu_search_sorted_batch(ctx._h, sr._segs, sr._bases, 2, m.queries, fsr, 1, C.cast(h.outs, C.POINTER(_lib.FieldDocs)))
say("sorted32_over_64", f"{rc} {L.nrtgpu_sorted_supported(ctx._h, sr._segs, 2, m.queries, fsr)}")
say("sorted32_names_the_entry", int("nrtgpu_search_sorted64_batch" in err()))
for name, fn, sup in (("terms32_over_64", lambda: api.count_terms_batch(sr, [OR], [api.TermsCollector(COL, 10)], 16),
                       lambda: api.count_terms_supported(sr, OR, api.TermsCollector(COL, 10), 16)),
                      ("docset_sorted32_over_64", lambda: api.search_docset_sorted_batch(sr, [ALL], [top], [SORT32]),
                       lambda: api.docset_sorted_supported(sr, ALL, top, SORT32)),
                      ("docset_terms32_over_64", lambda: api.count_docset_terms_batch(sr, [ALL], [api.TermsCollector(COL, 10)], 16),
                       lambda: api.count_docset_terms_supported(sr, ALL, api.TermsCollector(COL, 10), 16)),
                      ("docset_range32_over_64", lambda: api.search_docset_sorted_batch(sr, [api.DocSetQuery(ranges=(api.RangeClause(COL, "int", 0, 5),))], [top],
                                                                                        [api.SortField(COL32, "int")]),
                       lambda: api.docset_sorted_supported(sr, api.DocSetQuery(ranges=(api.RangeClause(COL, "int", 0, 5),)), top, api.SortField(COL32, "int")))):
    try:
        fn()
        rc = 0
    except _lib.NrtGpuError as e:
        rc = e.code
        text_of = str(e)
    say(name, f"{rc} {_lib.NRTGPU_ERR_UNSUPPORTED if sup() is False else 0}")
    if name == "terms32_over_64":
        say("terms32_says_buckets", int("64-bit buckets are not built" in text_of))
vc32 = (_lib.ValueClause * 1)()
vc32[0].kind, vc32[0].field_id = _lib.NRTGPU_CLAUSE_EXISTS, COL
say("mask32_over_64", L.nrtgpu_segment_set_mask_from_values(leaves[0]._h, 30, vc32, 1, None))
say("mask32_names_the_entry", int("nrtgpu_segment_set_mask_from_values64" in err()))

# ---- the fit boundary: a leaf at doc base 2^30 with 3000 docs -- db = 31 leaves 33 bits; and with the leaf at base 0 (the bases the
# predicate derives): db = 12 leaves 52
bcorpus = fs.make_corpus([3000], {1: 1.0}, seed=12)
bseg = bcorpus.segments[0]
for base, vb, tag in ((2**30, 33, "boundary"), (0, 52, "inorder_boundary")):
    b = api.GpuSegment(ctx, 3000, base)
    b.add_field_norms(0, bseg.norms)
    b.add_terms(0, bseg.term_ids, bseg.offsets, bseg.docids, bseg.freqs)
    for field, span in ((20, 2**vb - 4), (21, 2**vb - 3)):
        col = np.full(3000, -17, dtype=np.int64)
        col[2999] = -17 + span
        b.add_doc_values64(field, "long", col)
    b.seal()
    bs = api.GpuIndexSearcher(ctx, [b], api.IndexStatistics.from_corpus(bcorpus))
    if base:   # the predicate has no doc bases: it answers for the leaves in order (include/nrtgpu.h), where both columns fit
        say(f"{tag}_span_fits", text(bs, [T1], [api.SortField64(20, "long")])[0])
        r = text(bs, [T1], [api.SortField64(21, "long")])
        say(f"{tag}_span_plus_one", r[0])
        say(f"{tag}_says", int(f"span needs {vb + 1} bits, 31-bit docids leave 33" in err()))
        say(f"{tag}_predicate_answers_for_in_order_bases", r[1])
        say(f"{tag}_docset_fits", docset(bs, [ALL], [api.SortField64(20, "long")])[0])
        say(f"{tag}_docset_plus_one", docset(bs, [ALL], [api.SortField64(21, "long")])[0])
    else:
        say(f"{tag}_span_fits", pair(text(bs, [T1], [api.SortField64(20, "long")])))
        say(f"{tag}_span_plus_one", pair(text(bs, [T1], [api.SortField64(21, "long")])))
        say(f"{tag}_docset_fits", pair(docset(bs, [ALL], [api.SortField64(20, "long")])))
        say(f"{tag}_docset_plus_one", pair(docset(bs, [ALL], [api.SortField64(21, "long")])))
    b.release()

# ---- masks from 64-bit columns ---------------------------------------------------------------------------------------------------------
VC = api.ValueClause64
g0 = leaves[0]
WORDS = (g0.max_doc + 63) // 64
count = C.c_int64(-1)


def raw(hnd, mask_id, clauses, n=None, out=True):
    vc = None
    if clauses is not None:
        vc = (_lib.ValueClause64 * max(len(clauses), 1))(*[_lib.ValueClause64(*c) for c in clauses])
    return L.nrtgpu_segment_set_mask_from_values64(hnd, mask_id, vc, len(clauses) if n is None else n, C.byref(count) if out else None)


RANGE, EXISTS = _lib.NRTGPU_CLAUSE_RANGE, _lib.NRTGPU_CLAUSE_EXISTS
ok_range = (RANGE, COL, 3, 9, 0)
say("mask_range", f"{g0.set_mask_from_values64(20, [VC.range_(COL, 'long', 1_700_000_000_000, 1_700_000_000_050)])} {int(g0.get_mask(20).any())}")
say("mask_exists", g0.set_mask_from_values64(21, [VC.exists(DCOL)]))
say("mask_two_clauses", g0.set_mask_from_values64(22, [VC.range_(DCOL, 'double', float('-inf'), float('inf')), VC.exists(COL)]))
say("mask_null_out_count", raw(g0._h, 23, [ok_range], out=False))
say("mask_seg_null", raw(None, 5, [ok_range]))
say("mask_clauses_null", raw(g0._h, 5, None, n=1))
say("mask_id_zero", raw(g0._h, 0, [ok_range]))
say("mask_n_zero", raw(g0._h, 5, [ok_range], n=0))
say("mask_n_five", raw(g0._h, 5, [ok_range] * 5))
say("mask_kind_in_set", raw(g0._h, 5, [(_lib.NRTGPU_CLAUSE_IN_SET, COL, 0, 0, 0)]))
say("mask_kind_negative", raw(g0._h, 5, [(-1, COL, 0, 0, 0)]))
say("mask_reserved", raw(g0._h, 5, [(RANGE, COL, 3, 9, 1)]))
unsealed = upload(ctx, seal=False)
say("mask_unsealed", raw(unsealed[0]._h, 5, [ok_range]))
say("mask_invalid_before_unsealed", raw(unsealed[0]._h, 5, [(2, COL, 0, 0, 0)]))
say("mask_unsealed_before_unsupported", raw(unsealed[0]._h, 5, [(RANGE, 55, 0, 0, 0)]))
for u in unsealed:
    u.release()
say("mask64_column_not_resident", raw(g0._h, 5, [(RANGE, 55, 0, 0, 0)]))
say("mask_over_a_32_bit_column", raw(g0._h, 5, [(RANGE, COL32, 0, 0, 0)]))
say("mask_names_the_32_bit_entry", int("nrtgpu_segment_set_mask_from_values" in err() and "values64" not in err()))
say("mask_over_a_multi_column", raw(g0._h, 5, [(EXISTS, MCOL, 0, 0, 0)]))
say("mask_invalid_in_clause_1_first", raw(g0._h, 5, [(RANGE, 55, 0, 0, 0), (RANGE, COL, 0, 0, 1)]))
pattern = np.arange(1, WORDS + 1, dtype=np.uint64) * np.uint64(0x0101010101010101)
g0.set_mask(6, pattern)
rc = raw(g0._h, 6, [(RANGE, 55, 0, 0, 0)])
say("mask_failed_call_keeps_the_old", f"{int(rc != 0)} {int(np.array_equal(g0.get_mask(6), pattern))}")
before = g0.device_bytes
g0.set_mask_from_values64(24, [VC.exists(COL)])
say("mask_device_bytes_unchanged", int(g0.device_bytes == before))
for leaf in leaves:
    leaf.set_mask_from_values64(40, [VC.range_(COL, "long", 0, INT64_MAX)])
say("mask_usable_as_a_filter", pair(text(sr, [api.BooleanQuery((T1,), 1, (api.MaskFilter(40),))], [SORT])))

for leaf in leaves:
    leaf.release()
ctx.close()
print("done", flush=True)
