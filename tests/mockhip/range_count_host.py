"""Run by tests/test_range_count_host.py in a subprocess with tests/mockhip preloaded (kernels do nothing): the HOST side of the
numeric range facet -- nrtgpu_count_ranges_batch and nrtgpu_count_docset_ranges_batch with their predicates.  Every refusal that
needs a context with its status, the precedence of the statuses (an invalid argument in query 1 before an unsupported query 0),
predicate == entry on each case, the mixed-width batch, the multi-valued column, the context flags.  One line `name value` per
case on stdout; where a predicate exists the value is `entry-status predicate-status`.  The kernels' results are not looked at."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from nrtsearch_amd import _lib, api   # noqa: E402
from tests import _field_sort_ref as fs   # noqa: E402

L = _lib.load()
COL, COL32, MCOL, DCOL, FCOL, DIFF = 7, 8, 9, 13, 14, 11
T1, T2 = api.TermQuery(0, 1), api.TermQuery(0, 2)
OR = api.BooleanQuery((T1, T2))
ALL = api.DocSetQuery()
R = ((3, 9), (5, 20))
LONG, INT = api.RangeCounter(COL, "long", R), api.RangeCounter(COL32, "int", R)
DOUBLE = api.RangeCounter(DCOL, "double", ((api._value_bits64("double", 1.5), api._value_bits64("double", 9.0)),))
FLOAT = api.RangeCounter(FCOL, "float", ((api._value_bits("float", 1.5), api._value_bits("float", 9.0)),))


def say(name, text):
    print(name, text, flush=True)


def err():
    return L.nrtgpu_last_error().decode()


corpus = fs.make_corpus([130, 70], {1: 1.0, 2: 0.5}, seed=11, delete_fraction=0.05)


def upload(c):
    leaves = []
    for si, seg in enumerate(corpus.segments):
        n = seg.max_doc
        g = api.GpuSegment(c, n, seg.doc_base)
        g.add_field_norms(0, seg.norms)
        g.add_terms(0, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
        g.add_doc_values64(COL, "long", np.arange(n, dtype=np.int64))
        g.add_doc_values(COL32, "int", np.arange(n, dtype=np.int32))
        g.add_doc_values_multi(MCOL, "int", np.arange(2 * n, dtype=np.int32), np.repeat(np.arange(n, dtype=np.int32), 2))
        g.add_doc_values64(DCOL, "double", 1.5 + np.arange(n, dtype=np.float64))
        g.add_doc_values(FCOL, "float", (1.5 + np.arange(n)).astype(np.float32))
        g.add_doc_values64(DIFF, ("long", "double")[si], np.zeros(n, dtype=np.uint64))
        g.seal()
        g.set_mask(5, np.full((n + 63) // 64, 2**64 - 1, dtype=np.uint64))
        leaves.append(g)
    return leaves


ctx = api.GpuContext(device_id=0, max_batch=64)
leaves = upload(ctx)
sr = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics.from_corpus(corpus))


def text(s, queries, counters, managers=None, tweak=None, which=0, predicate=True):
    m = api._marshal_range_queries(s, queries, counters, managers)
    rc, outs, counts, keep = api._marshal_range_counters(counters)
    if tweak:
        tweak(rc, outs)
    r2 = L.nrtgpu_count_ranges_supported(s.ctx._h, s._segs, len(s.leaves), C.byref(m.queries[which]), C.byref(rc[which])) if predicate else None
    r = L.nrtgpu_count_ranges_batch(s.ctx._h, s._segs, s._bases, len(s.leaves), m.queries, rc, len(queries), outs)
    return f"{r} {r2}" if predicate else str(r)


def docset(s, docsets, counters, managers=None, tweak=None, which=0, predicate=True):
    ds, dkeep = api._marshal_docsets(docsets, managers or [api.TopScoreDocCollectorManager(1)] * len(docsets))
    rc, outs, counts, keep = api._marshal_range_counters(counters)
    if tweak:
        tweak(rc, outs)
    r2 = L.nrtgpu_count_docset_ranges_supported(s.ctx._h, s._segs, len(s.leaves), C.byref(ds[which]), C.byref(rc[which])) if predicate else None
    r = L.nrtgpu_count_docset_ranges_batch(s.ctx._h, s._segs, s._bases, len(s.leaves), ds, rc, len(docsets), outs)
    return f"{r} {r2}" if predicate else str(r)


def set_count(qi=0, **kw):
    def tweak(rc, outs):
        for k, v in kw.items():
            setattr(rc[qi], k, v)
    return tweak


def set_out(**kw):
    def tweak(rc, outs):
        for k, v in kw.items():
            setattr(outs[0], k, v)
    return tweak


def null_ranges(rc, outs):
    rc[0].ranges = C.POINTER(_lib.ValueRange)()


def null_counts(rc, outs):
    outs[0].counts = C.POINTER(C.c_int64)()


HIGH = api.RangeCounter(COL32, "int", ((3, 2**32 + 9),))
for tag, run, q, masked, unmasked in (("text", text, OR, api.BooleanQuery((T1,), 1, (api.MaskFilter(77),)), api.BooleanQuery((T1,), 1, (api.MaskFilter(5),))),
                                      ("docset", docset, ALL, api.DocSetQuery((api.MaskFilter(77),)), api.DocSetQuery((api.MaskFilter(5),)))):
    say(f"{tag}_runs_64", run(sr, [q, unmasked], [LONG, DOUBLE]))
    say(f"{tag}_runs_32", run(sr, [q, unmasked], [INT, FLOAT]))
    say(f"{tag}_64_ranges", run(sr, [q], [api.RangeCounter(COL, "long", tuple((i, i + 3) for i in range(64)))]))
    say(f"{tag}_n_ranges_0", run(sr, [q], [LONG], tweak=set_count(n_ranges=0)))
    say(f"{tag}_n_ranges_65", run(sr, [q], [LONG], tweak=set_count(n_ranges=65)))
    say(f"{tag}_n_ranges_says", int("query 0" in err() and "1..64" in err()))
    say(f"{tag}_ranges_null", run(sr, [q], [LONG], tweak=null_ranges))
    say(f"{tag}_high_word_over_32", run(sr, [q], [HIGH]))
    say(f"{tag}_high_word_over_64_is_a_value", run(sr, [q], [api.RangeCounter(COL, "long", ((3, 2**32 + 9),))]))
    say(f"{tag}_capacity_short", run(sr, [q], [LONG], tweak=set_out(capacity=1), predicate=False))
    say(f"{tag}_counts_null", run(sr, [q], [LONG], tweak=null_counts, predicate=False))
    say(f"{tag}_reserved_1", run(sr, [q], [LONG], tweak=set_out(reserved=1), predicate=False))
    say(f"{tag}_num_hits_0", run(sr, [q], [LONG], [api.TopScoreDocCollectorManager(0)]))
    say(f"{tag}_kinds_differ", run(sr, [q], [api.RangeCounter(DIFF, "long", R)]))
    say(f"{tag}_no_column", run(sr, [q], [api.RangeCounter(55, "long", R)]))
    say(f"{tag}_no_column_says", int("query 0" in err() and "field 55" in err()))
    say(f"{tag}_multi_column", run(sr, [q], [api.RangeCounter(MCOL, "int", R)]))
    say(f"{tag}_multi_says", int("query 0" in err() and "multi-valued" in err()))
    say(f"{tag}_mixed_widths", run(sr, [q, q], [LONG, INT], predicate=False))
    say(f"{tag}_mixed_says", int("query 1" in err() and "split" in err()))
    say(f"{tag}_mixed_widths_other_order", run(sr, [q, q, q], [FLOAT, INT, DOUBLE], predicate=False))
    say(f"{tag}_each_width_alone", run(sr, [q], [INT]) + " " + run(sr, [q], [LONG]))
    say(f"{tag}_mask_not_resident", run(sr, [masked], [LONG]))
    say(f"{tag}_invalid_in_query_1_before_unsupported_in_query_0",
        run(sr, [q, q], [api.RangeCounter(55, "long", R), LONG], tweak=set_count(1, n_ranges=0), predicate=False))
    say(f"{tag}_high_word_in_query_1_before_multi_in_query_0", run(sr, [q, q], [api.RangeCounter(MCOL, "int", R), HIGH], predicate=False))
    say(f"{tag}_invalid_in_query_1_before_mixed_widths", run(sr, [q, q, q], [LONG, INT, LONG], tweak=set_count(2, n_ranges=-1), predicate=False))
    say(f"{tag}_multi_before_no_mask", run(sr, [masked], [api.RangeCounter(MCOL, "int", R)]))

# the text entry's own table
say("text_dismax", text(sr, [api.DisjunctionMaxQuery((T1, T2))], [LONG]))
say("text_must_next_to_should", text(sr, [api.BooleanQuery((T2,), 0, (), (), (T1,))], [LONG]))
say("text_min_competitive", text(sr, [OR], [LONG], [api.TopScoreDocCollectorManager(10, None, 1000, 0.5)]))
say("text_num_hits_2000", text(sr, [OR], [LONG], [api.TopScoreDocCollectorManager(2000)]))
say("text_has_after_is_not_read", text(sr, [OR], [LONG], [api.TopScoreDocCollectorManager(10, api.ScoreDoc(3, 1.0), 0)]))
# the doc set's own table
say("docset_k_0", docset(sr, [ALL], [LONG], [api.TopScoreDocCollectorManager(0)]))
say("docset_range_32_beside_a_64_count", docset(sr, [api.DocSetQuery(ranges=(api.RangeClause(COL32, "int", 3, 90), api.RangeClause(MCOL, "int", 0, 50)))], [LONG]))
say("docset_range_over_a_64_bit_column", docset(sr, [api.DocSetQuery(ranges=(api.RangeClause(COL, "int", 0, 5),))], [INT]))

# NULL arguments with a context
q0, r0, o0, d0 = _lib.Bm25Query(), _lib.RangeCount(), _lib.RangeCounts(), _lib.DocsetQuery()
say("null_arguments", " ".join(str(x) for x in (
    L.nrtgpu_count_ranges_batch(ctx._h, sr._segs, sr._bases, 2, None, C.byref(r0), 1, C.byref(o0)),
    L.nrtgpu_count_ranges_batch(ctx._h, sr._segs, sr._bases, 2, C.byref(q0), None, 1, C.byref(o0)),
    L.nrtgpu_count_ranges_batch(ctx._h, sr._segs, sr._bases, 2, C.byref(q0), C.byref(r0), 1, None),
    L.nrtgpu_count_ranges_supported(ctx._h, sr._segs, 2, None, C.byref(r0)),
    L.nrtgpu_count_docset_ranges_batch(ctx._h, sr._segs, sr._bases, 2, None, C.byref(r0), 1, C.byref(o0)),
    L.nrtgpu_count_docset_ranges_batch(ctx._h, sr._segs, sr._bases, 2, C.byref(d0), C.byref(r0), 1, None),
    L.nrtgpu_count_docset_ranges_supported(ctx._h, sr._segs, 2, C.byref(d0), None))))

# the context flags: the text entry refuses both (an invalid argument still comes first), the doc-set entry runs under both
for name, flag in (("no_fixed_point", _lib.NRTGPU_FLAG_NO_FIXED_POINT), ("packed_postings", _lib.NRTGPU_FLAG_PACKED_POSTINGS)):
    c2 = api.GpuContext(device_id=0, max_batch=4, flags=flag)
    l2 = upload(c2)
    s2 = api.GpuIndexSearcher(c2, l2, api.IndexStatistics.from_corpus(corpus))
    say(f"text_{name}", text(s2, [OR], [LONG]))
    say(f"text_{name}_says", int("NRTGPU_FLAG" in err()))
    say(f"text_{name}_invalid_first", text(s2, [OR], [LONG], tweak=set_count(n_ranges=0)))
    say(f"docset_{name}", docset(s2, [ALL], [LONG]) + " " + docset(s2, [ALL], [INT]))
    for leaf in l2:
        leaf.release()
    c2.close()

for leaf in leaves:
    leaf.release()
ctx.close()
print("done", flush=True)
