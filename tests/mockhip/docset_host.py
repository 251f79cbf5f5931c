"""Run by tests/test_docset_host.py in a subprocess with tests/mockhip preloaded (kernels do nothing): the HOST side of the doc-set
requests (nrtgpu_search_docset_sorted_batch / nrtgpu_count_docset_terms_batch and their predicates) -- what plans and runs, and
every refusal that needs a context, with its status.  One line `name sorted | counted` per case on stdout, each half
`status names-the-query`; for a refusal the predicate and the call must agree, or the half says `status/status`.  The kernels'
results are not looked at."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from nrtsearch_amd import _lib, api   # noqa: E402
from tests import _field_sort_ref as fs   # noqa: E402

L = _lib.load()
COL, COL2, FCOL = 7, 8, 9
top = api.TopScoreDocCollectorManager(10)
SORT = api.SortField(COL, "int")
INT = api.TermsCollector(COL, 10)
ALL = api.DocSetQuery()


def say(name, text):
    print(name, text, flush=True)


def field_outputs(n, caps):
    width = max(max(caps), 1)
    docs, bits = np.zeros((n, width), np.int32), np.zeros((n, width), np.uint32)
    outs = (_lib.FieldDocs * n)()
    for qi in range(n):
        outs[qi].capacity = caps[qi]
        outs[qi].docs = C.cast(docs.ctypes.data + qi * width * 4, C.POINTER(C.c_int32))
        outs[qi].value_bits = C.cast(bits.ctypes.data + qi * width * 4, C.POINTER(C.c_uint32))
    outs._rows = (docs, bits)
    return outs


def count_outputs(n, caps, null=False):
    width = max(max(caps), 1)
    bits, counts = np.zeros((n, width), np.uint32), np.zeros((n, width), np.int32)
    outs = (_lib.TermCounts * n)()
    for qi in range(n):
        outs[qi].capacity = caps[qi]
        if not null:
            outs[qi].value_bits = C.cast(bits.ctypes.data + qi * width * 4, C.POINTER(C.c_uint32))
            outs[qi].counts = C.cast(counts.ctypes.data + qi * width * 4, C.POINTER(C.c_int32))
    outs._rows = (bits, counts)
    return outs


def half(rc, rc2, which):
    text = L.nrtgpu_last_error().decode() if rc else ""   # (the batch call came last)
    named = int(f"query {which}" in text) if rc else 0
    return f"{rc} {named}" if rc2 == rc else f"{rc}/{rc2} {named}"


def sorted_half(sr, docsets, managers=None, sorts=None, afters=None, tweak=None, which=0):
    n = len(docsets)
    managers = managers or [top] * n
    ds, keep = api._marshal_docsets(docsets, managers)
    fsr = api._docset_sorts(sorts or [SORT] * n, afters, n)
    if tweak:
        tweak(ds, fsr)
    rc2 = L.nrtgpu_docset_sorted_supported(sr.ctx._h, sr._segs, len(sr.leaves), C.byref(ds[which]), C.byref(fsr[which]))
    rc = L.nrtgpu_search_docset_sorted_batch(sr.ctx._h, sr._segs, sr._bases, len(sr.leaves), ds, fsr, n, field_outputs(n, [max(m.num_hits, 1) for m in managers]))
    return half(rc, rc2, which)


def counted_half(sr, docsets, managers=None, collectors=None, max_buckets=16, caps=None, tweak=None, which=0):
    n = len(docsets)
    ds, keep, tc, bounds = api._docset_terms(docsets, collectors or [INT] * n, max_buckets, managers)
    if tweak:
        tweak(ds, tc)
    rc2 = L.nrtgpu_count_docset_terms_supported(sr.ctx._h, sr._segs, len(sr.leaves), C.byref(ds[which]), C.byref(tc[which]))
    rc = L.nrtgpu_count_docset_terms_batch(sr.ctx._h, sr._segs, sr._bases, len(sr.leaves), ds, tc, n, count_outputs(n, caps if caps is not None else [max(b, 1) for b in bounds]))
    return half(rc, rc2, which)


def both(sr, docsets, managers=None, tweak=None, which=0):
    return f"{sorted_half(sr, docsets, managers, tweak=tweak, which=which)} | {counted_half(sr, docsets, managers, tweak=tweak, which=which)}"


corpus = fs.make_corpus([130, 50, 20], {1: 1.0}, seed=11, delete_fraction=0.05)
rng = np.random.default_rng(12)
ctx = api.GpuContext(device_id=0, max_batch=512)


def upload(c, kinds=("int", "int", "int"), seal=True):
    leaves = []
    for seg, kind in zip(corpus.segments, kinds):
        g = api.GpuSegment(c, seg.max_doc, seg.doc_base)
        g.add_field_norms(0, seg.norms)
        g.add_terms(0, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
        g.add_doc_values(COL, kind, np.zeros(seg.max_doc, dtype=np.uint32))
        g.add_doc_values(COL2, "int", np.arange(seg.max_doc, dtype=np.uint32))
        g.add_doc_values(FCOL, "float", np.zeros(seg.max_doc, dtype=np.uint32))
        if seal:
            g.seal()
            for mid in (5, 6, 11, 12, 13, 14, 15, 16, 17):
                g.set_mask(mid, np.full((g.max_doc + 63) // 64, 2**64 - 1, dtype=np.uint64))
        leaves.append(g)
    return leaves


leaves = upload(ctx)
sr = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics.from_corpus(corpus))
R = api.RangeClause
MF = api.MaskFilter

say("match_all", both(sr, [ALL]))
say("masks", both(sr, [api.DocSetQuery((MF(5), MF(11)), (MF(6),))]))
say("four_ranges", both(sr, [api.DocSetQuery((), (), (R(COL, "int", -5, 5), R(FCOL, "float", -np.inf, np.inf), R(COL2, "int", 0, 100), R(COL, "int", 0, 0)))]))
say("empty_range", both(sr, [api.DocSetQuery((), (), (R(COL, "int", 5, -5),))]))
say("k_1024", both(sr, [ALL], [api.TopScoreDocCollectorManager(1024)]))
say("threshold_int_max", both(sr, [ALL], [api.TopScoreDocCollectorManager(10, None, 2**31 - 1)]))
say("eight_masks", both(sr, [api.DocSetQuery(tuple(MF(m) for m in (5, 11, 12, 13, 14, 15, 16, 17)), tuple(MF(m) for m in (6, 11, 12, 13, 14, 15, 16, 17)))]))
ctx.reset_stats()
four = [ALL, api.DocSetQuery((MF(5),)), api.DocSetQuery((), (), (R(COL2, "int", 3, 9),)), ALL]
got_s = api.search_docset_sorted_batch(sr, four, [top] * 4, [SORT] * 4)
d = api.GpuContext.last_diagnostics()
got_c = api.count_docset_terms_batch(sr, four, [INT] * 4, [16, 1, 65536, 4])
say("batch_of_4", f"{len(got_s)} {sum(g.total_hits + len(g.docs) for g in got_s)} | {len(got_c)} {sum(g.total_hits + len(g.counts) + g.hits_with_value + int(g.overflowed) for g in got_c)}")
say("diagnostics", f"{d['items_maxscore']} {int(d['items_scan'] >= 4)} {d['postings']}")
st = ctx.stats()
say("stats_counted", int(st["scan_launches"] == 2 and st["maxscore_launches"] == 0 and st["scan_items"] >= 8 and st["scan_postings"] == 0))
say("plan_items", int(d["items_scan"] == 4))   # 200 docs: one item per query

for name, k in (("k_zero", 0), ("k_1025", 1025)):
    say(name, both(sr, [ALL], [api.TopScoreDocCollectorManager(k)]))
say("threshold_negative", both(sr, [ALL], [api.TopScoreDocCollectorManager(10, None, -1)]))
one = api.DocSetQuery((), (), (R(COL, "int", 0, 0),))


def set_field(name, value, of_clause=False):
    def tweak(ds, _):
        setattr(ds[0].ranges[0] if of_clause else ds[0], name, value)
    return tweak


say("n_ranges_5", both(sr, [one], tweak=set_field("n_ranges", 5)))
say("n_ranges_negative", both(sr, [one], tweak=set_field("n_ranges", -1)))
say("ranges_null", both(sr, [ALL], tweak=set_field("n_ranges", 1)))
say("clause_reserved", both(sr, [one], tweak=set_field("reserved", 1, True)))
say("query_reserved", both(sr, [ALL], tweak=set_field("reserved", 1)))
say("mask_negative", both(sr, [ALL], tweak=set_field("filter_mask", -1)))
say("n_more_negative", both(sr, [ALL], tweak=set_field("n_more_must_not", -1)))
say("more_null", both(sr, [ALL], tweak=set_field("n_more_filters", 1)))
say("nine_masks", both(sr, [api.DocSetQuery(tuple(MF(m) for m in (5, 6, 11, 12, 13, 14, 15, 16, 17)))]))
say("more_id_zero", both(sr, [api.DocSetQuery((MF(5), MF(0)))]))

say("reverse_2", sorted_half(sr, [ALL], tweak=lambda ds, f: setattr(f[0], "reverse", 2)))
say("has_after_2", sorted_half(sr, [ALL], tweak=lambda ds, f: setattr(f[0], "has_after", 2)))
say("after_doc_negative", sorted_half(sr, [ALL], afters=[api.FieldDoc(-1, 0)]))
say("max_buckets_0", counted_half(sr, [ALL], max_buckets=0))
say("max_buckets_65537", counted_half(sr, [ALL], max_buckets=65537))
say("capacity_below_max_buckets", counted_half(sr, [ALL], caps=[15]).split("/")[0])
ds, keep, tc, _ = api._docset_terms([ALL], [INT], 16, None)
say("null_arrays", L.nrtgpu_count_docset_terms_batch(ctx._h, sr._segs, sr._bases, 3, ds, tc, 1, count_outputs(1, [16], null=True)))
say("batch_of_257_at_65536", counted_half(sr, [ALL] * 257, max_buckets=65536, which=256))
say("names_the_limit", int("33554432" in L.nrtgpu_last_error().decode() or "2^25" in L.nrtgpu_last_error().decode()))

say("no_column_on_any_leaf", f"{sorted_half(sr, [ALL], sorts=[api.SortField(55, 'int')])} | {counted_half(sr, [ALL], collectors=[api.TermsCollector(55, 10)])}")
say("range_column_on_no_leaf", both(sr, [api.DocSetQuery((), (), (R(COL, "int", 0, 0), R(55, "int", 0, 0)))]))
say("mask_not_resident", both(sr, [api.DocSetQuery((MF(77),))]))
say("must_not_mask_not_resident", both(sr, [api.DocSetQuery((), (MF(78),))]))
say("more_mask_not_resident", both(sr, [api.DocSetQuery((MF(5), MF(79)))]))
# precedence: an invalid argument anywhere in the batch comes before what is merely unsupported
say("invalid_before_unsupported", both(sr, [api.DocSetQuery((MF(77),))], [api.TopScoreDocCollectorManager(0)]))
say("invalid_in_query_1_before_unsupported_in_query_0", both(sr, [api.DocSetQuery((MF(77),)), ALL], [top, api.TopScoreDocCollectorManager(0)], which=1))

dq, s, t, fo, to = _lib.DocsetQuery(), _lib.FieldSort(), _lib.TermsCount(COL, 16), _lib.FieldDocs(), _lib.TermCounts()
dq.k = 1
h, sg, bs = ctx._h, sr._segs, sr._bases
say("null_docsets", f"{L.nrtgpu_search_docset_sorted_batch(h, sg, bs, 3, None, C.byref(s), 1, C.byref(fo))} | {L.nrtgpu_count_docset_terms_batch(h, sg, bs, 3, None, C.byref(t), 1, C.byref(to))}")
say("null_records", f"{L.nrtgpu_search_docset_sorted_batch(h, sg, bs, 3, C.byref(dq), None, 1, C.byref(fo))} | {L.nrtgpu_count_docset_terms_batch(h, sg, bs, 3, C.byref(dq), None, 1, C.byref(to))}")
say("null_out", f"{L.nrtgpu_search_docset_sorted_batch(h, sg, bs, 3, C.byref(dq), C.byref(s), 1, None)} | {L.nrtgpu_count_docset_terms_batch(h, sg, bs, 3, C.byref(dq), C.byref(t), 1, None)}")
say("null_supported", f"{L.nrtgpu_docset_sorted_supported(h, sg, 3, None, C.byref(s))} | {L.nrtgpu_count_docset_terms_supported(h, sg, 3, C.byref(dq), None)}")
say("batch_above_max_batch", f"{sorted_half(sr, [ALL] * 513).split('/')[0]} | {counted_half(sr, [ALL] * 513, max_buckets=1).split('/')[0]}")

# leaves that hold a named column under different kinds: the sort's, the count's, a range clause's
mixed = upload(ctx, ("int", "float", "int"))
sm = api.GpuIndexSearcher(ctx, mixed, api.IndexStatistics.from_corpus(corpus))
say("sort_kinds_differ", sorted_half(sm, [ALL]))
say("count_kinds_differ", counted_half(sm, [ALL]))
say("range_kinds_differ", f"{sorted_half(sm, [one], sorts=[api.SortField(COL2, 'int')])} | {counted_half(sm, [one], collectors=[api.TermsCollector(COL2, 10)])}")
say("kinds_differ_text", int("kinds" in L.nrtgpu_last_error().decode()))
for g in mixed:
    g.release()

raw = upload(ctx, seal=False)
su = api.GpuIndexSearcher(ctx, raw, api.IndexStatistics.from_corpus(corpus))
say("unsealed_leaf", f"{sorted_half(su, [ALL]).split(' ')[0]} | {counted_half(su, [ALL]).split(' ')[0]}")
for g in raw:
    g.release()

# the route reads no posting and sums no score: it runs under the two flags the text routes over a column refuse
for name, flag in (("no_fixed_point", _lib.NRTGPU_FLAG_NO_FIXED_POINT), ("packed_postings", _lib.NRTGPU_FLAG_PACKED_POSTINGS)):
    c2 = api.GpuContext(device_id=0, max_batch=4, flags=flag)
    l2 = upload(c2)
    sr2 = api.GpuIndexSearcher(c2, l2, api.IndexStatistics.from_corpus(corpus))
    say("flag_" + name, both(sr2, [api.DocSetQuery((MF(5),), (), (R(COL, "int", 0, 0),))]))
    for leaf in l2:
        leaf.release()
    c2.close()

say("still_answers", both(sr, [ALL]))
for leaf in leaves:
    leaf.release()
ctx.close()
print("done", flush=True)
