"""Run by tests/test_terms_count_host.py in a subprocess with tests/mockhip preloaded (kernels do nothing): the HOST side of the
terms aggregation (nrtgpu_count_terms_batch / nrtgpu_count_terms_supported) -- what plans and runs, and every refusal that needs a
context, with its status.  One line `name status [names the query]` per case on stdout; for a refusal the predicate and the call
must agree, or the line says so.  The kernels' results are not looked at (every table stays empty)."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from nrtsearch_amd import _lib, api   # noqa: E402
from tests import _field_sort_ref as fs   # noqa: E402

L = _lib.load()
COL = 7
T = {t: api.TermQuery(0, t) for t in (1, 2, 3)}
OR3 = api.BooleanQuery((T[1], T[2], T[3]))
top = api.TopScoreDocCollectorManager(10)
INT = api.TermsCollector(COL, 10)


def say(name, rc):
    print(name, rc, flush=True)


def outputs(n, caps, null=False):
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


def both(sr, queries, collectors, max_buckets, managers=None, caps=None, tweak=None, which=0):
    """`status names-the-query` of the call; `status/status` when the predicate on queries[which] disagrees with it."""
    n = len(queries)
    m, tc, bounds = api._marshal_terms(sr, queries, collectors, max_buckets, managers)
    if tweak:
        tweak(m.queries, tc)
    outs = outputs(n, caps if caps is not None else [max(b, 1) for b in bounds])
    rc = L.nrtgpu_count_terms_batch(sr.ctx._h, sr._segs, sr._bases, len(sr.leaves), m.queries, tc, n, outs)
    text = L.nrtgpu_last_error().decode() if rc else ""
    rc2 = L.nrtgpu_count_terms_supported(sr.ctx._h, sr._segs, len(sr.leaves), C.byref(m.queries[which]), C.byref(tc[which]))
    named = int(f"query {which}" in text) if rc else 0
    return f"{rc} {named}" if rc2 == rc else f"{rc}/{rc2} {named}"


corpus = fs.make_corpus([130, 50, 20], {1: 0.6, 2: 0.4, 3: 0.3}, seed=11, delete_fraction=0.05)
rng = np.random.default_rng(12)
columns = [(None, rng.integers(0, 5, size=s.max_doc).astype(np.int32).view(np.uint32)) for s in corpus.segments]
ctx = api.GpuContext(device_id=0, max_batch=512)
leaves = fs.upload(ctx, corpus, "int", columns, column_field=COL)
for leaf in leaves:
    leaf.set_mask(5, np.full((leaf.max_doc + 63) // 64, 2**64 - 1, dtype=np.uint64))
sr = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics.from_corpus(corpus))

say("supported", both(sr, [OR3], [INT], 16))
say("supported_must", both(sr, [api.BooleanQuery((), 0, (), (), (T[1], T[2]))], [INT], 16))
say("supported_msm2_with_mask", both(sr, [api.BooleanQuery((T[1], T[2], T[3]), 2, (api.MaskFilter(5),))], [INT], 16))
say("max_buckets_1", both(sr, [OR3], [INT], 1))
say("max_buckets_65536", both(sr, [OR3], [INT], 65536))
say("the_query_has_after", both(sr, [OR3], [INT], 16, [api.TopScoreDocCollectorManager(10, api.ScoreDoc(3, 1.0))]))
got = api.count_terms_batch(sr, [OR3, T[1], T[2], OR3], [INT] * 4, [16, 1, 65536, 4])
say("batch_of_4", f"{len(got)} {sum(g.total_hits + len(g.counts) + g.hits_with_value + int(g.overflowed) for g in got)}")
d = api.GpuContext.last_diagnostics()
say("diagnostics_items", f"{d['items_maxscore']} {int(d['items_scan'] > 0)}")
st = ctx.stats()
say("stats_counted", int(st["scan_launches"] == st["fixed_point_launches"] and st["scan_launches"] >= 7 and st["maxscore_launches"] == 0 and st["scan_items"] > 0))
say("batch_of_256_at_65536", both(sr, [OR3] * 256, [INT] * 256, 65536))
say("batch_of_257_at_65536", both(sr, [OR3] * 257, [INT] * 257, 65536, which=256))
say("names_the_limit", int("33554432" in L.nrtgpu_last_error().decode() or "2^25" in L.nrtgpu_last_error().decode()))
say("batch_above_max_batch", both(sr, [OR3] * 513, [INT] * 513, 1).split("/")[0])

for name, b in (("max_buckets_0", 0), ("max_buckets_negative", -1), ("max_buckets_65537", 65537)):
    say(name, both(sr, [OR3], [INT], b))
say("capacity_below_max_buckets", both(sr, [OR3], [INT], 16, caps=[15]).split("/")[0])
m, tc, _ = api._marshal_terms(sr, [OR3], [INT], 16, None)
say("null_arrays", L.nrtgpu_count_terms_batch(ctx._h, sr._segs, sr._bases, 3, m.queries, tc, 1, outputs(1, [16], null=True)))
say("k_zero", both(sr, [OR3], [INT], 16, [api.TopScoreDocCollectorManager(0)]))
say("k_2000", both(sr, [OR3], [INT], 16, [api.TopScoreDocCollectorManager(2000)]))
say("no_column_on_any_leaf", both(sr, [OR3], [api.TermsCollector(55, 10)], 16))
say("dismax", both(sr, [api.DisjunctionMaxQuery((T[1], T[2]))], [INT], 16))
say("dismax_tie_breaker", both(sr, [api.DisjunctionMaxQuery((T[1], T[2]), 0.3)], [INT], 16))
say("must_next_to_should", both(sr, [api.BooleanQuery((T[2],), 0, (), (), (T[1],))], [INT], 16))
say("min_competitive_score", both(sr, [OR3], [INT], 16, [api.TopScoreDocCollectorManager(10, None, 1000, 0.5)]))
say("mask_not_resident", both(sr, [api.BooleanQuery((T[1],), 1, (api.MaskFilter(77),))], [INT], 16))
say("must_not_mask_not_resident", both(sr, [api.BooleanQuery((T[1],), 1, (), (api.MaskFilter(78),))], [INT], 16))
say("weights_span_too_many_binades", both(sr, [api.BooleanQuery((T[1], api.BoostQuery(T[2], 2.0 ** -20)))], [INT], 16).split(" ")[0])
# precedence: an invalid argument anywhere in the batch comes before what is merely unsupported
say("invalid_before_unsupported", both(sr, [OR3], [api.TermsCollector(55, 10)], 0))
say("invalid_in_query_1_before_unsupported_in_query_0", both(sr, [api.DisjunctionMaxQuery((T[1], T[2])), OR3], [INT, INT], [16, 0], which=1))
q, t, o = _lib.Bm25Query(), _lib.TermsCount(), _lib.TermCounts()
say("null_queries", L.nrtgpu_count_terms_batch(ctx._h, sr._segs, sr._bases, 3, None, C.byref(t), 1, C.byref(o)))
say("null_terms", L.nrtgpu_count_terms_batch(ctx._h, sr._segs, sr._bases, 3, C.byref(q), None, 1, C.byref(o)))
say("null_out", L.nrtgpu_count_terms_batch(ctx._h, sr._segs, sr._bases, 3, C.byref(q), C.byref(t), 1, None))
say("null_supported", L.nrtgpu_count_terms_supported(ctx._h, sr._segs, 3, None, C.byref(t)))

# leaves that hold the column under different kinds
mixed = []
for seg, kind in zip(corpus.segments, ("int", "float", "int")):
    g = api.GpuSegment(ctx, seg.max_doc, seg.doc_base)
    mixed.append(g)
    g.add_field_norms(0, seg.norms)
    g.add_terms(0, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
    g.add_doc_values(COL, kind, np.zeros(seg.max_doc, dtype=np.uint32))
    g.seal()
sm = api.GpuIndexSearcher(ctx, mixed, api.IndexStatistics.from_corpus(corpus))
say("kinds_differ", both(sm, [T[1]], [INT], 16))
say("kinds_differ_text", int("kinds" in L.nrtgpu_last_error().decode()))
for g in mixed:
    g.release()

for name, flag in (("no_fixed_point", _lib.NRTGPU_FLAG_NO_FIXED_POINT), ("packed_postings", _lib.NRTGPU_FLAG_PACKED_POSTINGS)):
    c2 = api.GpuContext(device_id=0, max_batch=4, flags=flag)
    l2 = fs.upload(c2, corpus, "int", columns, column_field=COL)
    sr2 = api.GpuIndexSearcher(c2, l2, api.IndexStatistics.from_corpus(corpus))
    say("flag_" + name, both(sr2, [OR3], [INT], 16).split(" ")[0])
    for leaf in l2:
        leaf.release()
    c2.close()

say("still_answers", both(sr, [OR3], [INT], 16))
for leaf in leaves:
    leaf.release()
ctx.close()
print("done", flush=True)
