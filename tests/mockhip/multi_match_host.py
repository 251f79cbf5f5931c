"""Run by tests/test_multi_match_host.py in a subprocess with tests/mockhip preloaded (kernels do nothing): the HOST side of
multi-match queries (nrtgpu_search_multi_match_batch / nrtgpu_multi_match_supported) -- what plans and runs, and every refusal that
needs a context, with its status.  One line `name status` per case on stdout; the kernels' results are not looked at."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from nrtsearch_amd import _lib, api   # noqa: E402
from tests import _multi_match_ref as ref   # noqa: E402

L = _lib.load()
fields = ref.build_index()
top = api.TopScoreDocCollectorManager(10)
CROSS = ref.cross_fields_groups((2, 4, 7))
BEST = ref.best_fields_groups((2, 4, 7))


def say(name, rc):
    print(name, rc, flush=True)


def status(call):
    try:
        call()
        return 0
    except api.NrtGpuError as e:
        return e.code


def supported_rc(sr, query, mgr=top, tweak=None):
    m, gs = sr._marshal_multi_match([query], [mgr])
    if tweak:
        tweak(m.queries[0], gs[0])
    return L.nrtgpu_multi_match_supported(sr.ctx._h, sr._segs, len(sr.leaves), m.queries, gs)


ctx = api.GpuContext(device_id=0, max_batch=4)
leaves, stats = ref.upload(api, ctx, fields)
for extra in (3, 4):   # two more scored fields for the "more than four" case: statistics only, no leaf holds them
    stats.fields[extra] = stats.fields[0]
    stats.doc_freq[(extra, 2)] = stats.doc_freq[(0, 2)]
sr = api.GpuIndexSearcher(ctx, leaves, stats)

say("cross_supported", supported_rc(sr, ref.to_query(api, CROSS, "cross_fields", "should", 2, 0.3)))
say("best_supported", supported_rc(sr, ref.to_query(api, BEST, "best_fields", "should", (1, 2), 0.3)))
say("best_must_supported", supported_rc(sr, ref.to_query(api, BEST, "best_fields", "must", 0, 0.3)))
say("escape_terms_supported", supported_rc(sr, ref.to_query(api, ref.cross_fields_groups((1, 12, 13), (0, 1, 2)), "cross_fields", "should", 0, 1.0)))
say("msm_above_n_groups", supported_rc(sr, ref.to_query(api, CROSS, "cross_fields", "should", 9, 0.0)))
say("term_nowhere", supported_rc(sr, ref.to_query(api, ref.cross_fields_groups((2, ref.TERM_NOWHERE)), "cross_fields", "must")))
say("search_cross", status(lambda: sr.search_multi_match_batch([ref.to_query(api, CROSS, "cross_fields", "should", 0, 0.3)], [top])))
say("search_batch_of_4", status(lambda: sr.search_multi_match_batch([ref.to_query(api, BEST, "best_fields", "should", 0, 0.3),
                                                                       ref.to_query(api, CROSS, "cross_fields", "must")] * 2, [top] * 4)))
say("search_batch_above_max_batch", status(lambda: sr.search_multi_match_batch([ref.to_query(api, CROSS, "cross_fields")] * 5, [top] * 5)))
d = api.GpuContext.last_diagnostics()
say("diagnostics_items", f"{d['items_maxscore']} {int(d['items_scan'] > 0)}")
st = ctx.stats()
say("stats_counted", int(st["scan_launches"] == 2 and st["fixed_point_launches"] == 2 and st["maxscore_launches"] == 0 and st["scan_items"] > 0))

cross = ref.to_query(api, CROSS, "cross_fields", "should", 0, 0.3)
say("disjunction_max_set", supported_rc(sr, cross, tweak=lambda q, g: setattr(q, "disjunction_max", 1)))
say("query_tie_breaker_set", supported_rc(sr, cross, tweak=lambda q, g: setattr(q, "tie_breaker", 0.3)))
say("min_competitive_score", supported_rc(sr, cross, api.TopScoreDocCollectorManager(10, None, 1000, 0.5)))
say("mask_not_resident", supported_rc(sr, ref.to_query(api, CROSS, "cross_fields", filter=(7,))))
say("must_not_mask_not_resident", supported_rc(sr, ref.to_query(api, CROSS, "cross_fields", must_not=(7,))))
say("five_fields", supported_rc(sr, ref.to_query(api, ref.cross_fields_groups((2,), (0, 1, 2, 3, 4)), "cross_fields")))
say("33_clauses", supported_rc(sr, ref.to_query(api, [[(0, 1 + i % 12, 1.0) for i in range(33)]], "best_fields")))
say("32_clauses", supported_rc(sr, ref.to_query(api, [[(i % 3, 1 + i % 12, 1.0) for i in range(32)]], "best_fields")))
say("weights_span_too_many_binades", supported_rc(sr, ref.to_query(api, [[(0, 2, 1.0), (1, 2, 2.0 ** -20)], [(0, 4, 1.0)]], "cross_fields")))
say("mixed_group", supported_rc(sr, ref.to_query(api, BEST, "best_fields", "must"), tweak=lambda q, g: setattr(q.terms[1], "occur", 0)))
say("k_zero", supported_rc(sr, cross, api.TopScoreDocCollectorManager(0)))
say("null_groups", L.nrtgpu_multi_match_supported(ctx._h, sr._segs, len(leaves), sr._marshal_multi_match([cross], [top])[0].queries, None))

for name, flag in (("no_fixed_point", _lib.NRTGPU_FLAG_NO_FIXED_POINT), ("packed_postings", _lib.NRTGPU_FLAG_PACKED_POSTINGS)):
    c2 = api.GpuContext(device_id=0, max_batch=4, flags=flag)
    l2, s2 = ref.upload(api, c2, fields)
    sr2 = api.GpuIndexSearcher(c2, l2, s2)
    say("flag_" + name, supported_rc(sr2, cross))
    say("flag_" + name + "_search", status(lambda: sr2.search_multi_match_batch([cross], [top])))
    for leaf in l2:
        leaf.release()
    c2.close()

for leaf in leaves:
    leaf.release()
ctx.close()
print("done", flush=True)
