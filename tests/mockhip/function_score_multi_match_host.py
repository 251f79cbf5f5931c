"""Run by tests/test_function_score_multi_match_host.py in a subprocess with tests/mockhip preloaded (kernels do nothing): the HOST
side of a function score over multi-match queries (nrtgpu_search_function_score_multi_match_batch /
nrtgpu_function_score_multi_match_supported) -- what plans and runs, and every refusal that needs a context, with its status and
in the header's order.  One line `name status` per case on stdout; the kernels' results are not looked at."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from nrtsearch_amd import _lib, api   # noqa: E402
from tests import _function_score_multi_match_ref as ref   # noqa: E402
from tests import _multi_match_ref as mm_ref   # noqa: E402

L = _lib.load()
fields = mm_ref.build_index()
masks = ref.function_masks(fields)
top = api.TopScoreDocCollectorManager(10)
CROSS = mm_ref.cross_fields_groups((2, 4, 7))
BEST = mm_ref.best_fields_groups((2, 4, 7))
FUNCTIONS = ((7, 1.5), (9, 3.0), (0, 0.5))
FLAT = [[(0, 2, 1.0), (0, 4, 1.0), (0, 7, 1.0)]]


def say(name, rc):
    print(name, rc, flush=True)


def status(call):
    try:
        call()
        return 0
    except api.NrtGpuError as e:
        return e.code


def supported_rc(sr, query, mgr=top, tweak=None):
    m, gs, fs = sr._marshal_function_score_multi_match([query], [mgr])
    if tweak:
        tweak(m.queries[0], gs[0], fs[0])
    return L.nrtgpu_function_score_multi_match_supported(sr.ctx._h, sr._segs, len(sr.leaves), m.queries, gs, fs)


def old_entry_rc(sr, inner):
    q = api.FunctionScoreQuery(inner, tuple(api.WeightFunction(w, m) for m, w in FUNCTIONS))
    m = sr._marshal([q.inner], [top])
    return L.nrtgpu_function_score_supported(sr.ctx._h, sr._segs, len(sr.leaves), m.queries, sr._marshal_function_scores([q], m))


def upload(ctx):
    leaves, stats = mm_ref.upload(api, ctx, fields)
    for (si, mid), bits in masks.items():
        leaves[si].set_mask(mid, bits)
    return leaves, stats


ctx = api.GpuContext(device_id=0, max_batch=4)
leaves, stats = upload(ctx)
for extra in (3, 4):   # two more scored fields for the "more than four" case: statistics only, no leaf holds them
    stats.fields[extra] = stats.fields[0]
    stats.doc_freq[(extra, 2)] = stats.doc_freq[(0, 2)]
sr = api.GpuIndexSearcher(ctx, leaves, stats)

cross = ref.to_query(api, CROSS, "cross_fields", "should", 0, 0.3, FUNCTIONS)
say("cross_supported", supported_rc(sr, ref.to_query(api, CROSS, "cross_fields", "should", 2, 0.3, FUNCTIONS, "sum", "sum", 1.0, True)))
say("best_supported", supported_rc(sr, ref.to_query(api, BEST, "best_fields", "should", (1, 2), 0.3, FUNCTIONS, "multiply", "replace")))
say("best_must_supported", supported_rc(sr, ref.to_query(api, BEST, "best_fields", "must", 0, 0.3, FUNCTIONS)))
say("no_functions_supported", supported_rc(sr, ref.to_query(api, CROSS, "cross_fields", "should", 0, 0.3)))
say("eight_functions_supported", supported_rc(sr, ref.to_query(api, CROSS, "cross_fields", "should", 0, 0.3, ((7, 1.5), (9, 3.0), (0, 0.5), (7, 2.0)) * 2)))
# the flat shapes the function-score entry refuses, one group each
t = [api.TermQuery(0, 2), api.TermQuery(0, 4), api.TermQuery(0, 7)]
say("flat_must_supported", supported_rc(sr, ref.to_query(api, FLAT, "best_fields", "must", 0, 0.0, FUNCTIONS)))
say("flat_msm_supported", supported_rc(sr, ref.to_query(api, FLAT, "best_fields", "should", (2,), 0.0, FUNCTIONS)))
say("flat_dismax_supported", supported_rc(sr, ref.to_query(api, FLAT, "cross_fields", "should", 0, 0.3, FUNCTIONS)))
say("flat_must_old_entry", old_entry_rc(sr, api.BooleanQuery(must=tuple(t))))
say("flat_msm_old_entry", old_entry_rc(sr, api.BooleanQuery(tuple(t), 2)))
say("flat_dismax_old_entry", old_entry_rc(sr, api.DisjunctionMaxQuery(tuple(t), 0.3)))

say("search_cross", status(lambda: sr.search_function_score_multi_match_batch([cross], [top])))
say("search_batch_of_4", status(lambda: sr.search_function_score_multi_match_batch(
    [ref.to_query(api, BEST, "best_fields", "should", 0, 0.3, FUNCTIONS), ref.to_query(api, CROSS, "cross_fields", "must")] * 2, [top] * 4)))
say("search_batch_above_max_batch", status(lambda: sr.search_function_score_multi_match_batch([cross] * 5, [top] * 5)))
d = api.GpuContext.last_diagnostics()
say("diagnostics_items", f"{d['items_maxscore']} {int(d['items_scan'] > 0)}")
st = ctx.stats()
say("stats_counted", int(st["scan_launches"] == 2 and st["fixed_point_launches"] == 2 and st["maxscore_launches"] == 0 and st["scan_items"] > 0))

# 1. what the multi-match entry refuses of (query, groups)
best_must = ref.to_query(api, BEST, "best_fields", "must", 0, 0.3, FUNCTIONS)
say("disjunction_max_set", supported_rc(sr, cross, tweak=lambda q, g, f: setattr(q, "disjunction_max", 1)))
say("query_tie_breaker_set", supported_rc(sr, cross, tweak=lambda q, g, f: setattr(q, "tie_breaker", 0.3)))
say("k_zero", supported_rc(sr, cross, api.TopScoreDocCollectorManager(0)))
m0, gs0, fs0 = sr._marshal_function_score_multi_match([cross], [top])
say("null_groups", L.nrtgpu_function_score_multi_match_supported(ctx._h, sr._segs, len(leaves), m0.queries, None, fs0))
say("null_functions", L.nrtgpu_function_score_multi_match_supported(ctx._h, sr._segs, len(leaves), m0.queries, gs0, None))
say("min_competitive_score", supported_rc(sr, cross, api.TopScoreDocCollectorManager(10, None, 1000, 0.5)))
say("mixed_group", supported_rc(sr, best_must, tweak=lambda q, g, f: setattr(q.terms[1], "occur", 0)))
say("33_clauses", supported_rc(sr, ref.to_query(api, [[(0, 1 + i % 12, 1.0) for i in range(33)]], "best_fields", functions=FUNCTIONS)))
# 2. what the function-score entry refuses of the functions
say("nine_functions", supported_rc(sr, cross, tweak=lambda q, g, f: setattr(f, "n_functions", 9)))
say("weight_zero", supported_rc(sr, ref.to_query(api, CROSS, "cross_fields", functions=((7, 0.0),))))
say("score_mode_2", supported_rc(sr, cross, tweak=lambda q, g, f: setattr(f, "score_mode", 2)))
say("min_score_negative", supported_rc(sr, cross, tweak=lambda q, g, f: setattr(f, "min_score", -1.0)))
say("weight_negative", supported_rc(sr, ref.to_query(api, CROSS, "cross_fields", functions=((7, -2.0),))))
# ... in that order
say("mixed_group_and_weight_zero", supported_rc(sr, ref.to_query(api, BEST, "best_fields", "must", functions=((7, 0.0),)),
                                                tweak=lambda q, g, f: setattr(q.terms[1], "occur", 0)))
say("weight_zero_and_function_mask_not_resident", supported_rc(sr, ref.to_query(api, CROSS, "cross_fields", functions=((33, 0.0),))))
# 4. function masks, 5. the planner
say("function_mask_not_resident", supported_rc(sr, ref.to_query(api, CROSS, "cross_fields", functions=((33, 2.0),))))
leaves[0].set_mask(13, masks[(0, 7)])
say("function_mask_on_one_leaf", supported_rc(sr, ref.to_query(api, CROSS, "cross_fields", functions=((13, 2.0),))))
leaves[0].set_mask(13, None)
say("filter_mask_not_resident", supported_rc(sr, ref.to_query(api, CROSS, "cross_fields", functions=FUNCTIONS, filter=(21,))))
say("five_fields", supported_rc(sr, ref.to_query(api, mm_ref.cross_fields_groups((2,), (0, 1, 2, 3, 4)), "cross_fields", functions=FUNCTIONS)))
say("weights_span_too_many_binades", supported_rc(sr, ref.to_query(api, [[(0, 2, 1.0), (1, 2, 2.0 ** -20)], [(0, 4, 1.0)]], "cross_fields",
                                                                     functions=FUNCTIONS)))

# 3. the context's flags -- before the function masks are looked at
for name, flag in (("no_fixed_point", _lib.NRTGPU_FLAG_NO_FIXED_POINT), ("packed_postings", _lib.NRTGPU_FLAG_PACKED_POSTINGS)):
    c2 = api.GpuContext(device_id=0, max_batch=4, flags=flag)
    l2, s2 = upload(c2)
    sr2 = api.GpuIndexSearcher(c2, l2, s2)
    say("flag_" + name, supported_rc(sr2, cross))
    say("flag_" + name + "_search", status(lambda: sr2.search_function_score_multi_match_batch([cross], [top])))
    if name == "packed_postings":
        supported_rc(sr2, ref.to_query(api, CROSS, "cross_fields", functions=((33, 2.0),)))
        say("flag_before_function_mask", "flags" if "NRTGPU_FLAG" in L.nrtgpu_last_error().decode() else L.nrtgpu_last_error().decode())
    for leaf in l2:
        leaf.release()
    c2.close()

for leaf in leaves:
    leaf.release()
ctx.close()
print("done", flush=True)
