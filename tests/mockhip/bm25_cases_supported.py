"""Run by tests/test_bm25_cases_host.py in a subprocess with tests/mockhip preloaded (kernels do nothing): nrtgpu_query_supported --
the planner as a predicate -- on every request of tests/_bm25_cases.py's layout sweep, under the default flags, under
NRTGPU_FLAG_NO_PRUNE and under NRTGPU_FLAG_NO_FIXED_POINT, and of its default fuzz rounds under each round's own context.  What
_bm25_cases.refusal says a context takes, the library must take; what it says a context refuses -- the second-accumulator shapes
without the MaxScore route, the clause-counting shapes without the fixed-point sums -- the library must refuse with that message
of the planner's, not another.  One line per index on stdout; argv: the fuzz's seed base and its number of rounds."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from nrtsearch_amd import _lib   # noqa: E402
from tests import _bm25_cases as bc   # noqa: E402
from tests import test_bm25_edges_gpu as edges   # noqa: E402


def verdicts(name, m, reqs, flags, packed=False, budget_pct=0):
    ctx = edges.open_context(m, flags, packed, budget_pct)
    leaves, searcher = edges.upload(ctx, m)
    wrong = []
    for i, r in enumerate(reqs):
        ok = searcher.supported(bc.query_of(r), bc.manager_of(r))
        reason = "" if ok else _lib.load().nrtgpu_last_error().decode("utf-8", "replace")
        want = bc.refusal(r, flags)
        # (planner.cpp refuses a second-accumulator shape only where the query has a part in some leaf: with a MUST term that no leaf
        #  holds it plans to nothing, and what plans to nothing is taken)
        if ok and want == bc.REFUSED_SECOND_ACCUMULATOR and r.mixed_must and m.expected(r)[2] == 0:
            continue
        if ok != (want is None) or (not ok and want not in reason):
            wrong.append(f"request {i} ({bc.describe(r)}): expected {want!r}, the library says {ok} {reason[:120]!r}")
    edges.release(leaves)
    ctx.close()
    print(name, "ok" if not wrong else "WRONG " + "; ".join(wrong[:3]), len(reqs), sum(1 for r in reqs if not bc.taken_by(r, flags)), flush=True)


base, rounds = int(sys.argv[1]), int(sys.argv[2])
for layout in bc.LAYOUTS:
    m, reqs, _ = bc.sweep_case(layout)
    for flags in (0, bc.NO_PRUNE, bc.NO_FIXED_POINT):
        verdicts(f"layout_{layout}_{flags}", m, reqs, flags)
for round_ in range(rounds):
    m, knobs, batches = bc.fuzz_round(base, round_)
    verdicts(f"round_{round_}", m, [r for b in batches for r in b], knobs.flags, knobs.packed, knobs.budget_pct)
print("done", flush=True)
