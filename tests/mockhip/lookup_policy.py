"""Run by tests/test_lookup_policy_host.py in a subprocess with tests/mockhip preloaded and the DEVELOPMENT library loaded
(NRTGPU_LIB_PATH): which lookup structure the seal gives each term (segment.cpp: build_term_aux), read back through
nrtgpu_debug_term_lookup.  Seals only, no search.  One JSON line per case on stdout: what the library answered; the test holds
the expectations."""
import faulthandler
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np   # noqa: E402

from nrtsearch_amd import _lib, api   # noqa: E402
from tests import _lookup_cases as lc   # noqa: E402

faulthandler.dump_traceback_later(240, exit=True)
PACKED = _lib.NRTGPU_FLAG_PACKED_POSTINGS


def context(policy, pct, packed):
    os.environ["NRTGPU_LOOK_POLICY"] = policy      # (the development build reads it at every seal)
    return api.GpuContext(0, max_batch=16, flags=PACKED if packed else 0, lookup_budget_pct=pct)


def report(name, leaves, terms_of):
    rows = [{str(t): list(leaf.debug_term_lookup(0, t)) for t in terms} for leaf, terms in zip(leaves, terms_of)]
    print("CASE", json.dumps({"name": name, "terms": rows, "device_bytes": [leaf.device_bytes for leaf in leaves]}), flush=True)


# ---- the GPU test's corpus under the GPU test's matrix, and the same percentage under the other layout ------------------------
corpus = lc.build_corpus()
terms_of = [[int(t) for t in s.term_ids] for s in corpus.segments]
for case in lc.MATRIX + [lc.Case("small12_packed", lc.DEFAULT_POLICY, 12, True)]:
    ctx = context(case.policy, case.pct, case.packed)
    leaves = [api.GpuSegment.from_data(ctx, s) for s in corpus.segments]
    report(case.name, leaves, terms_of)
    for g in leaves:
        g.release()
    ctx.close()


# ---- boundaries the corpus cannot hold ---------------------------------------------------------------------------------------
def segment(ctx, max_doc, groups, norms=True):
    """groups: one add_terms call each, [(term id, postings)] with the postings spread evenly over the segment."""
    g = api.GpuSegment(ctx, max_doc)
    g.add_field_norms(0, np.full(max_doc, 10, np.uint8) if norms else None)
    for terms in groups:
        offs, docs = [0], []
        for _, c in terms:
            docs.append((np.arange(c, dtype=np.int64) * (max_doc // c)).astype(np.int32))
            offs.append(offs[-1] + c)
        g.add_terms(0, [t for t, _ in terms], offs, np.concatenate(docs), None)
    g.seal()
    return g


def one(name, policy, pct, packed, max_doc, groups, norms=True):
    ctx = context(policy, pct, packed)
    g = segment(ctx, max_doc, groups, norms)
    report(name, [g], [[t for terms in groups for t, _ in terms]])
    g.release()
    ctx.close()


# a posting per 256 docs: count * 256 == max_doc is dense, one posting fewer is not
one("density_equal", lc.DEFAULT_POLICY, 100000, False, 65_536, [[(20, 256), (21, 255)]])
# two terms of one size and a budget for one set of records: the term added first is served first, whatever its id; with a cells
# rule behind the records the second term still gets the cheaper structure
one("tie_bits", "bits", 400, False, 65_536, [[(31, 300), (30, 300)]])
one("tie_bits_cells", "bits,cells", 400, False, 65_536, [[(31, 300), (30, 300)]])
# two add_terms calls on one field: each upload group has its own budget
one("two_groups", "bits", 130, False, 65_536, [[(40, 3000)], [(41, 300)]])
one("one_group", "bits", 130, False, 65_536, [[(40, 3000), (41, 300)]])
# 64 postings in 2^27 docs, norms omitted: cells of 2^21 docs would hold a posting each -- a packed context stops at 2^20
one("huge_plain", lc.DEFAULT_POLICY, 0, False, 1 << 27, [[(50, 64)]], norms=False)
one("huge_packed", lc.DEFAULT_POLICY, 0, True, 1 << 27, [[(50, 64)]], norms=False)
one("huge_packed_100000", lc.DEFAULT_POLICY, 100000, True, 1 << 27, [[(50, 64)]], norms=False)
print("done", flush=True)
