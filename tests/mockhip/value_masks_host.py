"""Run by tests/test_value_masks_host.py in a subprocess with tests/mockhip preloaded (kernels do nothing: a built mask holds no
doc): the HOST side of nrtgpu_segment_set_mask_from_values / nrtgpu_segment_get_mask -- every refusal with its status and the
precedence of the statuses, and the bookkeeping: a failed call keeps the old mask, get_mask round-trips what set_mask registered,
a rebuild drops the combined accept sets, device_bytes is unchanged by the call, a fork's masks are its own.  One line
`name value` per case on stdout."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from nrtsearch_amd import _lib, api   # noqa: E402
from tests import _field_sort_ref as fs   # noqa: E402

L = _lib.load()
COL, MCOL, FCOL, EMPTY = 7, 8, 9, 10
VC = api.ValueClause


def say(name, text):
    print(name, text, flush=True)


corpus = fs.make_corpus([130], {1: 1.0}, seed=11)
seg = corpus.segments[0]
N, WORDS = seg.max_doc, (seg.max_doc + 63) // 64
ctx = api.GpuContext(device_id=0, max_batch=16)


def upload(seal=True):
    g = api.GpuSegment(ctx, N, 0)
    g.add_field_norms(0, seg.norms)
    g.add_terms(0, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
    g.add_doc_values(COL, "int", np.arange(N, dtype=np.int32))
    g.add_doc_values_multi(MCOL, "int", np.arange(2 * N, dtype=np.int32), np.repeat(np.arange(N, dtype=np.int32), 2))
    g.add_doc_values(FCOL, "float", np.zeros(5, dtype=np.float32), np.arange(5, dtype=np.int32))
    g.add_doc_values_multi(EMPTY, "float", np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.int32))
    if seal:
        g.seal()
    return g


g = upload()
count = C.c_int64(-1)


def raw(h, mask_id, clauses, n=None, out=True):
    """the status of the C call over hand-made records ([(kind, field, lower, upper, n_values, reserved, values or None)])"""
    vc, keep = None, []
    if clauses is not None:
        vc = (_lib.ValueClause * max(len(clauses), 1))()
        for i, (kind, field, lo, hi, n_values, reserved, values) in enumerate(clauses):
            r = vc[i]
            r.kind, r.field_id, r.lower_bits, r.upper_bits, r.n_values, r.reserved = kind, field, lo, hi, n_values, reserved
            if values is not None:
                arr = (C.c_uint32 * max(len(values), 1))(*values)
                keep.append(arr)
                r.value_bits = arr
    return L.nrtgpu_segment_set_mask_from_values(h, mask_id, vc, len(clauses) if n is None else n, C.byref(count) if out else None)


RANGE, EXISTS, IN_SET = _lib.NRTGPU_CLAUSE_RANGE, _lib.NRTGPU_CLAUSE_EXISTS, _lib.NRTGPU_CLAUSE_IN_SET
ok_range = (RANGE, COL, 3, 9, 0, 0, None)

# ---- what runs (the stand-in's kernel writes nothing: no doc)
say("range", f"{g.set_mask_from_values(20, [VC.range_(COL, 'int', 3, 9)])} {int(g.get_mask(20).any())}")
say("exists", g.set_mask_from_values(21, [VC.exists(FCOL)]))
say("in_set", g.set_mask_from_values(22, [VC.in_set(MCOL, 'int', [5, 5, 1])]))
say("in_set_4096", g.set_mask_from_values(23, [VC.in_set(COL, 'int', np.arange(4096, dtype=np.int32))]))
say("four_mixed", g.set_mask_from_values(24, [VC.range_(COL, 'int', 9, 3), VC.exists(MCOL), VC.in_set(FCOL, 'float', [-0.0, 0.0, float('nan')]),
                                              VC.in_set(MCOL, 'int', np.arange(4096, dtype=np.int32))]))
say("column_without_values", g.set_mask_from_values(25, [VC.exists(EMPTY)]))
say("null_out_count", raw(g._h, 26, [ok_range], out=False))

# ---- invalid arguments
say("seg_null", raw(None, 5, [ok_range]))
say("clauses_null", raw(g._h, 5, None, n=1))
say("mask_id_zero", raw(g._h, 0, [ok_range]))
say("mask_id_negative", raw(g._h, -3, [ok_range]))
say("n_clauses_zero", raw(g._h, 5, [ok_range], n=0))
say("n_clauses_five", raw(g._h, 5, [ok_range] * 5))
say("kind_three", raw(g._h, 5, [(3, COL, 0, 0, 0, 0, None)]))
say("kind_negative", raw(g._h, 5, [(-1, COL, 0, 0, 0, 0, None)]))
say("reserved", raw(g._h, 5, [(RANGE, COL, 3, 9, 0, 1, None)]))
say("in_set_no_values", raw(g._h, 5, [(IN_SET, COL, 0, 0, 0, 0, [1])]))
say("in_set_4097", raw(g._h, 5, [(IN_SET, COL, 0, 0, 4097, 0, list(range(4097)))]))
say("in_set_null_values", raw(g._h, 5, [(IN_SET, COL, 0, 0, 2, 0, None)]))
say("range_with_n_values", raw(g._h, 5, [(RANGE, COL, 3, 9, 1, 0, None)]))
say("exists_with_values", raw(g._h, 5, [(EXISTS, COL, 0, 0, 0, 0, [1])]))
say("names_the_clause", int("clause 1" in L.nrtgpu_last_error().decode()) if raw(g._h, 5, [ok_range, (EXISTS, COL, 0, 0, 0, 0, [1])]) else -1)

# ---- state, unsupported, and the precedence
u = upload(seal=False)
say("unsealed", raw(u._h, 5, [ok_range]))
say("invalid_before_unsealed", raw(u._h, 5, [(3, COL, 0, 0, 0, 0, None)]))
say("unsealed_before_unsupported", raw(u._h, 5, [(RANGE, 55, 0, 0, 0, 0, None)]))
u.release()
say("column_not_resident", raw(g._h, 5, [(RANGE, 55, 0, 0, 0, 0, None)]))
say("names_the_field", int("55" in L.nrtgpu_last_error().decode()))
say("postings_field_is_no_column", raw(g._h, 5, [(EXISTS, 0, 0, 0, 0, 0, None)]))
say("invalid_in_clause_1_before_unsupported_in_clause_0", raw(g._h, 5, [(RANGE, 55, 0, 0, 0, 0, None), (RANGE, COL, 0, 0, 0, 1, None)]))

buf = np.zeros(WORDS, dtype=np.uint64)
say("get_null_seg", L.nrtgpu_segment_get_mask(None, 20, buf.ctypes.data, WORDS))
say("get_null_bits", L.nrtgpu_segment_get_mask(g._h, 20, None, WORDS))
say("get_short", L.nrtgpu_segment_get_mask(g._h, 20, buf.ctypes.data, WORDS - 1))
say("get_not_registered", L.nrtgpu_segment_get_mask(g._h, 77, buf.ctypes.data, WORDS))
say("get_short_before_not_registered", L.nrtgpu_segment_get_mask(g._h, 77, buf.ctypes.data, WORDS - 1))
say("get_more_room", L.nrtgpu_segment_get_mask(g._h, 20, np.zeros(WORDS + 3, dtype=np.uint64).ctypes.data, WORDS + 3))

# ---- bookkeeping
pattern = np.arange(1, WORDS + 1, dtype=np.uint64) * np.uint64(0x0101010101010101)
g.set_mask(5, pattern)
say("get_round_trips_set_mask", int(np.array_equal(g.get_mask(5), pattern)))
for name, bad in (("unsupported", [(RANGE, 55, 0, 0, 0, 0, None)]), ("invalid", [(3, COL, 0, 0, 0, 0, None)])):
    rc = raw(g._h, 5, bad)
    say(f"a_failed_call_keeps_the_old_mask_{name}", f"{int(rc != 0)} {int(np.array_equal(g.get_mask(5), pattern))}")

sr = api.GpuIndexSearcher(ctx, [g], api.IndexStatistics.from_corpus(corpus))
top, sort = api.TopScoreDocCollectorManager(10), api.SortField(COL, "int")
before = g.device_bytes
api.search_docset_sorted_batch(sr, [api.DocSetQuery((api.MaskFilter(5),))], [top], [sort])
with_set = g.device_bytes
g.set_mask_from_values(5, [VC.range_(COL, "int", 0, 50)])
say("a_rebuild_drops_the_accept_sets", f"{int(with_set > before)} {int(g.device_bytes == before)}")
say("the_rebuilt_mask_replaced_the_old", int(not g.get_mask(5).any()))
api.search_docset_sorted_batch(sr, [api.DocSetQuery((api.MaskFilter(5),))], [top], [sort])
say("a_built_mask_is_resident_for_a_query", int(g.device_bytes == with_set))
g.set_mask(5, None)
say("dropped_like_any_mask", L.nrtgpu_segment_get_mask(g._h, 5, buf.ctypes.data, WORDS))
say("device_bytes_unchanged", int(g.device_bytes == before))

g.set_mask(6, pattern)
f = g.fork(None)
say("a_fork_starts_without_masks", L.nrtgpu_segment_get_mask(f._h, 6, buf.ctypes.data, WORDS))
f.set_mask_from_values(6, [VC.exists(COL)])
say("a_forks_masks_are_its_own", f"{int(np.array_equal(g.get_mask(6), pattern))} {int(not f.get_mask(6).any())}")
f.release()
say("the_parent_keeps_its_mask", int(np.array_equal(g.get_mask(6), pattern)))

g.release()
ctx.close()
print("done", flush=True)
