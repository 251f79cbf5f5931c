"""tests/_column64_cases.py checked without a device: (1) floors on what the sweep's layouts and the default fuzz rounds contain,
computed from the references alone, so that tests/test_column64_edges_gpu.py and tests/test_fuzz_columns64_gpu.py cannot go hollow --
they are conditions on the INPUTS, not on the library; (2) the 64-bit references against plain per-doc Python loops over one tiny
corpus (leaves of 1, 64 and 65 docs): ordering and paging under Long.compare / Double.compare written out on Python ints and floats,
negative doubles, signed zeros, NaN payloads, mask words, range counts -- an error in a reference cannot hide the same error in a
kernel."""
import collections
import dataclasses
import struct

import numpy as np
import pytest

from nrtsearch_amd import synth

from tests import _column64_cases as c64
from tests import _column_cases as cc
from tests import _field_sort64_ref as f64
from tests import _field_sort_ref as fs
from tests.test_column_cases_host import loop_hits, loop_values, text_items_at_most   # the hit sets one doc at a time (32-bit range clauses included)
from tests.test_fuzz_columns64_gpu import BASE

DEFAULT_ROUNDS = 8


def where(m: c64.Model, key, bits: int) -> str:
    """"inside" the column's window, "outside" it, or "none" (no leaf holds a value), by the kind's order"""
    w = m.window(key)
    if w is None:
        return "none"
    return "inside" if w[0] <= f64.order_int(key[1], bits) <= w[1] else "outside"


def same_value(kind: str, a: int, b: int) -> bool:
    return f64.order_int(kind, a) == f64.order_int(kind, b)


# ---- the sweep ---------------------------------------------------------------------------------------------------------------------------
NANINF = ("s", "double", "naninf")
# the layouts of at most 4096 docs, written out: 12 docid bits leave 52 for a span of 2^51 + 1
NANINF_FITS = [(1,), (63,), (64,), (65,), (1023,), (1024,), (1025,), (1024, 1, 1023), (64, 65, 63, 1), (1025, 1024, 1023, 40)]


def test_the_sweep_layouts():
    assert cc.SINGLE_LEAF == (1, 63, 64, 65, 1023, 1024, 1025, 12287, 12288, 12289) and len(cc.LAYOUTS) == 15
    assert [l for l in cc.LAYOUTS if c64.sweep_case(l, False)[0].fits(NANINF)] == NANINF_FITS
    for layout, deletes in [(l, False) for l in cc.LAYOUTS] + [(cc.HOLES, True)]:
        m, reqs = c64.sweep_case(layout, deletes)
        edges = {seg.doc_base + d for seg in m.corpus.segments for d in cc.edge_docs(seg.max_doc)}
        live = {seg.doc_base + d for seg in m.corpus.segments for d in range(seg.max_doc) if seg.live_bits is None or fs._bits(seg.live_bits, seg.max_doc)[d]}
        assert all(m.fits(key) for key in c64.SORT_COLUMNS if key != NANINF) and m.fits(NANINF) == (m.n_docs <= 4096), layout
        if m.n_docs > 4096:   # ... because the column does hold both ends of its pool
            assert m.window(NANINF) == (f64.order_int("double", c64.DBL_MAX), f64.order_int("double", c64.NAN))
        seen = collections.Counter()
        for entry in c64.ENTRIES:
            for r in reqs[entry]:
                seen[entry] += 1
                if entry == "mask64":
                    continue
                exp = m.expected(r)
                seen["multi_clause"] += int(r.docset and any(key[0] == "m" for key, _, _ in r.ranges))
                seen["multi_clause_beside_single"] += int(r.docset and {key[0] for key, _, _ in r.ranges} == {"s", "m"})
                if r.counts:
                    seen["sixty_four"] += int(len(r.count_ranges) == 64)
                    seen["counted"] += int(sum(exp[0]) > 0)
                    continue
                seen["cursors"] += int(r.after is not None)
                if r.after is not None and where(m, r.column, r.after[1]) != "inside" and not same_value(r.column[1], r.after[1], r.missing):
                    seen["cursors_outside"] += 1
                seen["cursor_is_missing"] += int(r.after is not None and same_value(r.column[1], r.after[1], r.missing))
                seen["missing_" + where(m, r.column, r.missing)] += 1
                seen["nan_payload_missing"] += int(r.missing == c64.NAN_PAYLOAD)
                if r.column[2] == "best" and r.after is None and not r.filters and not r.must_nots and not r.ranges and r.clauses in ((), (cc.ALL,)) and layout != cc.HOLES:
                    # an edge doc heads the page in both directions (they hold, in turn, the lowest and the highest values)
                    assert len(edges & live) < 2 or int(exp[0][0]) in edges, (layout, c64.describe(r), exp[0][:4])
                    seen["edge_heads_descending"] += int(r.reverse)
                    seen["edge_heads"] += 1
        assert all(seen[e] >= 8 for e in c64.ENTRIES), (layout, dict(seen))
        assert seen["multi_clause"] >= 4 and seen["multi_clause_beside_single"] >= 2 and seen["sixty_four"] >= 8 and seen["counted"] >= 8, (layout, dict(seen))
        assert seen["cursors"] >= 8 and seen["cursors_outside"] >= 2 and seen["cursor_is_missing"] >= 2, (layout, dict(seen))
        assert seen["missing_outside"] >= 8 and seen["nan_payload_missing"] >= 8 and (seen["missing_inside"] >= 8 or m.n_docs == 1), (layout, dict(seen))
        assert (seen["edge_heads"] >= 4 and seen["edge_heads_descending"] >= 2) or layout == cc.HOLES, (layout, dict(seen))
        for key in c64.SORT_COLUMNS:
            gap = c64.GAP[key[1:]]
            if gap is not None and m.window(key) is not None and m.window(key)[0] < m.window(key)[1]:   # inside the window, and no doc holds it
                assert where(m, key, gap) == "inside" or key[2] != "best", (layout, key)
                assert all(col is None or gap not in col[1].tolist() for col in m.columns[key]), (layout, key)
            assert where(m, key, c64.TRAP[key[1]]) != "inside"
            for n, col in zip(layout, m.columns[key]):
                if col is None or not len(col[1]):
                    continue
                if key[2] == "best":       # no value near the kind's minimum: a padded slot would show
                    assert int(f64.order_key("long", col[1]).min()) > -2**62
                if key[2] == "sparse_last":    # the sparse columns do end, or do not end, on the last doc, as their names say
                    assert int(col[0][-1]) == n - 1 and len(col[0]) < n or n == 1
                if key[2] == "sparse_nolast":
                    assert int(col[0][-1]) < n - 1
            if key[2] == "empty":
                assert all(col is None or (col[0] is not None and len(col[0]) == 0) for col in m.columns[key])
        if layout == cc.HOLES:
            assert all(cols[1] is None and len(cols[2][1]) == 0 for cols in m.columns.values())


# ---- the fuzz ----------------------------------------------------------------------------------------------------------------------------
def take_census(base: int, rounds: int = DEFAULT_ROUNDS) -> collections.Counter:
    c = collections.Counter()
    for round_ in range(rounds):
        m, batches = c64.fuzz_round(base, round_)
        assert (m.flags != 0) == (round_ % 4 == 3) and sum(n == cc.FUZZ_LARGE for n in m.sizes) <= 1
        assert all(m.fits(key) for key in c64.FUZZ_COLUMNS) and NANINF not in m.columns
        cut = False
        for entry, reqs in batches:
            assert 1 <= len(reqs) <= 16 and not (m.flags and not entry.startswith("docset"))
            c["mixed_kinds"] += int(entry.endswith("sorted64") and {r.column[1] for r in reqs} == {"long", "double"})
            for r in reqs:
                c["requests"] += 1
                if entry == "mask64":
                    c["masks_several_clauses"] += int(len(r.value_clauses) >= 2)
                    continue
                exp = m.expected(r)
                c["empty_hit_set"] += int(exp[1 if r.counts else 2] == 0)
                multi = r.docset and any(key[0] == "m" for key, _, _ in r.ranges)
                items = m.docset_items(len(reqs)) if r.docset else text_items_at_most(m, r)
                cut = cut or (r.docset and items >= 2)
                if r.counts:
                    c["multi_clause_counted"] += int(multi)
                    c["sixty_four_ranges"] += int(len(r.count_ranges) == 64)
                    continue
                c["multi_clause_sorted"] += int(multi)
                kind = r.column[1]
                if r.after is not None:
                    c["cursor_in_a_run"] += int(len(exp[0]) > 0 and same_value(kind, int(exp[1][0]), r.after[1]))
                    c["cursor_outside"] += int(where(m, r.column, r.after[1]) == "outside" and not same_value(kind, r.after[1], r.missing))
                c["missing_sentinel"] += int(where(m, r.column, r.missing) != "inside")
                c["missing_inside"] += int(where(m, r.column, r.missing) == "inside")
                # more hits than the candidate buffer holds inside ONE item (by the pigeonhole, whatever the cut), every one a candidate
                if r.after is None and r.k >= 1000 and exp[2] > cc.CAND_CAP * items:
                    c["buffer_overflows_" + entry] += 1
        c["rounds_cut_into_items"] += int(cut)
    return c


@pytest.fixture(scope="module")
def census():
    return take_census(BASE)


@pytest.mark.parametrize("what", ["buffer_overflows_sorted64", "buffer_overflows_docset_sorted64", "cursor_in_a_run", "cursor_outside", "missing_sentinel",
                                  "missing_inside", "empty_hit_set", "multi_clause_sorted", "multi_clause_counted", "mixed_kinds"])
def test_the_default_rounds_hold_at_least_three_of(census, what):
    assert census[what] >= 3, dict(census)


def test_the_default_rounds_cut_queries_into_items(census):
    assert census["rounds_cut_into_items"] >= 2 and census["requests"] >= 400, dict(census)


# ---- the references against plain loops ---------------------------------------------------------------------------------------------------
def loop_key(kind: str, bits: int):
    """Long.compare / Double.compare as a Python sort key, from the value itself"""
    if kind == "long":
        return (0, struct.unpack("<q", struct.pack("<Q", bits))[0], 0)
    f = struct.unpack("<d", struct.pack("<Q", bits))[0]
    if f != f:
        return (1, 0.0, 0)                                   # every NaN equal, above +inf
    return (0, f, 0 if f != 0.0 or bits >> 63 else 1)        # -0.0 below +0.0


def loop_bits(kind: str, bits: int) -> int:
    return 0x7FF8000000000000 if kind == "double" and loop_key(kind, bits)[0] == 1 else bits


def loop_expected(m: c64.Model, r: c64.Req):
    if r.entry == "mask64":
        n = m.sizes[r.leaf]
        words = [0] * ((n + 63) // 64)
        for d in range(n):
            ok = True
            for c in r.value_clauses:
                v = loop_values(m.columns[c[0]][r.leaf], d)
                ok = ok and len(v) == 1 and (c[1] == "exists" or loop_key(c[0][1], c[2]) <= loop_key(c[0][1], v[0]) <= loop_key(c[0][1], c[3]))
            words[d // 64] |= int(ok) << (d % 64)
        return words, sum(bin(w).count("1") for w in words)
    kind = r.column[1]
    hits = loop_hits(m, r)
    if r.counts:
        counts, valued = [0] * len(r.count_ranges), 0
        for si, d in hits:
            for v in loop_values(m.columns[r.column][si], d):
                valued += 1
                for i, (lo, hi) in enumerate(r.count_ranges):
                    counts[i] += int(loop_key(kind, lo) <= loop_key(kind, v) <= loop_key(kind, hi))
        return counts, len(hits), valued
    rows = []
    for si, d in hits:   # (in docid order)
        v = loop_values(m.columns[r.column][si], d)
        bits = loop_bits(kind, v[0] if v else r.missing)
        rows.append((loop_key(kind, bits), m.corpus.segments[si].doc_base + d, bits))
    rows = sorted(rows, key=lambda row: row[0], reverse=r.reverse)   # stable: equal values stay in docid order, in both directions
    if r.after is not None:
        ak = loop_key(kind, r.after[1])
        rows = [row for row in rows if (row[0] < ak if r.reverse else row[0] > ak) or (row[0] == ak and row[1] > r.after[0])]
    page = rows[: r.k]
    gte = len(hits) > max(r.threshold, r.k) and len(page) == r.k   # (one slice: m.slicing[0] == 0)
    return [row[1] for row in page], [row[2] for row in page], len(hits), gte


def test_the_references_equal_plain_loops():
    sizes = (1, 64, 65)
    corpus = fs.make_corpus(sizes, {cc.ALL: 1.0, 2: 0.5, 3: 0.3}, seed=27, delete_fraction=0.1)
    rng = np.random.default_rng(28)
    masks = {mid: [synth.random_mask(n, dens, 9 * mid + si) for si, n in enumerate(sizes)] for mid, dens in ((5, 0.6), (6, 0.2))}
    columns = {}
    for si, n in enumerate(sizes):
        for key, col in c64._range32_columns(rng, n).items():
            columns.setdefault(key, []).append(col)
    for kind in c64.KINDS:   # the bounds hold negative doubles, both zeros, the infinities and NaNs under four payloads
        columns[("s", kind, "dense")] = [(None, rng.choice(c64.BOUNDS[kind], size=n)) for n in sizes]
        sparse = []
        for n in (1, None, 65):
            d = None if n is None else np.nonzero(rng.random(n) < 0.5)[0].astype(np.int32)
            sparse.append(None if n is None else (d, rng.choice(c64.BOUNDS[kind], size=len(d))))
        columns[("s", kind, "sparse")] = sparse
    m = c64.Model(corpus, masks, columns, slicing=(0, 5, 1))
    text_sets = [dict(clauses=(cc.ALL,)), dict(clauses=(2, 3, 3), need=2), dict(clauses=(2, 3), need=2, must=True), dict(clauses=(2, 3), filters=(5,), must_nots=(6,)),
                 dict(clauses=(cc.NOWHERE,))]
    doc_sets = c64.doc_set_shapes()
    reqs = []
    for kind in c64.KINDS:
        bounds = [int(b) for b in c64.BOUNDS[kind]]
        for entry, sets in (("sorted64", text_sets), ("docset_sorted64", doc_sets)):
            for hi, hs in enumerate(sets):
                for name in ("dense", "sparse"):
                    for rev in (False, True):
                        for ki, (k, thr) in enumerate(((1, 1000), (7, 0), (130, 10))):
                            missing = (c64.KIND_MIN[kind], c64.KIND_MAX[kind], bounds[(hi + ki) % len(bounds)], c64.NAN_PAYLOAD if kind == "double" else bounds[3])[(hi + ki + rev) % 4]
                            base = c64.Req(entry, column=("s", kind, name), k=k, reverse=rev, missing=missing, threshold=thr, **hs)
                            reqs.append(base)
                            page = m.expected(base)
                            if len(page[0]):   # the next page, and a cursor that is no hit
                                reqs.append(dataclasses.replace(base, after=(int(page[0][-1]), int(page[1][-1]))))
                                reqs.append(dataclasses.replace(base, after=(64, bounds[(3 * hi + ki) % len(bounds)])))
        for entry, sets in (("ranges64", text_sets), ("docset_ranges64", doc_sets)):
            for hs in sets:
                for name in ("dense", "sparse"):
                    pairs = [(bounds[i % len(bounds)], bounds[(5 * i + 2) % len(bounds)]) for i in range(len(bounds))]
                    reqs.append(c64.Req(entry, column=("s", kind, name), count_ranges=tuple(pairs + [(c64.KIND_MIN[kind], c64.KIND_MAX[kind])]), **hs))
        for leaf in (0, 2, 1):
            for name in ("dense", "sparse"):
                if columns[("s", kind, name)][leaf] is None:
                    continue
                key = ("s", kind, name)
                reqs.append(c64.Req("mask64", leaf=leaf, value_clauses=((key, "exists"),)))
                reqs += [c64.Req("mask64", leaf=leaf, value_clauses=((key, "range", a, b),)) for a in bounds[::3] for b in bounds[1::4]]
                reqs.append(c64.Req("mask64", leaf=leaf, value_clauses=((key, "range", c64.KIND_MIN[kind], c64.KIND_MAX[kind]), (("s", kind, "dense"), "range", bounds[0], bounds[-1]))))
    seen = collections.Counter()
    for r in reqs:
        got, exp = m.expected(r), loop_expected(m, r)
        got = tuple(x.tolist() if isinstance(x, np.ndarray) else x for x in got)
        assert got == tuple(exp), f"{c64.describe(r)}: the reference {got}, the loop {exp}"
        seen[r.entry] += 1
        if r.sorts:
            seen["paged"] += int(r.after is not None and len(got[0]) > 0)
            seen["in_a_run"] += int(r.after is not None and len(got[0]) > 0 and got[1][0] == loop_bits(r.column[1], r.after[1]))
            seen["nan_reported"] += int(0x7FF8000000000000 in got[1])
            seen["negative_double"] += int(r.column[1] == "double" and any(b >> 63 and b != c64.NZERO for b in got[1]))
            seen["signed_zeros_adjacent"] += int(any({a, b} == {c64.NZERO, c64.PZERO} for a, b in zip(got[1], got[1][1:])))
            assert all(b == 0x7FF8000000000000 or loop_key(r.column[1], b)[0] == 0 for b in got[1])   # no NaN payload is ever reported
        elif r.entry == "mask64":
            seen["mask_docs"] += got[1]
        else:
            seen["counted"] += sum(got[0])
    assert len(reqs) > 700 and seen["paged"] > 50 and seen["in_a_run"] > 10 and seen["nan_reported"] > 10 and seen["negative_double"] > 10, dict(seen)
    assert seen["signed_zeros_adjacent"] > 3 and seen["mask_docs"] > 500 and seen["counted"] > 500 and all(seen[e] >= 20 for e in c64.ENTRIES), dict(seen)
