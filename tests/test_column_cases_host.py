"""tests/_column_cases.py checked without a device: (1) floors on what the default fuzz rounds and the sweep's layouts contain,
computed from the references alone, so that tests/test_fuzz_columns_gpu.py and tests/test_column_edges_gpu.py cannot go hollow --
they are conditions on the INPUTS, not on the library; (2) the four references against plain per-doc Python loops over one tiny
corpus (leaves of 1, 64 and 65 docs): ordering, paging, ranges, counting -- an error in a reference cannot hide the same error in a
kernel."""
import collections
import dataclasses
import struct

import numpy as np
import pytest

from nrtsearch_amd import synth

from tests import _column_cases as cc
from tests import _field_sort_ref as fs
from tests import test_docset_gpu as dg
from tests.test_fuzz_columns_gpu import BASE

DEFAULT_ROUNDS = 8
TEXT_MIN_ITEM_COST, TILE_COST = 1 << 17, 48   # planner.cpp: build_plan's min_item_cost, kTileCostPostings


def text_items_at_most(m: cc.Model, r: cc.Req) -> int:
    """an upper bound of the items a text query is cut into: its cost over the least cost of an item, rounded (host_math.h)"""
    cost = sum(m.corpus.doc_freq.get(t, 0) for t in r.clauses) + TILE_COST * sum((n + cc.TILE_DOCS - 1) // cc.TILE_DOCS for n in m.sizes)
    return max(1, (cost + TEXT_MIN_ITEM_COST // 2) // TEXT_MIN_ITEM_COST)


def take_census(base: int) -> collections.Counter:
    c = collections.Counter()
    for round_ in range(DEFAULT_ROUNDS):
        m, batches = cc.fuzz_round(base, round_)
        assert (m.flags != 0) == (round_ % 4 == 3)
        for entry, reqs in batches:
            assert 1 <= len(reqs) <= 16 and not (m.flags and not entry.startswith("docset"))
            arities = set()
            for r in reqs:
                exp = m.expected(r)
                arities |= {r.column[0]} | {key[0] for key, _, _ in r.ranges}
                c["requests"] += 1
                c["empty_hit_set"] += int(exp[3 if not r.sorts else 2] == 0)
                c["four_ranges"] += int(len(r.ranges) == 4)
                items = m.docset_items(len(reqs)) if r.docset else text_items_at_most(m, r)
                c["cut_into_items"] += int(r.docset and items >= 2)
                if not r.sorts:
                    c["overflowed"] += exp[5]
                    continue
                if r.after is not None and len(exp[0]) and int(exp[1][0]) == int(fs.canonical_bits(r.column[1], [r.after[1]])[0]):
                    c["cursor_in_a_run"] += 1
                # more hits than the candidate buffer holds inside ONE item (by the pigeonhole, whatever the cut), every one a candidate
                if r.after is None and r.k >= 1000 and exp[2] > cc.CAND_CAP * items:
                    c["buffer_overflows"] += 1
                    every = m.expected(dataclasses.replace(r, k=exp[2]))[1]
                    keys = fs.order_key(r.column[1], every)   # (the high word of a key is this + 2^31, complemented when ascending)
                    c["buffer_overflows_full_range"] += int(abs(int(keys[-1]) - int(keys[0])) >= 2**31)
            c["mixed_arities"] += int(arities == {"s", "m"})
    return c


@pytest.fixture(scope="module")
def census():
    return take_census(BASE)


@pytest.mark.parametrize("what", ["buffer_overflows", "buffer_overflows_full_range", "cursor_in_a_run", "overflowed", "empty_hit_set", "four_ranges",
                                  "mixed_arities"])
def test_the_default_rounds_hold_at_least_three_of(census, what):
    assert census[what] >= 3, dict(census)


def test_the_default_rounds_cut_queries_into_items(census):
    assert census["cut_into_items"] >= 2 and census["requests"] >= 400, dict(census)


def test_the_sweep_layouts():
    assert cc.SINGLE_LEAF == (1, 63, 64, 65, 1023, 1024, 1025, 12287, 12288, 12289) and len(cc.LAYOUTS) == 15
    whole_tiles = 0
    for layout, deletes in [(l, False) for l in cc.LAYOUTS] + [(cc.HOLES, True)]:
        m, reqs = cc.sweep_case(layout, deletes)
        edges = {seg.doc_base + d for seg in m.corpus.segments for d in cc.edge_docs(seg.max_doc)}
        live = {seg.doc_base + d for seg in m.corpus.segments for d in range(seg.max_doc) if seg.live_bits is None or fs._bits(seg.live_bits, seg.max_doc)[d]}
        seen = collections.Counter()
        for entry in cc.ENTRIES:
            for r in reqs[entry]:
                exp = m.expected(r)
                seen[entry] += 1
                seen["cursors"] += int(r.after is not None)
                seen["multi"] += int(r.column[0] == "m")
                seen["four_ranges"] += int(len(r.ranges) == 4)
                if not r.sorts:
                    seen["overflowed"] += exp[5]
                elif r.column[2] == "best" and r.after is None and not r.filters and not r.must_nots and not r.ranges and r.clauses in ((), (cc.ALL,)) and layout != cc.HOLES:
                    # an edge doc heads the page in both directions (they hold, in turn, the lowest and the highest values)
                    assert len(edges & live) < 2 or int(exp[0][0]) in edges, (layout, cc.describe(r), exp[0][:4])
                    seen["descending_heads"] += int(r.reverse)
                    seen["edge_heads"] += 1
        assert all(seen[e] >= 8 for e in cc.ENTRIES) and seen["multi"] >= 8 and seen["overflowed"] >= 4 and seen["four_ranges"] >= 4, (layout, dict(seen))
        assert seen["cursors"] >= 16 and (seen["edge_heads"] >= 8 or layout == cc.HOLES), (layout, dict(seen))
        for key, cols in m.columns.items():
            if key[2] == "best":   # no column holds the kind's minimum where the sweep says so
                assert all(col is None or fs.KIND_MIN[key[1]] not in col[1].tolist() for col in cols)
            if key[:1] == ("m",) and key[2] in ("last2", "only_last", "last65"):   # the last doc holds values: on a leaf of 1024 n docs start[d + 1] is the "+ 1" entry
                assert all(col is None or len(col[0]) == 0 or int(col[0][-1]) == n - 1 for n, col in zip(layout, cols))
        whole_tiles += sum(int(n % cc.TILE_DOCS == 0) for n in layout) if layout != cc.HOLES else 0
    assert whole_tiles >= 5


# ---- the references against plain loops ---------------------------------------------------------------------------------------------------
def loop_key(kind: str, bits: int):
    """Integer.compare / Float.compare as a Python sort key, from the value itself"""
    if kind == "int":
        return (0, struct.unpack("<i", struct.pack("<I", bits))[0], 0)
    f = struct.unpack("<f", struct.pack("<I", bits))[0]
    if f != f:
        return (1, 0.0, 0)                                   # every NaN equal, above +inf
    return (0, f, 0 if f != 0.0 or bits >> 31 else 1)        # -0.0 below +0.0


def loop_bits(kind: str, bits: int) -> int:
    return 0x7FC00000 if kind == "float" and loop_key(kind, bits)[0] == 1 else bits


def loop_values(col, d: int):
    """the values of leaf doc d: a list (single-valued: at most one)"""
    if col is None:
        return []
    docs, bits = col
    if docs is None:
        return [int(bits[d])]
    return [int(b) for dd, b in zip(docs.tolist(), bits.tolist()) if dd == d]


def loop_hits(m: cc.Model, r: cc.Req):
    """[(leaf, leaf doc)] of the request's hits, one doc at a time"""
    out = []
    for si, seg in enumerate(m.corpus.segments):
        postings = {t: set(seg.postings(t)[0].tolist()) if t in seg.term_ids.tolist() else set() for t in set(r.clauses)}
        for d in range(seg.max_doc):
            bit = lambda words: bool((int(words[d // 64]) >> (d % 64)) & 1)
            ok = seg.live_bits is None or bit(seg.live_bits)
            ok = ok and all(bit(m.masks[i][si]) for i in r.filters) and not any(bit(m.masks[i][si]) for i in r.must_nots)
            if not r.docset:
                ok = ok and sum(1 for t in r.clauses if d in postings[t]) >= max(r.need, 1)
            for key, lo, hi in r.ranges:
                ok = ok and any(loop_key(key[1], lo) <= loop_key(key[1], v) <= loop_key(key[1], hi) for v in loop_values(m.columns[key][si], d))
            if ok:
                out.append((si, d))
    return out


def loop_expected(m: cc.Model, r: cc.Req):
    kind = r.column[1]
    hits = loop_hits(m, r)
    if r.sorts:
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
    counts = collections.Counter()
    for si, d in hits:
        for v in loop_values(m.columns[r.column][si], d):
            counts[loop_bits(kind, v)] += 1
    if len(counts) > r.max_buckets:
        return [], [], 0, len(hits), -1, 1
    order = sorted(counts, key=lambda b: loop_key(kind, b))
    return order, [counts[b] for b in order], len(order), len(hits), sum(counts.values()), 0


def test_the_references_equal_plain_loops():
    sizes = (1, 64, 65)
    corpus = fs.make_corpus(sizes, {cc.ALL: 1.0, 2: 0.5, 3: 0.3}, seed=17, delete_fraction=0.1)
    rng = np.random.default_rng(18)
    masks = {mid: [synth.random_mask(n, dens, 7 * mid + si) for si, n in enumerate(sizes)] for mid, dens in ((5, 0.6), (6, 0.2))}
    columns = {}
    for kind in cc.KINDS:
        edge = dg.POOLS[(kind, "edge")]
        columns[("s", kind, "dense")] = [cc._single(rng, n, edge) for n in sizes]
        columns[("s", kind, "sparse")] = [cc._single(rng, 1, edge, 0.5), None, cc._single(rng, 65, edge, 0.5)]
        columns[("m", kind, "some")] = [cc._multi(rng, rng.integers(0, 4, size=n), edge) for n in sizes]
    m = cc.Model(corpus, masks, columns, slicing=(0, 5, 1))
    reqs = []
    for kind in cc.KINDS:
        edge = [int(b) for b in dg.POOLS[(kind, "edge")]]
        text_sets = [dict(clauses=(cc.ALL,)), dict(clauses=(2, 3, 3), need=2), dict(clauses=(2, 3), need=2, must=True), dict(clauses=(2, 3), filters=(5,), must_nots=(6,)),
                     dict(clauses=(cc.NOWHERE,))]
        doc_sets = [dict(), dict(filters=(5,), must_nots=(6,))]
        for a, b in ((0, len(edge) - 1), (1, 3), (3, 1), (2, 2), (len(edge) - 1, len(edge) - 1)):
            doc_sets += [dict(ranges=((("s", kind, "dense"), edge[a], edge[b]),)), dict(ranges=((("m", kind, "some"), edge[a], edge[b]), (("s", kind, "sparse"), edge[0], edge[-1])))]
        for entry, sets in (("sorted", text_sets), ("docset_sorted", doc_sets)):
            for hs in sets:
                for name in ("dense", "sparse"):
                    for rev in (False, True):
                        for k, thr in ((1, 1000), (7, 0), (130, 10)):
                            base = cc.Req(entry, column=("s", kind, name), k=k, reverse=rev, missing=edge[2], threshold=thr, **hs)
                            reqs.append(base)
                            page = m.expected(base)
                            if len(page[0]):   # the next page, and a cursor that is no hit
                                reqs.append(dataclasses.replace(base, after=(int(page[0][-1]), int(page[1][-1]))))
                                reqs.append(dataclasses.replace(base, after=(64, edge[3])))
        for entry, sets in (("count", text_sets), ("docset_count", doc_sets)):
            for hs in sets:
                for key in (("s", kind, "dense"), ("s", kind, "sparse"), ("m", kind, "some")):
                    reqs += [cc.Req(entry, column=key, max_buckets=b, **hs) for b in (1, 3, 64)]
    paged = in_a_run = overflowed = 0
    for r in reqs:
        got, exp = m.expected(r), loop_expected(m, r)
        got = tuple(x.tolist() if isinstance(x, np.ndarray) else x for x in got)
        assert got == tuple(exp), f"{cc.describe(r)}: the reference {got}, the loop {exp}"
        paged += int(r.after is not None and len(got[0]) > 0)
        in_a_run += int(r.after is not None and len(got[0]) > 0 and got[1][0] == loop_bits(r.column[1], r.after[1]))
        overflowed += int(not r.sorts and got[5] == 1)
    assert len(reqs) > 500 and paged > 50 and in_a_run > 10 and overflowed > 10
