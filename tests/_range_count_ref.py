"""A NumPy reference of the numeric range facet (nrtgpu_count_ranges_batch, nrtgpu_count_docset_ranges_batch): a query's hits
counted per requested value range of ONE single-valued doc value column of any of the four kinds, independent of the library's
coding of the values, of its cut points and of its elementary intervals.

  hits      the existing references' matching: a text query's (tests/_field_sort64_ref.py: text_hits -- all clauses SHOULD: at least
            max(1, min_should_match) clauses, duplicates count each; all MUST: all of them; inside the accept set), or a doc set's
            (docset_hits: liveDocs AND every filter AND no must_not AND every 32-bit range clause)
  counted   per range sum(has & key(lo) <= key(v) <= key(hi)) with the order keys WRITTEN OUT on integers: Integer.compare /
            Long.compare for the int kinds; sortable bits for floats and doubles (-0.0 < +0.0, every NaN equal and above +inf).
            Ranges are counted independently; lower above upper counts 0; a hit without a value, or in a leaf without the column,
            adds to no range but counts in total_hits
  totCount  hits_with_value = the hits that have a value

Also what the host and the device tests of the route share: the value pools, the named range lists and the seeded fuzz rounds."""
from __future__ import annotations

import random
from typing import List, Optional, Sequence, Tuple

import numpy as np

from tests import _field_sort64_ref as f64
from tests import _field_sort_ref as fs

KINDS = ("int", "float", "long", "double")
WIDE = ("long", "double")
BITS_DTYPE = {"int": np.uint32, "float": np.uint32, "long": np.uint64, "double": np.uint64}
VALUE_DTYPE = {"int": np.int32, "float": np.float32, "long": np.int64, "double": np.float64}


def bits_of(kind: str, value) -> int:
    return int(np.array([value], dtype=VALUE_DTYPE[kind]).view(BITS_DTYPE[kind])[0])


def order_key(kind: str, bits) -> np.ndarray:
    """int64 keys that order like the kind's compare (written out on integers in the two references this one stands on)."""
    return f64.order_key(kind, bits) if kind in WIDE else fs.order_key(kind, bits)


def order_int(kind: str, bits: int) -> int:
    return int(order_key(kind, np.array([bits], dtype=BITS_DTYPE[kind]))[0])


# the least and the greatest value of each kind in its order: -inf is the least float (every NaN sorts above +inf)
LEAST = {"int": bits_of("int", -2**31), "float": bits_of("float", -np.inf), "long": bits_of("long", -2**63), "double": bits_of("double", -np.inf)}
GREATEST = {"int": bits_of("int", 2**31 - 1), "float": 0x7FC00000, "long": bits_of("long", 2**63 - 1), "double": 0x7FF8000000000000}
NAN_PAYLOADS = {"float": [0x7FC00000, 0x7FC00001, 0xFFC12345], "double": [0x7FF8000000000000, 0x7FF0000000000001, 0xFFF8000000000123]}
# The values the columns draw from.  long: values that straddle 2^32 -- 5 and 2^32 + 5, 2^33 + 5 agree in their low words, so a
# compare of 32 bits cannot tell them apart.  double: 1.5 + j ulp (codes that are consecutive integers), the zeros, three NaNs.
POOL = {
    "int": [bits_of("int", v) for v in (-2**31, -1000, -1, 0, 1, 7, 8, 9, 500, 2**31 - 1)],
    "float": [bits_of("float", v) for v in (-np.inf, -1.5, -0.0, 0.0, 1e-45, 3.25, 7.0, np.inf)] + NAN_PAYLOADS["float"],
    "long": [bits_of("long", v) for v in (-2**63, -2**32 - 5, -1, 0, 5, 2**32 - 1, 2**32, 2**32 + 5, 2**33 + 5, 1_700_000_000_000, 2**63 - 1)],
    "double": [bits_of("double", 1.5) + j for j in range(7)] + [bits_of("double", v) for v in (-np.inf, -0.0, 0.0, np.inf)] + NAN_PAYLOADS["double"],
}
# a range that no pool value lies in
GAP = {"int": (bits_of("int", 2), bits_of("int", 6)), "float": (bits_of("float", 0.5), bits_of("float", 1.0)),
       "long": (bits_of("long", 2**32 + 6), bits_of("long", 2**33)), "double": (bits_of("double", 2.0), bits_of("double", 3.0))}


def sorted_pool(kind: str) -> List[int]:
    """The pool's distinct values (one NaN) ascending in the kind's order."""
    seen = {}
    for b in POOL[kind]:
        seen.setdefault(order_int(kind, b), b)
    return [seen[k] for k in sorted(seen)]


def range_lists(kind: str) -> List[Tuple[str, List[Tuple[int, int]]]]:
    """The named range lists of the device tests: (lower_bits, upper_bits), both inclusive."""
    sp, G, L = sorted_pool(kind), GREATEST[kind], LEAST[kind]
    n = len(sp)
    return [
        ("disjoint", [(sp[0], sp[1]), (sp[3], sp[4]), (sp[6], sp[7])]),
        ("nested", [(sp[1], G), (sp[3], G), (sp[5], G)]),
        ("twice", [(sp[2], sp[5]), (sp[2], sp[5])]),
        ("touching", [(sp[1], sp[4]), (sp[4], sp[6])]),
        ("single", [(sp[3], sp[3])]),
        ("to_greatest", [(sp[4], G)]),
        ("from_least", [(L, sp[4])]),
        ("empty", [(sp[5], sp[2]), (sp[2], sp[5])]),
        ("none_inside", [GAP[kind]]),
        ("sixty_four", [(sp[i % n], sp[(i * 7 + 3) % n]) for i in range(64)]),
    ]


def column_arrays(seg, column, kind: str):
    """(has bool[max_doc], value bits[max_doc]) of one leaf's column: None, or (docs or None = every doc, value bits)."""
    has = np.zeros(seg.max_doc, dtype=bool)
    vals = np.zeros(seg.max_doc, dtype=BITS_DTYPE[kind])
    if column is not None:
        cd, cv = column
        idx = np.arange(seg.max_doc) if cd is None else np.asarray(cd)
        has[idx] = True
        vals[idx] = np.asarray(cv, dtype=BITS_DTYPE[kind])
    return has, vals


def count(corpus, hits: Sequence[np.ndarray], columns, kind: str, ranges: Sequence[Tuple[int, int]]):
    """-> (counts [int] in request order, total_hits, hits_with_value).  hits[leaf]: bool per doc; columns[leaf]: None (the leaf
    lacks the column) or (docs or None = every doc, value bits)."""
    total, keys = 0, []
    for si, seg in enumerate(corpus.segments):
        ok = np.asarray(hits[si], dtype=bool)
        total += int(ok.sum())
        has, vals = column_arrays(seg, columns[si], kind)
        keys.append(order_key(kind, vals[ok & has]))
    k = np.concatenate(keys) if keys else np.zeros(0, np.int64)
    counts = []
    for lo, hi in ranges:
        a, b = order_int(kind, lo), order_int(kind, hi)
        counts.append(int(((k >= a) & (k <= b)).sum()))
    return counts, total, int(len(k))


text_hits = f64.text_hits        # (corpus, term_ids, need, accept=, live=) -> per leaf bool[max_doc]
docset_hits = f64.docset_hits    # (corpus, filters, must_nots, ranges32) -> per leaf bool[max_doc]


# ---- the seeded fuzz rounds the host test judges and the device test runs ------------------------------------------------------
FUZZ_SIZES = [1500, 700, 90]
FUZZ_TERMS = {1: 1.0, 2: 0.5, 3: 0.3, 4: 0.15}
FUZZ_FIELD = {"int": 20, "float": 21, "long": 22, "double": 23}
FUZZ_ROUNDS = 8


def fuzz_corpus():
    return fs.make_corpus(FUZZ_SIZES, FUZZ_TERMS, seed=77, delete_fraction=0.03)


def fuzz_columns(corpus):
    """kind -> per leaf column: 85 % of leaf 0, all of leaf 1, absent from leaf 2."""
    rng = np.random.default_rng(78)
    out = {}
    for kind in KINDS:
        pool = np.array(POOL[kind], dtype=BITS_DTYPE[kind])
        d0 = np.nonzero(rng.random(FUZZ_SIZES[0]) < 0.85)[0].astype(np.int32)
        out[kind] = [(d0, rng.choice(pool, size=len(d0))), (None, rng.choice(pool, size=FUZZ_SIZES[1])), None]
    return out


def fuzz_round(seed: int):
    """One round: a list of calls, each (entry, width kinds' requests) -- entry "text" or "docset"; a request is
    (kind, query spec, ranges).  Query spec: text (term ids, need, must) / docset (range32 over the int column or None).  The first
    three requests of every round are built to hold a range with count 0, a range that holds every valued hit, and two overlapping
    non-empty ranges; the rest is drawn."""
    rnd = random.Random(9000 + seed)
    calls = []
    for entry in ("text", "docset"):
        for width in (("int", "float"), ("long", "double")):
            reqs = []
            n_req = rnd.randint(3, 6)
            for i in range(n_req):
                kind = rnd.choice(width)
                sp = sorted_pool(kind)
                if entry == "text":
                    terms = tuple(rnd.choice([1, 2, 3, 4]) for _ in range(rnd.randint(1, 3)))
                    must = rnd.random() < 0.3
                    need = len(terms) if must else rnd.randint(1, min(2, len(terms)))
                    spec = (terms, need, must)
                else:
                    spec = None if rnd.random() < 0.5 else (bits_of("int", rnd.choice([-1000, -1, 0])), bits_of("int", rnd.choice([8, 500, 2**31 - 1])))
                if i == 0:      # a range nothing lies in; everything; an overlapping pair around the pool's middle
                    if entry == "text":
                        spec = ((1,), 1, False)
                    ranges = [GAP[kind], (LEAST[kind], GREATEST[kind]), (sp[0], sp[len(sp) // 2]), (sp[1], sp[-1])]
                else:
                    ranges = []
                    for _ in range(rnd.choice([1, 2, 3, 5, 17, 64])):
                        a, b = rnd.choice(sp), rnd.choice(sp)
                        shape = rnd.random()
                        if shape < 0.15:
                            b = a
                        elif shape < 0.3:
                            a, b = (LEAST[kind], b) if rnd.random() < 0.5 else (a, GREATEST[kind])
                        elif shape < 0.9 and order_int(kind, a) > order_int(kind, b):
                            a, b = b, a          # (the rest stay as drawn: one in ten is an empty range)
                        ranges.append((a, b))
                reqs.append((kind, spec, ranges))
            calls.append((entry, reqs))
    return calls


def fuzz_expect(corpus, columns, entry: str, request):
    kind, spec, ranges = request
    if entry == "text":
        hits = text_hits(corpus, spec[0], spec[1])
    else:
        hits = docset_hits(corpus, ranges32=() if spec is None else ((columns["int"], "int", spec[0], spec[1]),))
    return count(corpus, hits, columns[kind], kind, ranges)
