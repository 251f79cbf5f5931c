"""The hand-built corpus, the assignment matrix and the expected lookup structures shared by tests/test_lookup_policy_host.py
(through tests/mockhip/lookup_policy.py: the selection rule alone, no kernel) and tests/test_lookup_structures_gpu.py (the
MaxScore walk's three doc -> posting lookup paths against the oracle).  No test lives here.

What a term is given is written down twice, both from the rule as the comment above segment.cpp: build_term_aux states it and
neither by asking the library: `expected_assignment`, a plain restatement of the rule for every term of every case, and
`PINNED`, literal (kind, shift, bytes) worked out by hand for the terms a case is about.  The host test holds the library to
both, so the restatement cannot drift from the arithmetic in the comments below."""
import dataclasses

import numpy as np

from nrtsearch_amd import synth

NONE, BITS, CELLS = 0, 1, 2          # plan.h: kLookNone, kLookBits, kLookCells
MIN_POSTINGS = 64                    # segment.cpp: kLookMinPostings
DEFAULT_PCT = 150                    # segment.cpp: kLookBudgetPct
DEFAULT_POLICY = "bits@256,cells"    # segment.cpp: kLookPolicy
PACK_DOC_BITS = 20                   # plan.h: kPackDocBits -- a lookup cell of a packed context is one 2^20-doc super-window at most

# one multiple of 32 (and of the 1024-doc tile), one 32k + 1, one that is neither; three segments, the first without ABSENT
MAX_DOCS = (2048, 65_537, 200_003)
DENSE, PER100, PER256, UNDER256, P63, P64, P65, ENDS, LAST32, TILE300, ABSENT = range(1, 12)
NAMES = {DENSE: "dense", PER100: "per100", PER256: "per256", UNDER256: "under256", P63: "p63", P64: "p64", P65: "p65", ENDS: "ends",
         LAST32: "last32", TILE300: "tile300", ABSENT: "absent"}


def term_docs(term: int, n: int, seg_index: int):
    """The docids of `term` in a segment of n docs (ascending), None when the segment does not hold the term."""
    a = np.arange
    if term == DENSE:
        return a(0, n, 2)                                   # every 2nd doc
    if term == PER100:
        return a(0, n, 100)
    if term == PER256:
        return a(0, n, 256)                                 # a posting per 256 docs exactly: count * 256 >= n
    if term == UNDER256:
        return a(100, n, 256)                               # one posting fewer: count * 256 < n where n is no multiple of 256
    if term in (P63, P64, P65):
        c = {P63: 63, P64: 64, P65: 65}[term]
        return 7 + a(c) * ((n - 16) // c)
    if term == ENDS:
        return a(100) * (n - 1) // 99                       # doc 0 and doc n - 1, 98 between them
    if term == LAST32:
        return a(n - 32, n)
    if term == TILE300:                                     # 300 postings inside one 1024-doc tile: a long search in one cell
        tile = min(37, n // 1024 - 1)
        rng = np.random.Generator(np.random.PCG64(300 + seg_index))
        return tile * 1024 + np.sort(rng.choice(1024, size=300, replace=False))
    if term == ABSENT:
        return None if seg_index == 0 else a(3, n, 50)
    raise ValueError(term)


def build_corpus(delete_fraction: float = 0.0) -> synth.Corpus:
    """Freqs <= 12 except 3 % in 13..300 (exception postings of the packed layout); norm bytes < 128 (doc lengths <= 4000), so
    that every query keeps the fixed-point accumulators and with them the MaxScore route."""
    segments, doc_freq, base, total_len = [], {}, 0, 0
    for si, n in enumerate(MAX_DOCS):
        rng = np.random.Generator(np.random.PCG64(9000 + si))
        lens = synth.doc_lengths(n, seed=77 + si)
        ids, offs, docs, freqs = [], [0], [], []
        for t in sorted(NAMES):
            d = term_docs(t, n, si)
            if d is None:
                continue
            d = np.asarray(d, dtype=np.int64)
            assert len(d) and d[0] >= 0 and d[-1] < n and np.all(np.diff(d) > 0), (t, n)
            f = rng.integers(1, 13, size=len(d), dtype=np.int32)
            hot = rng.random(len(d)) < 0.03
            f[hot] = rng.integers(13, 301, size=int(hot.sum()), dtype=np.int32)
            ids.append(t)
            docs.append(d.astype(np.int32))
            freqs.append(f)
            offs.append(offs[-1] + len(d))
            doc_freq[t] = doc_freq.get(t, 0) + len(d)
        live = None
        if delete_fraction > 0.0:
            alive = np.random.Generator(np.random.PCG64(555 + si)).random(n) >= delete_fraction
            padded = np.zeros(((n + 63) // 64) * 64, dtype=bool)
            padded[:n] = alive
            live = np.packbits(padded.reshape(-1, 64), axis=1, bitorder="little").view(np.uint64).reshape(-1)
        norms = synth.int_to_byte4(lens)
        assert int(norms.max()) < 128
        segments.append(synth.SegmentData(max_doc=n, doc_base=base, norms=norms, term_ids=np.array(ids, np.int64),
                                          offsets=np.array(offs, np.int64), docids=np.concatenate(docs), freqs=np.concatenate(freqs),
                                          live_bits=live))
        base += n
        total_len += int(lens.astype(np.int64).sum())
    return synth.Corpus(n_docs=base, doc_count=base, sum_total_term_freq=total_len, segments=segments, doc_freq=doc_freq)


# ---- the rule, restated (segment.cpp, the comment above build_term_aux) -------------------------------------------------
def bits_bytes(max_doc: int) -> int:
    """Records: 8 bytes per 32 docs and one record of slack, 16-byte aligned."""
    return (((max_doc + 31) // 32 + 1) * 8 + 15) & ~15


def cells_shift_bytes(count: int, max_doc: int, packed: bool):
    """Lookup cells of 2^shift docs: the largest power of two with at most one posting per cell on average (a packed context:
    2^20 docs at the most); one 4-byte entry per cell, entry 0 and one entry of slack, 16-byte aligned."""
    shift = 0
    while shift < (PACK_DOC_BITS if packed else 31) and (count << (shift + 1)) <= max_doc:
        shift += 1
    n_cells = ((max_doc - 1) >> shift) + 1
    return shift, ((n_cells + 2) * 4 + 15) & ~15


def parse_policy(text: str):
    """"kind:N" the N largest terms of the upload group, "kind@D" terms with a posting per D docs or more, "kind" every term."""
    rules = []
    for item in text.split(","):
        name, rank, density = item, None, None
        if ":" in item:
            name, v = item.split(":")
            rank = int(v)
        elif "@" in item:
            name, v = item.split("@")
            density = int(v)
        if name in ("bits", "cells"):
            rules.append((BITS if name == "bits" else CELLS, rank, density))
    return rules


def expected_assignment(counts, max_doc: int, policy: str, pct: int, packed: bool):
    """(kind, shift, bytes) per term of ONE upload group, in add order.  Terms of 64 postings or more are served largest first
    (ties: the term added first) by the first rule that applies to the term and whose structure the rest of the budget pays for;
    the budget is pct % (0: the default, negative: nothing) of the group's resident posting bytes, 8 per posting, 4 when packed."""
    budget = sum(counts) * (4 if packed else 8) * (DEFAULT_PCT if pct == 0 else max(pct, 0)) // 100
    out = [(NONE, 0, 0)] * len(counts)
    order = sorted((i for i, c in enumerate(counts) if c >= MIN_POSTINGS), key=lambda i: (-counts[i], i))
    for rank, i in enumerate(order):
        for kind, rank_limit, density in parse_policy(policy):
            if rank_limit is not None and rank >= rank_limit:
                continue
            if density is not None and counts[i] * density < max_doc:
                continue
            shift, cost = (0, bits_bytes(max_doc)) if kind == BITS else cells_shift_bytes(counts[i], max_doc, packed)
            if cost > budget:
                continue          # a later rule's structure may fit
            budget -= cost
            out[i] = (kind, shift, cost)
            break
    return out


# ---- the assignment matrix ---------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    policy: str      # NRTGPU_LOOK_POLICY of the development build, read at every seal
    pct: int         # nrtgpu_config.lookup_budget_pct
    packed: bool     # NRTGPU_FLAG_PACKED_POSTINGS


# "small": the budget that pays for the records of the two largest terms of the 200 003-doc segment and then runs out mid-list.
# The same BYTES under both layouts (12 % of 8 B per posting = 24 % of 4 B): what each layout makes of the same percentage is
# pinned by the host test's own "small12_packed" case.
SMALL_PCT = {False: 12, True: 24}
MATRIX = [Case(f"{name}_{'packed' if packed else 'plain'}", policy, pct if pct != "small" else SMALL_PCT[packed], packed)
          for packed in (False, True)
          for name, policy, pct in (("default_none", DEFAULT_POLICY, -1), ("default_small", DEFAULT_POLICY, "small"),
                                    ("default_default", DEFAULT_POLICY, 0), ("default_100000", DEFAULT_POLICY, 100000),
                                    ("bits", "bits", 100000), ("cells", "cells", 100000), ("norule", "", 100000),
                                    ("bits1_cells", "bits:1,cells", 100000))]


def expected_for(case: Case, corpus: synth.Corpus):
    """[{term id: (kind, shift, bytes)}] per segment of the corpus, uploaded as ONE group per segment (api.GpuSegment.from_data)."""
    out = []
    for seg in corpus.segments:
        counts = [int(c) for c in np.diff(seg.offsets)]
        out.append(dict(zip((int(t) for t in seg.term_ids), expected_assignment(counts, seg.max_doc, case.policy, case.pct, case.packed))))
    return out


# ---- the same, by hand, for the terms each case is about: PINNED[case][segment index][term] = (kind, shift, bytes) ----------
# Postings per term.  2048 docs: dense 1024, per100 21, per256 8, under256 8, p63/p64/p65, ends 100, last32 32, tile300 300
# (1685 in all).  65 537 docs: dense 32769, per100 656, per256 257 (257 * 256 = 65792 >= 65537), under256 256 (256 * 256 = 65536
# = max_doc - 1: NOT a posting per 256 docs), absent 1311.  200 003 docs: dense 100002, absent 4000, per100 2001, per256 782
# (782 * 256 = 200192 >= 200003), under256 781 (781 * 256 = 199936 < 200003), tile300 300, ends 100, p65, p64, p63, last32 32:
# 108190 postings, 865520 B in two columns, 432760 B packed.
# Records: ((max_doc + 31) / 32 + 1) * 8 -> 528 B (2048 docs), 16400 B (65 537: 2049 blocks, 16400 = 16-aligned), 50016 B (200 003).
# Cells, 200 003 docs: absent 4000 << 5 <= 200003 < 4000 << 6: shift 5, 6251 cells, 25024 B; per100: shift 6, 3126 cells, 12512 B;
# per256: shift 7, 1563 cells, 6272 B; under256: 781 << 8 = 199936 <= 200003: shift 8, 782 cells, 3136 B; tile300: shift 9, 391
# cells, 1584 B; ends: shift 10, 196 cells, 800 B; p65 and p64: shift 11, 98 cells, 400 B; dense: shift 0, 200003 cells, 800032 B.
_B200, _B65, _B2 = 50016, 16400, 528
_DEFAULT_200 = {DENSE: (BITS, 0, _B200), ABSENT: (BITS, 0, _B200), PER100: (BITS, 0, _B200), PER256: (BITS, 0, _B200),
                UNDER256: (CELLS, 8, 3136), TILE300: (CELLS, 9, 1584), ENDS: (CELLS, 10, 800), P65: (CELLS, 11, 400), P64: (CELLS, 11, 400),
                P63: (NONE, 0, 0), LAST32: (NONE, 0, 0)}
# 65 537 docs: under256 256 << 8 = 65536 <= 65537: shift 8, 257 cells, 1036 -> 1040 B; p64 64 << 10 = 65536: shift 10, 65 cells, 268
# -> 272 B; p65 65 << 9 = 33280, 65 << 10 = 66560 > 65537: shift 9, 129 cells, 524 -> 528 B
_DEFAULT_65 = {DENSE: (BITS, 0, _B65), PER256: (BITS, 0, _B65), UNDER256: (CELLS, 8, 1040), P63: (NONE, 0, 0), P64: (CELLS, 10, 272),
               P65: (CELLS, 9, 528), LAST32: (NONE, 0, 0)}
# 2048 docs: 64 * 256 >= 2048 -- every term that reaches 64 postings is "dense" here
_DEFAULT_2 = {DENSE: (BITS, 0, _B2), TILE300: (BITS, 0, _B2), ENDS: (BITS, 0, _B2), P65: (BITS, 0, _B2), P64: (BITS, 0, _B2), P63: (NONE, 0, 0),
              PER100: (NONE, 0, 0), LAST32: (NONE, 0, 0)}
# the small budget, 200 003 docs: 865520 * 12 / 100 = 432760 * 24 / 100 = 103862 B.  dense and absent take records: 3830 B left.
# per100: records no, cells 12512 no.  per256: 6272 no.  under256: 3136 yes, 694 left.  tile300 1584 no, ends 800 no, p65 400 yes,
# 294 left, p64 400 no.  (A budget running out mid-list, and smaller structures behind the first refusal still served.)
_SMALL_200 = {DENSE: (BITS, 0, _B200), ABSENT: (BITS, 0, _B200), PER100: (NONE, 0, 0), PER256: (NONE, 0, 0), UNDER256: (CELLS, 8, 3136),
              TILE300: (NONE, 0, 0), ENDS: (NONE, 0, 0), P65: (CELLS, 11, 400), P64: (NONE, 0, 0), P63: (NONE, 0, 0), LAST32: (NONE, 0, 0)}
_ALL_NONE = [{t: (NONE, 0, 0) for t in NAMES if not (si == 0 and t == ABSENT)} for si in range(3)]
PINNED = {}
for _p in ("plain", "packed"):
    PINNED[f"default_none_{_p}"] = _ALL_NONE
    PINNED[f"norule_{_p}"] = _ALL_NONE
    PINNED[f"default_default_{_p}"] = [_DEFAULT_2, _DEFAULT_65, _DEFAULT_200]
    PINNED[f"default_100000_{_p}"] = [_DEFAULT_2, _DEFAULT_65, _DEFAULT_200]
    PINNED[f"default_small_{_p}"] = [{}, {}, _SMALL_200]
    # "bits": a sparse term gets records; "cells": the dense term gets cells of ONE doc (shift 0; 2048 docs: 1024 << 1 = 2048 <= 2048,
    # shift 1, 1024 cells, 4104 -> 4112 B; 65 537 docs: shift 0, 65537 cells, 262156 -> 262160 B)
    PINNED[f"bits_{_p}"] = [{P64: (BITS, 0, _B2), P63: (NONE, 0, 0)}, {P64: (BITS, 0, _B65), UNDER256: (BITS, 0, _B65)},
                            {P64: (BITS, 0, _B200), ENDS: (BITS, 0, _B200), DENSE: (BITS, 0, _B200), P63: (NONE, 0, 0)}]
    PINNED[f"cells_{_p}"] = [{DENSE: (CELLS, 1, 4112), P63: (NONE, 0, 0)}, {DENSE: (CELLS, 0, 262160), PER256: (CELLS, 7, 2064)},
                             {DENSE: (CELLS, 0, 800032), ABSENT: (CELLS, 5, 25024), PER100: (CELLS, 6, 12512), PER256: (CELLS, 7, 6272)}]
    # "bits:1,cells": records for the largest term of the group alone
    PINNED[f"bits1_cells_{_p}"] = [{DENSE: (BITS, 0, _B2), TILE300: (CELLS, 2, 2064)}, {DENSE: (BITS, 0, _B65), ABSENT: (CELLS, 5, 8208)},
                                   {DENSE: (BITS, 0, _B200), ABSENT: (CELLS, 5, 25024), P64: (CELLS, 11, 400)}]
# 12 % of the PACKED bytes of the 200 003-doc segment: 432760 * 12 / 100 = 51931 B -- records for dense alone (1915 left), then
# nothing fits until tile300's 1584 B (331 left).  At 8 B per posting the same 12 % pays what _SMALL_200 lists.
SMALL12_PACKED_200 = {DENSE: (BITS, 0, _B200), ABSENT: (NONE, 0, 0), PER100: (NONE, 0, 0), PER256: (NONE, 0, 0), UNDER256: (NONE, 0, 0),
                      TILE300: (CELLS, 9, 1584), ENDS: (NONE, 0, 0), P65: (NONE, 0, 0), P64: (NONE, 0, 0)}
