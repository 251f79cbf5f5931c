"""The column routes at the layout boundaries -- sort by field, terms counts and doc-set requests over single-valued and
multi-valued columns, through the C ABI on the device, against the four NumPy references -- with max_doc on and next to the
64-doc mask word, the 1024-doc sub-tile (csrc/plan.h: kTileDocs) and the 12 288-doc round (kScanWaves x kTileDocs), and with
items whose sub-tiles cross from one leaf into the next on such a boundary.  The cases and what each must return come from
tests/_column_cases.py (sweep_case: the layouts, the columns whose edge docs decide the answers, the requests); here are the
upload, the calls and the comparisons: exact equality of every output field.  Needs a real MI355X."""
import numpy as np
import pytest

from nrtsearch_amd import api

from tests import _column_cases as cc
from tests import _field_sort_ref as fs
from tests import test_docset_gpu as dg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def two_column_postings():
    """The text routes over a column refuse packed postings: the contexts here keep the two-column layout whatever the suite runs under."""
    mp = pytest.MonkeyPatch()
    mp.delenv("NRTGPU_PACKED_POSTINGS", raising=False)
    yield
    mp.undo()


@pytest.fixture(scope="module")
def ctx(two_column_postings):
    c = api.GpuContext(device_id=0, max_batch=256)
    yield c
    c.close()


def upload(ctx, m: cc.Model, stray_bits: bool = False):
    """The model's leaves on the device -> (leaves, searcher).  stray_bits: the liveDocs and mask words carry ones at and beyond max_doc."""
    leaves = []
    for si, seg in enumerate(m.corpus.segments):
        g = api.GpuSegment(ctx, seg.max_doc, seg.doc_base)
        leaves.append(g)
        g.add_field_norms(0, seg.norms)
        g.add_terms(0, seg.term_ids, seg.offsets, seg.docids, seg.freqs)
        for key, cols in m.columns.items():
            if cols[si] is None:
                continue
            docs, bits = cols[si] if len(cols[si][1]) else cc._no_values()
            if key[0] == "m":
                g.add_doc_values_multi(m.field[key], key[1], bits, docs)
            else:
                g.add_doc_values(m.field[key], key[1], bits, docs)
        g.seal()
        if seg.live_bits is not None:
            g.set_live_docs(cc.dirty(seg.live_bits, seg.max_doc) if stray_bits else seg.live_bits)
        for mid, words in m.masks.items():
            g.set_mask(mid, cc.dirty(words[si], seg.max_doc) if stray_bits else words[si])
    return leaves, api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics.from_corpus(m.corpus))


def supported(searcher, m: cc.Model, r: cc.Req) -> bool:
    q = cc.query_of(m, r)
    if r.entry == "sorted":
        return api.sorted_supported(searcher, q, cc.manager_of(r), cc.sort_of(m, r), cc.after_of(r))
    if r.entry == "docset_sorted":
        return api.docset_sorted_supported(searcher, q, cc.manager_of(r), cc.sort_of(m, r), cc.after_of(r))
    if r.entry == "count":
        return api.count_terms_supported(searcher, q, cc.collector_of(m, r), r.max_buckets)
    return api.count_docset_terms_supported(searcher, q, cc.collector_of(m, r), r.max_buckets)


def run(searcher, m: cc.Model, entry: str, reqs):
    """one call of the entry over the requests (at most the context's max_batch of them)"""
    queries = [cc.query_of(m, r) for r in reqs]
    if entry.endswith("sorted"):
        call = api.search_sorted_batch if entry == "sorted" else api.search_docset_sorted_batch
        return call(searcher, queries, [cc.manager_of(r) for r in reqs], [cc.sort_of(m, r) for r in reqs], [cc.after_of(r) for r in reqs])
    call = api.count_terms_batch if entry == "count" else api.count_docset_terms_batch
    return call(searcher, queries, [cc.collector_of(m, r) for r in reqs], [r.max_buckets for r in reqs])


def check(name: str, m: cc.Model, r: cc.Req, got):
    """every output field against the reference; every docid below the index's doc count"""
    if r.sorts:
        dg.same_docs(name, got, m.expected(r))
        assert len(got.docs) == 0 or (0 <= int(got.docs.min()) and int(got.docs.max()) < m.n_docs), f"{name}: a docid at or beyond {m.n_docs}"
    else:
        dg.same_counts(name, got, m.expected(r))


def has_value(m: cc.Model, key) -> int:
    """the docs that have a value in the column"""
    return sum(0 if col is None else (seg.max_doc if col[0] is None else len(np.unique(col[0]))) for seg, col in zip(m.corpus.segments, m.columns[key]))


@pytest.mark.parametrize("deletes", [False, True], ids=["all_live", "deletes"])
@pytest.mark.parametrize("layout", cc.LAYOUTS, ids=["x".join(str(n) for n in l) for l in cc.LAYOUTS])
def test_boundary_layout(ctx, layout, deletes):
    m, reqs = cc.sweep_case(layout, deletes)
    assert all((seg.live_bits is not None) == deletes for seg in m.corpus.segments)   # all live: the nullptr paths
    variants = [False] + ([True] if any(n % 64 for n in layout) else [])   # clean words; then ones at and beyond max_doc: ignored
    for stray_bits in variants:
        leaves, searcher = upload(ctx, m, stray_bits)
        try:
            for entry in cc.ENTRIES:
                rs = reqs[entry]
                for lo in range(0, len(rs), 256):
                    got = run(searcher, m, entry, rs[lo: lo + 256])
                    for i, (r, g) in enumerate(zip(rs[lo: lo + 256], got)):
                        name = f"layout {layout}, deletes {deletes}, stray bits {stray_bits}, {entry}[{lo + i}]: {cc.describe(r)}"
                        assert supported(searcher, m, r) is True, name
                        check(name, m, r, g)
                        # a [kind min, kind max] range alone, nobody deleted: the docs that HAVE a value, never a padded slot more
                        if r.docset and not deletes and len(r.ranges) == 1 and not r.filters and not r.must_nots:
                            assert g.total_hits == has_value(m, r.ranges[0][0]), name
        finally:
            dg.release(leaves)


# ---- named cases, spelled out by hand; a mismatch that the sweep or the fuzz (tests/test_fuzz_columns_gpu.py) finds is added here ---------
def test_a_padded_slot_is_no_doc(ctx):
    """One leaf of 1025 docs (two sub-tiles, the second holding ONE doc), a dense int column without INT32_MIN, nobody deleted:
    ascending with the missing value INT32_MAX a padded slot would rank first, and a full-range clause would count it."""
    n = 1025
    corpus = fs.make_corpus([n], {cc.ALL: 1.0}, seed=3)
    key = ("s", "int", "dense")
    m = cc.Model(corpus, {}, {key: [(None, dg._i(np.arange(n) % 7 + 5))]})
    leaves, searcher = upload(ctx, m)
    try:
        full = ((key, fs.KIND_MIN["int"], fs.KIND_MAX["int"]),)
        for entry, hs in (("sorted", dict(clauses=(cc.ALL,))), ("docset_sorted", dict()), ("docset_sorted", dict(ranges=full))):
            rs = [cc.Req(entry, column=key, k=k, reverse=rev, missing=fs.KIND_MAX["int"], **hs) for k in (1, 1024) for rev in (False, True)]
            for r, g in zip(rs, run(searcher, m, entry, rs)):
                check(f"{entry}: {cc.describe(r)}", m, r, g)
                assert g.total_hits == n and int(g.values.min()) >= 5
        for entry, hs in (("count", dict(clauses=(cc.ALL,))), ("docset_count", dict()), ("docset_count", dict(ranges=full))):
            rs = [cc.Req(entry, column=key, max_buckets=b, **hs) for b in (7, 6)]
            got = run(searcher, m, entry, rs)
            for r, g in zip(rs, got):
                check(f"{entry}: {cc.describe(r)}", m, r, g)
            assert got[0].values.tolist() == list(range(5, 12)) and got[0].hits_with_value == n and got[1].overflowed
    finally:
        dg.release(leaves)
