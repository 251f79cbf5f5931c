"""The routes over 64-bit doc value columns at the layout boundaries -- sort by a LONG / DOUBLE field over a text query and over a doc
set, masks built from such columns, range counts over them -- through the C ABI on the device, against the NumPy references, with
max_doc on and next to the 64-doc mask word, the 1024-doc sub-tile and the 12 288-doc round, items whose sub-tiles cross from one
leaf into the next, columns that are absent from a leaf or empty on it, and sparse columns that do and do not end on the last doc.
The cases and what each must return come from tests/_column64_cases.py (sweep_case); here are the upload, the calls and the
comparisons: exact equality of every output field.  Needs a real MI355X."""
import numpy as np
import pytest

from nrtsearch_amd import _lib, api

from tests import _column64_cases as c64
from tests import _column_cases as cc
from tests import _field_sort64_ref as f64
from tests import _field_sort_ref as fs
from tests import _value_masks64_ref as vm
from tests import _value_masks_ref as vm32
from tests import test_field_sort64_gpu as s64     # same, release
from tests import test_range_count_gpu as rcg      # same

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


def upload(ctx, m: c64.Model, stray_bits: bool = False):
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
            docs, bits = cols[si]
            if key[1] in c64.KINDS:
                g.add_doc_values64(m.field[key], key[1], bits, docs)
            elif key[0] == "m":
                g.add_doc_values_multi(m.field[key], key[1], bits, docs)
            else:
                g.add_doc_values(m.field[key], key[1], bits, docs)
        g.seal()
        if seg.live_bits is not None:
            g.set_live_docs(cc.dirty(seg.live_bits, seg.max_doc) if stray_bits else seg.live_bits)
        for mid, words in m.masks.items():
            g.set_mask(mid, cc.dirty(words[si], seg.max_doc) if stray_bits else words[si])
    return leaves, api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics.from_corpus(m.corpus))


def supported(searcher, m: c64.Model, r: c64.Req) -> bool:
    q = c64.query_of(m, r)
    if r.entry == "sorted64":
        return api.sorted64_supported(searcher, q, c64.manager_of(r), c64.sort_of(m, r), c64.after_of(r))
    if r.entry == "docset_sorted64":
        return api.docset_sorted64_supported(searcher, q, c64.manager_of(r), c64.sort_of(m, r), c64.after_of(r))
    if r.entry == "ranges64":
        return api.count_ranges_supported(searcher, q, c64.counter_of(m, r))
    return api.count_docset_ranges_supported(searcher, q, c64.counter_of(m, r))


def run(searcher, m: c64.Model, entry: str, reqs):
    """one call of a batch entry over the requests (at most the context's max_batch of them)"""
    queries = [c64.query_of(m, r) for r in reqs]
    if entry.endswith("sorted64"):
        call = api.search_sorted64_batch if entry == "sorted64" else api.search_docset_sorted64_batch
        return call(searcher, queries, [c64.manager_of(r) for r in reqs], [c64.sort_of(m, r) for r in reqs], [c64.after_of(r) for r in reqs])
    call = api.count_ranges_batch if entry == "ranges64" else api.count_docset_ranges_batch
    return call(searcher, queries, [c64.counter_of(m, r) for r in reqs])


def check(name: str, m: c64.Model, r: c64.Req, got):
    """every output field against the reference; every docid below the index's doc count"""
    if r.sorts:
        s64.same(name, got, m.expected(r))
        assert len(got.docs) == 0 or (0 <= int(got.docs.min()) and int(got.docs.max()) < m.n_docs), f"{name}: a docid at or beyond {m.n_docs}"
    else:
        rcg.same(name, got, m.expected(r))


def check_mask(name: str, m: c64.Model, r: c64.Req, leaves):
    """set_mask_from_values64 then get_mask on the request's leaf: every word and the count; bits at or beyond max_doc are 0"""
    leaf, n = leaves[r.leaf], m.sizes[r.leaf]
    count = leaf.set_mask_from_values64(30, c64.clauses_of(m, r))
    words = leaf.get_mask(30)
    exp_words, exp_count = m.expected(r)
    assert words.tolist() == exp_words.tolist(), f"{name}: words"
    assert count == exp_count, f"{name}: count {count}, the reference has {exp_count}"
    assert n % 64 == 0 or int(words[-1]) >> (n % 64) == 0, f"{name}: bits at or beyond max_doc"
    return count


@pytest.mark.parametrize("deletes", [False, True], ids=["all_live", "deletes"])
@pytest.mark.parametrize("layout", cc.LAYOUTS, ids=["x".join(str(n) for n in l) for l in cc.LAYOUTS])
def test_boundary_layout(ctx, layout, deletes):
    m, reqs = c64.sweep_case(layout, deletes)
    assert all((seg.live_bits is not None) == deletes for seg in m.corpus.segments)   # all live: the nullptr paths
    variants = [False] + ([True] if any(n % 64 for n in layout) else [])   # clean words; then ones at and beyond max_doc: ignored
    for stray_bits in variants:
        leaves, searcher = upload(ctx, m, stray_bits)
        try:
            with_value = {}     # column -> hits_with_value of the full range under match-all
            for entry in c64.BATCH_ENTRIES:
                fit = [r for r in reqs[entry] if not r.sorts or m.fits(r.column)]
                for r in reqs[entry]:
                    name = f"layout {layout}, deletes {deletes}, stray bits {stray_bits}, {entry}: {c64.describe(r)}"
                    assert supported(searcher, m, r) is (not r.sorts or m.fits(r.column)), name   # the predicate equals the module's own fit verdict
                    if r.sorts and not m.fits(r.column):
                        with pytest.raises(_lib.NrtGpuError) as e:
                            run(searcher, m, entry, [r])
                        assert e.value.code == _lib.NRTGPU_ERR_UNSUPPORTED and f"{m.doc_bits()}-bit docids leave {64 - m.doc_bits()}" in str(e.value), f"{name}: {e.value}"
                for lo in range(0, len(fit), 256):
                    got = run(searcher, m, entry, fit[lo: lo + 256])
                    for i, (r, g) in enumerate(zip(fit[lo: lo + 256], got)):
                        name = f"layout {layout}, deletes {deletes}, stray bits {stray_bits}, {entry}[{lo + i}]: {c64.describe(r)}"
                        check(name, m, r, g)
                        if entry == "docset_ranges64" and not (r.filters or r.must_nots or r.ranges) and r.count_ranges == ((c64.KIND_MIN[r.column[1]], c64.KIND_MAX[r.column[1]]),):
                            assert g.hits_with_value == int(g.counts[0])
                            with_value[r.column] = g.hits_with_value
            counted = {}        # column -> the docs of its [kind min, kind max] masks, over the leaves
            for i, r in enumerate(reqs["mask64"]):
                count = check_mask(f"layout {layout}, deletes {deletes}, mask64[{i}]: {c64.describe(r)}", m, r, leaves)
                if len(r.value_clauses) == 1 and r.value_clauses[0][1:] == ("range", c64.KIND_MIN[r.value_clauses[0][0][1]], c64.KIND_MAX[r.value_clauses[0][0][1]]):
                    counted[r.value_clauses[0][0]] = counted.get(r.value_clauses[0][0], 0) + count
            # a [kind min, kind max] mask counts the docs that HAVE a value, never a padded slot more -- and, nobody deleted, so does
            # the full-range count under match-all
            assert set(counted) == set(c64.SORT_COLUMNS) == set(with_value)
            for key, count in counted.items():
                assert count == m.value_docs(key), (layout, key)
                if not deletes:
                    assert count == with_value[key], (layout, key)
        finally:
            s64.release(leaves)


# ---- named cases, spelled out by hand; a mismatch that the sweep or the fuzz (tests/test_fuzz_columns64_gpu.py) finds is added here ------
def test_a_padded_slot_is_no_doc(ctx):
    """One leaf of 1025 docs (two sub-tiles, the second holding ONE doc), a dense long column with no value near INT64_MIN, nobody
    deleted: ascending with the missing value INT64_MAX a padded slot (code 0) would rank first, and a full-range mask would count it."""
    n = 1025
    corpus = fs.make_corpus([n], {cc.ALL: 1.0}, seed=3)
    key = ("s", "long", "dense")
    values = c64.EPOCH + (np.arange(n, dtype=np.int64) % 7) * 86_400_000
    m = c64.Model(corpus, {}, {key: [(None, values.view(np.uint64))]})
    leaves, searcher = upload(ctx, m)
    try:
        for entry, hs in (("sorted64", dict(clauses=(cc.ALL,))), ("docset_sorted64", dict())):
            rs = [c64.Req(entry, column=key, k=k, reverse=rev, missing=c64.KIND_MAX["long"], **hs) for k in (1, 1024) for rev in (False, True)]
            for r, g in zip(rs, run(searcher, m, entry, rs)):
                check(f"{entry}: {c64.describe(r)}", m, r, g)
                assert g.total_hits == n and int(g.values.min()) >= c64.EPOCH
        full = c64.Req("mask64", value_clauses=((key, "range", c64.KIND_MIN["long"], c64.KIND_MAX["long"]),))
        assert check_mask("full range", m, full, leaves) == n
        for entry, hs in (("ranges64", dict(clauses=(cc.ALL,))), ("docset_ranges64", dict())):
            r = c64.Req(entry, column=key, count_ranges=((c64.KIND_MIN["long"], c64.KIND_MAX["long"]), (c64.KIND_MIN["long"], f64.bits_of("long", c64.EPOCH - 1))), **hs)
            g = run(searcher, m, entry, [r])[0]
            check(entry, m, r, g)
            assert g.counts.tolist() == [n, 0] and g.hits_with_value == n
    finally:
        s64.release(leaves)


def test_the_grid_strides_second_trip(ctx):
    """One leaf of 2048 x 4 x 64 + 65 docs: the mask kernels' grid is capped at 2048 blocks of 4 waves, a wave builds one 64-doc word
    per trip, so the words from 524 288 docs on -- the 65-doc tail -- are built on a second trip of the grid-stride loop.  A sparse
    long and a sparse int column whose values are a function of the docid; a range and an exists clause over each; every word."""
    n = 2048 * 4 * 64 + 65
    g = api.GpuSegment(ctx, n, 0)
    try:
        d = np.arange(n, dtype=np.int64)
        d64, d32 = np.nonzero(d % 3 != 1)[0].astype(np.int32), np.nonzero(d % 5 != 3)[0].astype(np.int32)
        assert int(d64[-1]) == n - 1 and int(d32[-1]) == n - 1   # the last doc of the tail word holds values (a third / a fifth of the tail's docs hold none)
        v64 = (c64.EPOCH + (d64.astype(np.int64) * 2_654_435_761) % 2**36 - 2**35).view(np.uint64)     # spread over 36 bits around the epoch
        v32 = ((d32.astype(np.int64) * 7919) % 2001 - 1000).astype(np.int32).view(np.uint32)
        g.add_doc_values64(7, "long", v64, d64)
        g.add_doc_values(8, "int", v32, d32)
        g.seal()
        lo64, hi64 = f64.bits_of("long", c64.EPOCH - 2**33), f64.bits_of("long", c64.EPOCH + 2**34)
        lo32, hi32 = fs.bits_of("int", -250), fs.bits_of("int", 600)
        for name, clauses, exp in (
                ("range64", [api.ValueClause64("range", 7, "long", lo64, hi64)], vm.mask(n, [((d64, v64), "long", ("range", lo64, hi64))])),
                ("exists64", [api.ValueClause64.exists(7)], vm.mask(n, [((d64, v64), "long", ("exists",))]))):
            count, words = g.set_mask_from_values64(30, clauses), g.get_mask(30)
            assert words.tolist() == exp.tolist(), name
            assert count == int(fs._bits(exp, n).sum()) and 0 < int(fs._bits(exp, n)[2048 * 4 * 64:].sum()) < 65, name
        for name, clauses, exp in (
                ("range32", [api.ValueClause.range_(8, "int", -250, 600)], vm32.mask_words(n, [(("single", d32, v32), ("range", "int", lo32, hi32))])[0]),
                ("exists32", [api.ValueClause.exists(8)], vm32.mask_words(n, [(("single", d32, v32), ("exists",))])[0])):
            count, words = g.set_mask_from_values(31, clauses), g.get_mask(31)
            assert words.tolist() == exp.tolist(), name
            assert count == int(fs._bits(exp, n).sum()) and 0 < int(fs._bits(exp, n)[2048 * 4 * 64:].sum()) < 65, name
    finally:
        g.release()


@pytest.mark.parametrize("column", ["pos", "naninf"])
def test_a_nan_missing_value_with_a_payload_comes_back_canonical(ctx, column):
    """The missing value 0x7FF8000000000123 over `pos` (no NaN in the column: the missing value lies outside the window, a sentinel)
    and over `naninf` (the column holds NaNs: the missing value's code is the window's greatest), in both directions, on a 3000-doc
    leaf: missing docs and NaN docs tie and rank by docid, and EVERY reported NaN is 0x7FF8000000000000."""
    n = 3000
    corpus = fs.make_corpus([n], {cc.ALL: 1.0}, seed=23)
    rng = np.random.default_rng(24)
    docs = np.nonzero(rng.random(n) < 0.7)[0].astype(np.int32)
    key = ("s", "double", column)
    m = c64.Model(corpus, {}, {key: [(docs, rng.choice(c64.POOLS[("double", column)], size=len(docs)))]})
    assert m.fits(key)
    leaves, searcher = upload(ctx, m)
    try:
        for entry, hs in (("sorted64", dict(clauses=(cc.ALL,))), ("docset_sorted64", dict())):
            rs = [c64.Req(entry, column=key, k=1024, reverse=rev, missing=c64.NAN_PAYLOAD, **hs) for rev in (False, True)]
            for r, g in zip(rs, run(searcher, m, entry, rs)):
                name = f"{entry}: {c64.describe(r)}"
                nans = g.value_bits[(g.value_bits & np.uint64(2**63 - 1)) > np.uint64(c64.PINF)]
                assert len(nans) >= n - len(docs) or not r.reverse                  # descending the NaNs head the page: every missing doc among them
                assert nans.tolist() == [f64.CANONICAL_NAN] * len(nans), f"{name}: a NaN with a payload"
                at = np.nonzero(g.value_bits == np.uint64(f64.CANONICAL_NAN))[0]
                assert g.docs[at].tolist() == sorted(g.docs[at].tolist()), f"{name}: the NaNs rank by docid"
                check(name, m, r, g)
    finally:
        s64.release(leaves)
