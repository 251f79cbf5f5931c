"""The speculative estimate outside the meeting (maxscore.hip: ms_estimate): the wave that finds an estimate due makes it on its
own -- a one-wave selection over the candidate buffer the other eleven waves keep appending to -- instead of stopping the
workgroup.  What must hold: the answers are the oracle's (a guess changes what is skipped, never what is returned), guesses do
not fail on an index whose docs are spread like a sample, and no meeting is called for an estimate any more.
Development library: NRTGPU_MS_SPEC_FIRST=1 makes the estimates fall due at windows 1 and 13 of the 16 doc windows of these
corpora -- while every wave holds a window -- and NRTGPU_MS_SPEC_MEET=1 brings the old meetings back for comparison; the
instrumented kernels count meetings and estimates (nrtgpu_debug_maxscore_meetings).  Needs a real MI355X."""
import numpy as np
import pytest

from nrtsearch_amd import _lib, api, synth

pytestmark = pytest.mark.gpu

RANKS = [1, 2, 5, 9, 20, 60, 150, 400]
QUERIES = [[1, 5, 20, 150, 400], [2, 9, 60], [1, 2, 5, 9, 20, 60, 150, 400], [5, 400], [9, 20, 150]]
SETTINGS = ((1000, 1000), (100, 10), (10, 1000))   # (k, totalHitsThreshold); k = 1000 over the dense terms also overflows the buffer


def bq(terms):
    cl = [api.TermQuery(0, int(t)) for t in terms]
    return cl[0] if len(cl) == 1 else api.BooleanQuery(tuple(cl))


def check(name, got, exp, k, thr):
    edocs, escores, etotal, egte = exp
    assert got.docs.tolist() == edocs.tolist(), f"{name}: docids/ranks differ"
    assert got.scores.view(np.uint32).tolist() == escores.view(np.uint32).tolist(), f"{name}: score bits differ"
    assert got.relation_gte == egte, f"{name}: relation"
    if egte:
        assert max(thr, k) < got.total_hits <= etotal, f"{name}: lower bound {got.total_hits} not in ({max(thr, k)}, {etotal}]"
    else:
        assert got.total_hits == etotal, f"{name}: totalHits {got.total_hits} != {etotal}"


@pytest.fixture(scope="module", params=[1, 4], ids=["1_segment", "4_segments"])
def case(request, oracle):
    """(corpus, the oracle's answer per setting and query): computed once, shared, never changed."""
    corpus = synth.build_corpus(1_000_000, RANKS, n_segments=request.param)
    exp = {(k, thr, i): oracle.search_bm25(corpus, t, k, total_hits_threshold=thr) for k, thr in SETTINGS for i, t in enumerate(QUERIES)}
    return corpus, exp


def run_settings(ctx, corpus, exp, tag, settings=SETTINGS):
    leaves = [api.GpuSegment.from_data(ctx, s) for s in corpus.segments]
    try:
        sr = api.GpuIndexSearcher(ctx, leaves, api.IndexStatistics.from_corpus(corpus))
        ctx.set_speculation(5.0)
        ctx.reset_stats()
        for k, thr in settings:
            got = sr.search_batch([bq(t) for t in QUERIES], [api.TopScoreDocCollectorManager(k, None, thr)] * len(QUERIES))
            for i in range(len(QUERIES)):
                check(f"{tag}_{k}_{thr}_{i}", got[i], exp[(k, thr, i)], k, thr)
        c = ctx.spec_counters()
        assert c["queries"] == len(settings) * len(QUERIES) and not c["switched_off"], c
        assert c["reruns"] <= 1, c      # (five standard deviations, docs spread like a sample: a failed guess is a bug in the estimate)
        return ctx.maxscore_meetings()
    finally:
        for l in leaves:
            l.release()


def test_estimates_by_one_wave_leave_the_answers_alone(dev_lib, monkeypatch, case):
    """The product's instantiation of the kernel (no instrumentation), estimates due while every wave walks."""
    corpus, exp = case
    monkeypatch.setenv("NRTGPU_MS_SPEC_FIRST", "1")
    monkeypatch.setenv("NRTGPU_MS_SCATTER", "0")
    ctx = api.GpuContext(device_id=0, max_batch=64)
    try:
        run_settings(ctx, corpus, exp, "wave")
    finally:
        ctx.close()


def test_no_meeting_is_called_for_an_estimate(dev_lib, monkeypatch, case):
    """The instrumented instantiation: one wave made the estimates, and every meeting that took place was called by an overflow of
    the candidate buffer.  With NRTGPU_MS_SPEC_MEET=1 the estimates stop the workgroup as they used to: the same answers, and
    meetings that no overflow called.  (Their TOTAL need not differ on an index this small: a meeting called for an estimate also
    compacts a buffer that holds more than k keys, and the overflow it thereby prevents comes later instead -- measured here, one
    segment: 70 meetings either way, 25 of them overflows with the estimates in meetings, all 70 without.)"""
    corpus, exp = case
    monkeypatch.setenv("NRTGPU_MS_SPEC_FIRST", "1")
    monkeypatch.setenv("NRTGPU_MS_SCATTER", "0")
    ctx = api.GpuContext(device_id=0, max_batch=64, flags=_lib.NRTGPU_FLAG_PROFILE)
    try:
        wave = run_settings(ctx, corpus, exp, "wave_prof")
        print("estimates by one wave:", wave)
        assert wave["wave_estimates"] > 0, wave
        assert wave["meetings"] == wave["overflow_meetings"], wave
        monkeypatch.setenv("NRTGPU_MS_SPEC_MEET", "1")
        meet = run_settings(ctx, corpus, exp, "meeting_prof")
        print("estimates in meetings:", meet)
        assert meet["wave_estimates"] == 0, meet
        assert meet["meetings"] > meet["overflow_meetings"], meet   # (the estimates at windows 1 and 13: meetings nobody's overflow called)
    finally:
        ctx.close()
