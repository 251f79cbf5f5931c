"""The one-wave selection of the MaxScore walk's estimator (topk.hiph: topk_kth_wave) against numpy: the r-th largest of a set of
packed hit keys -- (score bits << 32) | ~docid -- held in LDS, found by ONE wave without a workgroup barrier.  Through the
development library's hook (include/nrtgpu_dev.h: nrtgpu_debug_wave_kth).  Needs a real MI355X."""
import numpy as np
import pytest

from nrtsearch_amd import api

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 1000, 2304)   # around the wave's width, a middling buffer, the walk's whole candidate buffer


def keys_of(kind: str, n: int, rng) -> np.ndarray:
    docs = rng.choice(1 << 24, size=n, replace=False).astype(np.uint64)
    if kind == "full":        # scores over the whole range of positive floats: wide buckets
        bits = rng.integers(1, 0x7F7FFFFF, size=n, dtype=np.uint64)
    elif kind == "unsigned":  # the sort routes' keys: order-preserving codes of a column over the whole unsigned range, top bit set too
        bits = rng.integers(0, 1 << 32, size=n, dtype=np.uint64)
        bits[:: 2] |= np.uint64(0x80000000)
        bits[0] = np.uint64(0xFFFFFFFF)
    elif kind == "equal":     # one score: every key in one bucket -- the byte radix once there are more than 64 of them
        bits = np.full(n, np.float32(7.25).view(np.uint32), dtype=np.uint64)
    else:                     # scores of one query: a narrow range, the one-histogram path
        bits = rng.uniform(10.0, 10.5, size=n).astype(np.float32).view(np.uint32).astype(np.uint64)
    keys = (bits << np.uint64(32)) | (~docs & np.uint64(0xFFFFFFFF))
    if kind == "third_zero":  # unwritten slots read 0 and rank below every key
        keys[::3] = 0
    return keys


@pytest.mark.parametrize("kind", ["narrow", "full", "unsigned", "equal", "third_zero"])
def test_one_wave_finds_the_rth_largest_key(dev_lib, kind):
    rng = np.random.Generator(np.random.PCG64(2024))
    for n in SIZES:
        keys = keys_of(kind, n, rng)
        ordered = np.sort(keys)
        for r in sorted({1, max(1, n // 2), n}):
            exp = int(np.partition(keys, n - r)[n - r])
            assert exp == int(ordered[n - r])
            got = api.debug_wave_kth(keys, r)
            assert got == exp, f"{kind}: n = {n}, r = {r}: {got:#x}, the r-th largest is {exp:#x}"
