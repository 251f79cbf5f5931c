"""The reference of tests/test_float_rescore_gpu.py checked on the host (tests/_float_rescore_ref.py): its derived interval must
HOLD for a float32 computation in the kernels' order -- a lane per 64th element, an xor butterfly; multiply and add rounded
separately, and fused -- and must be SHARP: three simulated mistakes of the kernels (a marker element left out, the last
element left out, rows read at the field's own dimension as stride instead of the resident one) land outside it.  Rows, queries
and weights are the GPU test's own generators and SHAPES; first-pass scores are drawn like BM25 scores of a few units."""
import numpy as np
import pytest

from tests import _float_rescore_ref as R

N_ROWS, N_QUERIES = 300, 3
f32 = np.float32


def _case(sim_name, dim):
    sim, kind = R.SIMS[sim_name], R.KIND_OF_SIM[sim_name]
    rng = np.random.default_rng([7, sim, dim])
    rows = R.make_rows(rng, N_ROWS, dim, kind)
    keep = rows.any(axis=1)               # (a zero row scores the same whatever is left out of the sum: not a hit a mistake can show on)
    queries = R.make_queries(rng, N_QUERIES, dim, kind)
    first = rng.uniform(0.1, 8.0, size=N_ROWS).astype(f32)
    return sim, rows, keep, queries, first


def _self_dot(rows, fused):
    """knn_row_norms_kernel: |v|^2 per row in the wave order."""
    res = R.resident(rows.shape[1])
    width = -(-res // 64) * 64
    vp = np.zeros((rows.shape[0], width), dtype=f32)
    vp[:, : rows.shape[1]] = rows
    acc = np.zeros((rows.shape[0], 64), dtype=f32)
    for k in range(0, width, 64):
        x = vp[:, k:k + 64]
        acc = (acc.astype(np.float64) + x.astype(np.float64) ** 2).astype(f32) if fused else acc + x * x
    lanes = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ d]
    return acc[:, 0]


def _ranges(sim, dim, q, rows, first):
    _, _, qw, rw, boost = R.SHAPES[dim]
    has = np.ones(len(rows), dtype=bool)
    return R.combined(qw, rw, first, has, R.second_pass(sim, q, rows, boost, dim))


def _simulated(sim, dim, q, rows, first, fused, nv, skip=None, as_rows=None):
    _, _, qw, rw, boost = R.SHAPES[dim]
    acc = R.wave_sum(sim, q, rows if as_rows is None else as_rows, fused, skip)
    return R.kernel_score(sim, acc, R.host_query_norm(q), nv, boost, qw, rw, first).astype(np.float64)


@pytest.mark.parametrize("dim", R.DIMS)
@pytest.mark.parametrize("sim_name", list(R.SIMS))
def test_the_interval_holds_for_the_kernels_order_in_float32(sim_name, dim):
    sim, rows, _, queries, first = _case(sim_name, dim)
    worst = 0.0
    for fused in (False, True):
        nv = _self_dot(rows, fused)
        for q in queries:
            ref, lo, hi = _ranges(sim, dim, q, rows, first)
            got = _simulated(sim, dim, q, rows, first, fused, nv)
            assert ((lo <= got) & (got <= hi)).all(), (sim_name, dim, fused, int(np.argmax((got < lo) | (got > hi))))
            worst = max(worst, float((np.abs(got - ref) / ((hi - lo) / 2)).max()))
    print(f"{sim_name} {dim}: simulated |got - ref| / half-width <= {worst:.3f}")


def _share_outside(sim, dim, queries, rows, keep, first, **mistake):
    outside = total = 0
    for fused in (False, True):
        nv = _self_dot(rows, fused)
        for q in queries:
            _, lo, hi = _ranges(sim, dim, q, rows, first)
            got = _simulated(sim, dim, q, rows, first, fused, nv, **mistake)
            outside += int((((got < lo) | (got > hi)) & keep).sum())
            total += int(keep.sum())
    return outside / total


@pytest.mark.parametrize("dim", R.DIMS)
@pytest.mark.parametrize("sim_name", list(R.SIMS))
def test_a_marker_or_the_last_element_left_out_lands_outside_the_interval(sim_name, dim):
    sim, rows, keep, queries, first = _case(sim_name, dim)
    for pos in R.marker_positions(dim):      # (dim - 1 is the last of them)
        share = _share_outside(sim, dim, queries, rows, keep, first, skip=pos)
        assert share >= 0.99, (sim_name, dim, pos, share)


@pytest.mark.parametrize("dim", [d for d in R.DIMS if R.resident(d) != d])
@pytest.mark.parametrize("sim_name", list(R.SIMS))
def test_rows_read_at_the_fields_own_stride_land_outside_the_interval(sim_name, dim):
    """Row r taken from element dim * r of the resident matrix (rows padded to a multiple of 16) instead of resident * r, over dim
    elements; its norm is the right row's.  Row 0 is read correctly either way and is left out of the count."""
    sim, rows, keep, queries, first = _case(sim_name, dim)
    res = R.resident(dim)
    flat = np.zeros((len(rows), res), dtype=f32)
    flat[:, :dim] = rows
    flat = flat.ravel()
    wrong = np.stack([flat[r * dim: r * dim + dim] for r in range(len(rows))])
    keep = keep.copy()
    keep[0] = False
    share = _share_outside(sim, dim, queries, rows, keep, first, as_rows=wrong)
    assert share >= 0.99, (sim_name, dim, share)


def test_the_cases_cover_what_they_must():
    windows = {d: s[1] for d, s in R.SHAPES.items()}
    assert sorted(R.SHAPES) == R.DIMS and [R.resident(d) for d in R.DIMS] == [16, 64, 112, 208, 272, 768, 2048]
    assert any(s[0] == 1024 for s in R.SHAPES.values()) and any(s[2] == 0.0 for s in R.SHAPES.values())
    assert sum(s[4] != 1.0 for s in R.SHAPES.values()) >= 2 and any(s[0] == s[1] for s in R.SHAPES.values())
    assert windows[100] > R.SHAPES[100][0]
    # the four-element step of knn_wave_partials (k + 192 < resident, k += 256): at 200 only lanes 0-15 take it; at 260 every lane
    # takes it once and lanes 0-15 a tail element behind it; it runs 3 and 8 times at 768 and 2048, never at 3, 64 and 100
    assert [lane for lane in range(64) if lane + 192 < R.resident(200)] == list(range(16))
    assert all(lane + 192 < R.resident(260) for lane in range(64)) and [lane for lane in range(64) if lane + 256 < R.resident(260)] == list(range(16))
    assert [len(range(0, R.resident(d) - 192, 256)) for d in (3, 64, 100, 768, 2048)] == [0, 0, 0, 3, 8]
