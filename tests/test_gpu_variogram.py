"""GPU: mcmc_gpu_amd.variogram (gsm_variogram_map, csrc/variogram_kernel.hip) against the all-pairs NumPy checker of
tests/variogram_common.py, which takes every pair's separation from the cells' coordinates and knows nothing of offsets.

Tolerance (derived, not tuned): every term of a sum is non-negative, so any summation order of n terms with three roundings each
(difference, square, addition) satisfies |dev - exact| <= (n + 3) 2^-53 exact; asserted exactly so, with n the count the device
returned.  Counts are asserted equal.

Cases (variogram_common.CASES), values N(300, 50) with 30 % of the cells NaN, drawn independently per field:
    base  24 x 20,  500 x  500 m, maxlag  4300, 7 lags, 3 fields   baseline
    wide  17 x 70,  500 x -500 m, maxlag  6100, 9 lags, 3 fields   W no multiple of the wavefront, descending y
    rect  21 x 19,  400 x -650 m, maxlag  5100, 8 lags, 3 fields   non-square cells, mi != mj
    far    9 x 13,  500 x  500 m, maxlag 20000, 6 lags, 3 fields   maxlag beyond the grid: empty far bins, gamma NaN there
    cols  12 x 150, 500 x  500 m, maxlag  3300, 5 lags, 2 fields   many columns (two column tiles), few offsets
The five above have at most 25 column offsets: one workgroup per block of row offsets.  A workgroup owns 64 column offsets, so:
    tiles 12 x 150, 500 x  500 m, maxlag 35200, 7 lags, 2 fields   mj = 70: 141 column offsets in three tiles, the last with 13 of
                                                                   its 64 lanes in use; mi = 11: three blocks of row offsets
    shift  4 x 260, 500 x  500 m, maxlag 104900, 7 lags, 2 fields  mj = 209: seven tiles; the leftmost tiles have no partner for the
                                                                   first columns and start at the second and third column tile;
                                                                   three column tiles of 128 with a ragged last one
Each case first asserts on the CPU that no offset distance lies within 1e-6 maxlag of a bin edge."""
import ctypes as C

import numpy as np
import pytest

import variogram_common as vc

pytestmark = pytest.mark.gpu
TAGS = list(vc.CASES)


def _case(tag):
    xx, yy, f, maxlag, n_lags = vc.case(tag)
    vc.assert_edge_margin(xx, yy, maxlag, vc.edges_of(maxlag, n_lags))
    return xx, yy, f, maxlag, n_lags


@pytest.mark.parametrize("tag", TAGS)
def test_variogram_map_equals_brute_force_offset_map(tag):
    from mcmc_gpu_amd import variogram
    xx, yy, f, maxlag, _ = _case(tag)
    _, _, ref_sum, ref_count = vc.reference(tag)
    vm = variogram.variogram_map(xx, yy, f, maxlag)
    H, W, dx, dy = vc.CASES[tag][:4]
    mi, mj = variogram.offset_extents(H, W, dx, dy, maxlag)
    assert (mi, mj) == {"tiles": (11, 70), "shift": (3, 209)}.get(tag, (mi, mj))
    assert vm.sum.shape == vm.count.shape == (f.shape[0], mi + 1, 2 * mj + 1) and vm.count.dtype == np.int64
    np.testing.assert_array_equal(vm.count, ref_count)
    vc.assert_within_bound(vm.sum, ref_sum, vm.count)
    assert np.all(vm.sum[:, 0, :mj + 1] == 0.0) and np.all(vm.count[:, 0, :mj + 1] == 0)      # (0, dj <= 0) is defined as zero
    np.testing.assert_array_equal(vm.di[:, 0], np.arange(mi + 1))
    np.testing.assert_array_equal(vm.dj[0], np.arange(-mj, mj + 1))
    np.testing.assert_array_equal(vm.dist, np.hypot(vm.dj * dx, vm.di * dy))
    with np.errstate(invalid="ignore", divide="ignore"):
        np.testing.assert_array_equal(vm.gamma, np.where(vm.count > 0, vm.sum / (2.0 * vm.count), np.nan))


@pytest.mark.parametrize("tag", TAGS)
def test_experimental_isotropic_equals_all_pairs(tag):
    from mcmc_gpu_amd import variogram
    xx, yy, f, maxlag, n_lags = _case(tag)
    ref_gamma, ref_counts, _, _ = vc.reference(tag)
    bins, gamma, counts = variogram.experimental(xx, yy, f, maxlag=maxlag, n_lags=n_lags)
    np.testing.assert_array_equal(bins, vc.edges_of(maxlag, n_lags))
    np.testing.assert_array_equal(counts, ref_counts)
    vc.assert_within_bound(gamma, ref_gamma, counts)
    if tag == "far":
        assert np.all(counts[:, -3:] == 0) and np.isnan(gamma[:, -3:]).all() and np.isfinite(gamma[:, 0]).all()


@pytest.mark.parametrize("azimuth", [0.0, 90.0])
def test_experimental_directional(azimuth):
    from mcmc_gpu_amd import variogram
    xx, yy, f, maxlag, n_lags = _case("rect")
    edges = vc.edges_of(maxlag, n_lags)
    _, gamma, counts = variogram.experimental(xx, yy, f, maxlag=maxlag, n_lags=n_lags, azimuth=azimuth, tolerance=22.5)
    iso = vc.reference("rect")[1]
    for r in range(f.shape[0]):
        g, c = vc.experimental(xx, yy, f[r], edges, azimuth=azimuth, tolerance=22.5)
        np.testing.assert_array_equal(counts[r], c)
        vc.assert_within_bound(gamma[r], g, counts[r])
    assert 0 < counts.sum() < iso.sum()


def test_experimental_mask_excludes_a_rectangle():
    from mcmc_gpu_amd import variogram
    xx, yy, f, maxlag, n_lags = _case("base")
    mask = np.ones(xx.shape, dtype=bool)
    mask[5:14, 3:11] = False
    _, gamma, counts = variogram.experimental(xx, yy, f, maxlag=maxlag, n_lags=n_lags, mask=mask)
    for r in range(f.shape[0]):
        g, c = vc.experimental(xx, yy, f[r], vc.edges_of(maxlag, n_lags), mask=mask)
        np.testing.assert_array_equal(counts[r], c)
        vc.assert_within_bound(gamma[r], g, counts[r])
    assert counts.sum() < vc.reference("base")[1].sum()


def test_2d_input_equals_one_field_batch():
    from mcmc_gpu_amd import variogram
    xx, yy, f, maxlag, n_lags = _case("base")
    a = variogram.experimental(xx, yy, f[0], maxlag=maxlag, n_lags=n_lags)
    b = variogram.experimental(xx, yy, f[:1], maxlag=maxlag, n_lags=n_lags)
    assert a[1].shape == (1, n_lags)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_same_call_twice_and_batch_row_are_bit_identical():
    from mcmc_gpu_amd import variogram
    xx, yy, f, maxlag, _ = _case("wide")
    a, b = variogram.variogram_map(xx, yy, f, maxlag), variogram.variogram_map(xx, yy, f, maxlag)
    assert a.sum.tobytes() == b.sum.tobytes() and a.count.tobytes() == b.count.tobytes()
    for r in range(f.shape[0]):
        one = variogram.variogram_map(xx, yy, f[r], maxlag)
        assert one.sum[0].tobytes() == a.sum[r].tobytes() and one.count[0].tobytes() == a.count[r].tobytes()


@pytest.mark.parametrize("rows", [4, 7])
def test_forced_row_split_keeps_counts_and_bound(rows):
    """24 rows in parts of 4 (six parts) and of 7 (ragged last part): partials added in part order."""
    from mcmc_gpu_amd import variogram
    xx, yy, f, maxlag, _ = _case("base")
    _, _, ref_sum, ref_count = vc.reference("base")
    vm = variogram.variogram_map(xx, yy, f, maxlag, _rows_per_part=rows)
    np.testing.assert_array_equal(vm.count, ref_count)
    vc.assert_within_bound(vm.sum, ref_sum, vm.count)
    again = variogram.variogram_map(xx, yy, f, maxlag, _rows_per_part=rows)
    assert again.sum.tobytes() == vm.sum.tobytes()
    one = variogram.variogram_map(xx, yy, f[2], maxlag, _rows_per_part=rows)
    assert one.sum[0].tobytes() == vm.sum[2].tobytes()


def test_c_abi_argument_errors_and_offsets_beyond_the_grid():
    import torch
    from mcmc_gpu_amd.engine import GsmEngine, _ptr
    from mcmc_gpu_amd._lib import GsmError
    xx, yy, f, maxlag, _ = _case("base")
    R, H, W = f.shape
    eng = GsmEngine(H, W, 1)
    try:
        d_f = torch.as_tensor(np.ascontiguousarray(f)).to(eng.dev)
        mi, mj = H + 3, W + 3
        d_s = torch.full((R, mi + 1, 2 * mj + 1), -1.0, dtype=torch.float64, device=eng.dev)
        d_c = torch.full((R, mi + 1, 2 * mj + 1), -1, dtype=torch.int64, device=eng.dev)
        null = C.c_void_p(0)

        def call(fields=_ptr(d_f), n=R, a=mi, b=mj, rows=0, s=_ptr(d_s), c=_ptr(d_c)):
            return eng.lib.gsm_variogram_map(eng.h, fields, n, null, a, b, rows, s, c, eng._stream())

        for bad in (dict(fields=null), dict(s=null), dict(c=null), dict(n=0), dict(a=-1), dict(b=-1), dict(rows=-1)):
            assert call(**bad) == -1, bad                                                    # GSM_E_ARG
            assert "gsm_variogram_map" in eng.lib.gsm_last_error(eng.h).decode()
            with pytest.raises(GsmError, match="gsm_variogram_map"):
                eng._check(call(**bad))
        assert torch.all(d_s == -1.0) and torch.all(d_c == -1)                               # a refused call writes nothing
        eng._check(call())                                                                   # a valid call afterwards succeeds
        torch.cuda.synchronize()
        s, c = d_s.cpu().numpy(), d_c.cpu().numpy()
    finally:
        eng.close()
    ref = [vc.offset_map(z, H - 1, W - 1) for z in f]
    inside = (slice(None), slice(0, H), slice(mj - (W - 1), mj + W))
    np.testing.assert_array_equal(c[inside], np.array([k for _, k in ref]))
    vc.assert_within_bound(s[inside], np.array([k for k, _ in ref]), c[inside])
    beyond = np.ones(s.shape, dtype=bool)
    beyond[inside] = False
    assert np.all(s[beyond] == 0.0) and np.all(c[beyond] == 0)                               # zeros beyond the grid


def test_variograms_end_to_end_fit_equals_fit_of_checker_variogram():
    """A 64 x 64 realisation of a known exponential model (interpolate.sgs_many); variograms() on it.  The fitted ranges are
    compared with the fit of the same field's all-pairs CPU variogram at 1e-9 relative -- not with the true model, whose
    distance from one realisation's fit is sampling noise."""
    from mcmc_gpu_amd import interpolate, variogram
    n = 64
    xx, yy = vc.grid_of(n, n, 500.0, -500.0)
    rng = np.random.default_rng(5)
    grid = np.full((n, n), np.nan)
    at = rng.choice(n * n, 200, replace=False)
    grid.ravel()[at] = rng.normal(0.0, 1.0, at.size)
    true = {"major_range": 6000.0, "minor_range": 6000.0, "azimuth": 0.0, "sill": 1.0, "nugget": 0.0, "vtype": "exponential"}
    field = interpolate.sgs_many(xx, yy, grid, true, [11], radius=8000.0, num_points=16, quiet=True)[0]
    assert np.isfinite(field).all()
    maxlag, n_lags = 11100.0, 12
    edges = vc.edges_of(maxlag, n_lags)
    vc.assert_edge_margin(xx, yy, maxlag, edges)
    models = ["exponential", "gaussian", "spherical"]
    vgrams, gamma, bins = variogram.variograms(xx, yy, field, maxlag=maxlag, n_lags=n_lags, covmodels=models)
    np.testing.assert_array_equal(bins, edges)
    scores = variogram._normal_scores(field[None])[0]
    g, c = vc.experimental(xx, yy, scores, edges)
    vc.assert_within_bound(gamma, g, c)
    for m in models:
        ref = variogram.fit(edges, g, c, m)
        assert set(vgrams[m]) >= {"major_range", "minor_range", "azimuth", "sill", "nugget", "vtype"} and vgrams[m]["vtype"] == m
        print(m, vgrams[m]["major_range"], ref["major_range"], vgrams[m]["sill"], ref["sill"])
        assert abs(vgrams[m]["major_range"] - ref["major_range"]) <= 1e-9 * ref["major_range"]
        assert abs(vgrams[m]["sill"] - ref["sill"]) <= 1e-9 * ref["sill"]
    assert 0.0 < vgrams["exponential"]["major_range"] < 20 * maxlag
