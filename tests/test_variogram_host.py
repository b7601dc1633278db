"""not gpu: the host side of mcmc_gpu_amd.variogram -- the library's new entry point, the binning of an offset map (the
(lo, hi] convention and the direction filter) on a hand-made map, the model fit on noise-free model values, the argument errors,
and the NumPy checker of tests/variogram_common.py against itself (all pairs by coordinates vs. its own offset map)."""
import subprocess

import numpy as np
import pytest

import variogram_common as vc


def test_library_declares_and_exports_gsm_variogram_map():
    import mcmc_gpu_amd
    from mcmc_gpu_amd import _lib, variogram
    for name in ("variogram_kernel.hip", "gsm_api_variogram.hip"):
        assert name in _lib.SOURCES and (_lib.CSRC / name).exists()
    assert "gsm_variogram_map" in _lib.declared_symbols()
    lib = _lib.load()
    assert hasattr(lib, "gsm_variogram_map") and len(lib.gsm_variogram_map.argtypes) == 10
    out = subprocess.run(["strings", "-n", "6", str(_lib.LIB_PATH)], capture_output=True, text=True).stdout
    assert "variogram_map_kernel" in out and "variogram_combine_kernel" in out              # the kernels are in the gfx950 code object
    assert "variogram" in mcmc_gpu_amd.__all__
    assert {"variogram_map", "experimental", "fit", "variograms"} <= set(variogram.__all__)


def _hand_map(dx=100.0, dy=-50.0, mi=4, mj=3):
    """One field's map with sum = 2 * count * (1 + index): gamma of an offset alone is 1 + its flat index."""
    from mcmc_gpu_amd import variogram
    n = (mi + 1) * (2 * mj + 1)
    count = np.arange(1, n + 1, dtype=np.int64).reshape(1, mi + 1, 2 * mj + 1)
    count[0, 0, :mj + 1] = 0
    s = 2.0 * count * (1.0 + np.arange(n).reshape(count.shape))
    return variogram._result(mi, mj, dx, dy, s, count)


def test_bins_are_left_open_right_closed():
    from mcmc_gpu_amd import variogram
    vm = _hand_map()
    # offsets at exactly 100 (dj = 1; di = 2), 200 (dj = 2; di = 4) and 300 (dj = 3): an edge takes the offsets ON it
    gamma, counts = variogram.bin_map(vm, np.array([100.0, 200.0, 300.0]))
    d, c, s = vm.dist[None], vm.count, vm.sum
    for k, (lo, hi) in enumerate([(0.0, 100.0), (100.0, 200.0), (200.0, 300.0)]):
        sel = (d > lo) & (d <= hi)
        assert counts[0, k] == c[sel].sum() and gamma[0, k] == s[sel].sum() / (2.0 * c[sel].sum())
    on_first_edge = int(vm.count[0, 0, 3 + 1] + vm.count[0, 2, 3])
    g2, c2 = variogram.bin_map(vm, np.array([99.999, 200.0]))
    assert counts[0, 0] - c2[0, 0] == on_first_edge and c2[0, 1] - counts[0, 1] == on_first_edge
    # offsets beyond the last edge are dropped, an empty bin is NaN / 0, the zero offset is in no bin
    g3, c3 = variogram.bin_map(vm, np.array([10.0, 50.0]))
    assert c3[0, 0] == 0 and np.isnan(g3[0, 0]) and c3[0, 1] == vm.count[0, 1, 3]
    np.testing.assert_array_equal(variogram.bin_edges("even", 700.0, 7), 100.0 * np.arange(1, 8))
    np.testing.assert_array_equal(variogram.bin_edges([50.0, 120.0], 1.0, 99), [50.0, 120.0])
    with pytest.raises(ValueError):
        variogram.bin_edges([120.0, 50.0], 1.0, 2)


def test_direction_filter_is_modulo_180():
    from mcmc_gpu_amd import variogram
    vm = _hand_map()
    edges = np.array([1e4])
    along_x = vm.di == 0                                       # hy = 0
    along_y = vm.dj == 0                                       # hx = 0
    _, c0 = variogram.bin_map(vm, edges, azimuth=0.0, tolerance=1.0)
    _, c90 = variogram.bin_map(vm, edges, azimuth=90.0, tolerance=1.0)
    _, c270 = variogram.bin_map(vm, edges, azimuth=-90.0, tolerance=1.0)
    _, c180 = variogram.bin_map(vm, edges, azimuth=180.0, tolerance=1.0)
    assert c0[0, 0] == vm.count[0][along_x].sum() == c180[0, 0]
    assert c90[0, 0] == vm.count[0][along_y].sum() == c270[0, 0]
    # dy < 0: offset (di, dj) = (2, -1) is the vector (-100, -100), direction 45 degrees modulo 180; (2, 1) is 135
    _, c45 = variogram.bin_map(vm, edges, azimuth=45.0, tolerance=1.0)
    assert c45[0, 0] == vm.count[0, 2, 3 - 1] + vm.count[0, 4, 3 - 2]
    _, call = variogram.bin_map(vm, edges, azimuth=17.0, tolerance=90.0)
    assert call[0, 0] == vm.count.sum()


@pytest.mark.parametrize("vtype,s", [("exponential", None), ("gaussian", None), ("spherical", None), ("matern", 1.5)])
def test_fit_recovers_range_and_sill_from_model_values(vtype, s):
    pytest.importorskip("scipy.optimize")
    from mcmc_gpu_amd import variogram
    from mcmc_gpu_amd.sgs import cov_norm
    h = np.linspace(500.0, 30e3, 40)
    rng, sill, nugget = 9000.0, (1.0 if vtype == "spherical" else 1.3), (0.0 if vtype == "spherical" else 0.1)
    hn = h / rng
    gamma = nugget + (sill - nugget) - cov_norm(hn, vtype, sill, nugget, s)                   # the kriging kernels' model
    out = variogram.fit(h, gamma, np.arange(10, 10 + h.size), vtype, nugget=nugget, s=s)
    assert abs(out["major_range"] - rng) <= 1e-6 * rng and abs(out["sill"] - sill) <= 1e-6 * sill
    assert out["minor_range"] == out["major_range"] and out["azimuth"] == 0.0 and out["nugget"] == nugget and out["vtype"] == vtype
    assert ("s" in out) == (vtype == "matern") and (vtype != "matern" or out["s"] == s)
    from mcmc_gpu_amd import interpolate
    xx, yy = vc.grid_of(4, 4, 500.0, 500.0)
    interpolate._sanity_checks(xx, yy, np.zeros((4, 4)), out, 1e3, 16, "ok", None)           # a dict interpolate.sgs accepts
    # empty bins are left out
    g2, c2 = np.append(gamma, np.nan), np.append(np.arange(10, 10 + h.size), 0)
    out2 = variogram.fit(np.append(h, 31e3), g2, c2, vtype, nugget=nugget, s=s)
    assert out2 == out


def test_argument_errors():
    from mcmc_gpu_amd import variogram
    xx, yy, f, maxlag, n_lags = vc.case("base")
    bent = xx.copy()
    bent[:, 3] += 1.0
    with pytest.raises(NotImplementedError, match="uniform grid spacing"):
        variogram.variogram_map(bent, yy, f, maxlag)
    with pytest.raises(NotImplementedError, match="axis-aligned"):
        variogram.experimental(xx + 0.1 * yy, yy, f, maxlag=maxlag, n_lags=n_lags)
    with pytest.raises(ValueError, match="fields must be"):
        variogram.variogram_map(xx, yy, f[:, :, :-1], maxlag)
    with pytest.raises(ValueError, match="mask must have"):
        variogram.variogram_map(xx, yy, f, maxlag, mask=np.ones((3, 3), bool))
    with pytest.raises(ValueError, match="same shape"):
        variogram.variograms(xx, yy, f[0][:-1])
    with pytest.raises(NotImplementedError, match="downsample"):
        variogram.variograms(xx, yy, f[0], downsample=10)
    with pytest.raises(NotImplementedError, match="bin_func"):
        variogram.experimental(xx, yy, f, bin_func="uniform")
    with pytest.raises(ValueError, match="at least 3 rows and 3 columns"):
        variogram.variogram_map(xx[:, :1], yy[:, :1], f[:, :, :1], maxlag)
    pytest.importorskip("scipy.optimize")
    with pytest.raises(ValueError, match="vtype"):
        variogram.fit([1.0, 2.0], [0.5, 0.6], [3, 3], "cubic")


@pytest.mark.parametrize("tag", list(vc.CASES))
def test_checker_all_pairs_equals_binning_of_its_offset_map(tag):
    """The two formulations on the CPU: binning the checker's offset map with the product's bin_map gives the all-pairs counts
    exactly and its gamma within the derived bound.  Pins bin_map, offset_extents and the edge margin of every GPU case."""
    from mcmc_gpu_amd import variogram
    xx, yy, f, maxlag, n_lags = vc.case(tag)
    edges = vc.edges_of(maxlag, n_lags)
    vc.assert_edge_margin(xx, yy, maxlag, edges)
    H, W, dx, dy = vc.CASES[tag][:4]
    gamma, counts, s, c = vc.reference(tag)
    mi, mj = variogram.offset_extents(H, W, dx, dy, maxlag)
    assert (mi, mj) == (min(H - 1, int(maxlag // abs(dy))), min(W - 1, int(maxlag // abs(dx))))
    g, n = variogram.bin_map(variogram._result(mi, mj, dx, dy, s, c), edges)
    np.testing.assert_array_equal(n, counts)
    vc.assert_within_bound(g, gamma, n)
