"""not gpu: the host side of the local variogram maps -- the library's entry point, the Python argument errors, the NumPy checker
of tests/variogram_local_common.py against the all-pairs checker of tests/variogram_common.py, fit_anisotropic on exact tables,
fit_local's fall-back and expansion on hand-made lattices, the estimator on the two-regime field, and the bar that the device's
end-to-end test is held to (measured here on the checker alone)."""
import subprocess

import numpy as np
import pytest

import variogram_common as vc
import variogram_local_common as vl


def test_library_declares_and_exports_gsm_variogram_local():
    from mcmc_gpu_amd import _lib, variogram
    assert "variogram_local_kernel.hip" in _lib.SOURCES and (_lib.CSRC / "variogram_local_kernel.hip").exists()
    assert "gsm_variogram_local" in _lib.declared_symbols()
    lib = _lib.load()
    assert hasattr(lib, "gsm_variogram_local") and len(lib.gsm_variogram_local.argtypes) == 11
    out = subprocess.run(["strings", "-n", "6", str(_lib.LIB_PATH)], capture_output=True, text=True).stdout
    assert "variogram_tile_kernel" in out and "variogram_window_kernel" in out               # the kernels are in the gfx950 code object
    assert {"LocalVariogramMap", "local_variogram_map", "fit_anisotropic", "fit_local", "local_variograms"} <= set(variogram.__all__)


def test_argument_errors():
    from mcmc_gpu_amd import variogram
    xx, yy, f, maxlag, _ = vc.case("base")
    with pytest.raises(ValueError, match="tile must be"):
        variogram.local_variogram_map(xx, yy, f, maxlag, 1)
    with pytest.raises(ValueError, match="tile must be"):
        variogram.local_variogram_map(xx, yy, f, maxlag, 4.5)
    with pytest.raises(ValueError, match="half_window must be"):
        variogram.local_variogram_map(xx, yy, f, maxlag, 4, half_window=-1)
    with pytest.raises(ValueError, match="fields must be"):
        variogram.local_variogram_map(xx, yy, f[:, :, :-1], maxlag, 4)
    with pytest.raises(ValueError, match="mask must have"):
        variogram.local_variogram_map(xx, yy, f, maxlag, 4, mask=np.ones((3, 3), bool))
    with pytest.raises(NotImplementedError, match="axis-aligned"):
        variogram.local_variogram_map(xx + 0.1 * yy, yy, f, maxlag, 4)
    with pytest.raises(ValueError, match="maxlag must be positive"):
        variogram.local_variogram_map(xx, yy, f, 0.0, 4)
    with pytest.raises(ValueError, match="same shape"):
        variogram.local_variograms(xx, yy, f[0][:-1], "exponential", maxlag, 4)
    with pytest.raises(TypeError, match="field"):
        variogram.local_variograms(xx, yy, f[0], "exponential", maxlag, 4, field=1)
    h = np.arange(12.0).reshape(3, 4)
    with pytest.raises(ValueError, match="vtype"):
        variogram.fit_anisotropic(h, h, h, h, "cubic")
    with pytest.raises(ValueError, match="pass s"):
        variogram.fit_anisotropic(h, h, h, h, "matern")
    with pytest.raises(ValueError, match="same shape"):
        variogram.fit_anisotropic(h, h, h[:2], h, "gaussian")
    with pytest.raises(ValueError, match="too few"):
        variogram.fit_anisotropic(h, 2.0 * h, h, h, "gaussian")                              # every offset in one direction
    xx2, yy2, _ = vl.two_regime()
    S, C = np.ones((2, 2, 3, 5)), np.ones((2, 2, 3, 5), dtype=np.int64)
    lm = vl.local_map(xx2[:8, :8], yy2[:8, :8], 4, 0, (2, 2), S, C)
    with pytest.raises(ValueError, match="expand"):
        variogram.fit_local(lm, "exponential", expand="cubic")
    with pytest.raises(ValueError, match="field must be"):
        variogram.fit_local(lm, "exponential", field=1)


@pytest.mark.parametrize("tag", ["ragged", "odd", "tile2", "lines"])
def test_checker_tiles_add_up_to_the_all_pairs_offset_map(tag):
    """The midpoint rule puts every pair into exactly one tile: the checker's tile tables, summed over the tiles, give the counts
    of variogram_common.offset_map (all pairs, no offsets, no tiles) exactly and its sums within the bound."""
    _, _, T, _, mi, mj, _ = vl.CASES[tag]
    f, mask = vl.case(tag)
    S, C = vl.tiles_of(tag)
    for r in range(2):
        s, c = vc.offset_map(f[r], mi, mj, mask)
        np.testing.assert_array_equal(C[r].sum(axis=(0, 1)), c)
        vc.assert_within_bound(S[r].sum(axis=(0, 1)), s, c)
    assert tag != "lines" or (C == 0).mean() > 0.1                                          # 'lines' has empty (tile, offset) entries


def test_checker_one_tile_is_the_offset_map():
    _, _, T, _, mi, mj, R = vl.CASES["one"]
    f, _ = vl.case("one")
    S, C = vl.tiles_of("one")
    assert S.shape == (R, 1, 1, mi + 1, 2 * mj + 1)
    for r in range(R):
        s, c = vc.offset_map(f[r], mi, mj)
        np.testing.assert_array_equal(C[r, 0, 0], c)
        vc.assert_within_bound(S[r, 0, 0], s, c)


def test_checker_windows_are_clipped_sums_of_tiles():
    S, C = vl.tiles_of("odd")
    WS, WC = vl.reference("odd", 2)
    Ty, Tx = C.shape[1:3]
    assert (Ty, Tx) == (5, 4)
    np.testing.assert_array_equal(WC[0, 2, 1], C[0, 0:5, 0:4].sum(axis=(0, 1)))             # every tile: clipped on all four sides
    np.testing.assert_array_equal(WC[0, 0, 0], C[0, 0:3, 0:3].sum(axis=(0, 1)))
    np.testing.assert_array_equal(WC[1, 4, 3], C[1, 2:5, 1:4].sum(axis=(0, 1)))
    vc.assert_within_bound(WS[1, 4, 3], S[1, 2:5, 1:4].sum(axis=(0, 1)), WC[1, 4, 3])


def _offset_table(mi=20, mj=20, dx=500.0, dy=-500.0):
    di, dj = np.meshgrid(np.arange(mi + 1), np.arange(-mj, mj + 1), indexing="ij")
    counts = ((60 - di) * (60 - np.abs(dj))).astype(np.float64)
    counts[0, :mj + 1] = 0                                                                   # the empty half row of a variogram map
    return dj * dx, di * dy, counts


def _exact_gamma(hx, hy, counts, vtype, major, minor, az, sill, nugget, s):
    from mcmc_gpu_amd import sgs, variogram
    R = sgs.rotation_matrix({"azimuth": az, "major_range": major, "minor_range": minor})
    u, v = hx * R[0, 0] + hy * R[1, 0], hx * R[0, 1] + hy * R[1, 1]                          # the lag times R from the left
    return np.where(counts > 0, variogram.model_gamma(np.hypot(u, v), vtype, 1.0, sill, nugget, s), np.nan)


@pytest.mark.parametrize("vtype,s", [("exponential", None), ("gaussian", None), ("spherical", None), ("matern", 1.5)])
@pytest.mark.parametrize("major,minor,az,sill,nugget", [(7000.0, 4000.0, 35.0, 1.0, 0.0), (9000.0, 3000.0, 130.0, 1.0, 0.05),
                                                         (5000.0, 4500.0, 95.0, 0.8, 0.02)])
def test_fit_anisotropic_recovers_exact_tables(vtype, s, major, minor, az, sill, nugget):
    """21 x 41 offsets at 500 m, the exact model values (the kriging kernels' own model): 1e-8 relative on ranges and sill,
    1e-8 x 180 degrees on the azimuth."""
    from mcmc_gpu_amd import interpolate, variogram
    hx, hy, counts = _offset_table()
    out = variogram.fit_anisotropic(hx, hy, _exact_gamma(hx, hy, counts, vtype, major, minor, az, sill, nugget, s), counts, vtype, nugget=nugget, s=s)
    err = {"major_range": abs(out["major_range"] / major - 1), "minor_range": abs(out["minor_range"] / minor - 1),
           "sill": abs(out["sill"] / sill - 1), "azimuth": abs(out["azimuth"] - az) / 180.0}
    print(vtype, err)
    assert max(err.values()) <= 1e-8, err
    assert out["major_range"] >= out["minor_range"] and 0.0 <= out["azimuth"] < 180.0
    assert out["nugget"] == nugget and out["vtype"] == vtype and (("s" in out) == (vtype == "matern"))
    xx, yy = vc.grid_of(4, 4, 500.0, 500.0)
    interpolate._sanity_checks(xx, yy, np.zeros((4, 4)), out, 1e3, 16, "ok", None)           # a dict interpolate.sgs accepts


@pytest.mark.parametrize("vtype,s", [("exponential", None), ("gaussian", None), ("spherical", None), ("matern", 1.5)])
def test_fit_anisotropic_isotropic_table_has_azimuth_zero(vtype, s):
    from mcmc_gpu_amd import variogram
    hx, hy, counts = _offset_table()
    out = variogram.fit_anisotropic(hx, hy, _exact_gamma(hx, hy, counts, vtype, 6250.0, 6250.0, 0.0, 1.0, 0.0, s), counts, vtype, s=s)
    assert out["azimuth"] == 0.0 and out["major_range"] == out["minor_range"]
    assert abs(out["major_range"] / 6250.0 - 1) <= 1e-8 and abs(out["sill"] - 1.0) <= 1e-8


def test_fit_anisotropic_serves_a_global_variogram_map():
    """The anisotropic counterpart of `fit`: a VariogramMap's own arrays go in as they are."""
    from mcmc_gpu_amd import variogram
    hx, hy, counts = _offset_table(8, 12, 400.0, 650.0)
    g = _exact_gamma(hx, hy, counts, "exponential", 6000.0, 2500.0, 160.0, 1.2, 0.1, None)
    c = counts.astype(np.int64)
    vm = variogram._result(8, 12, 400.0, 650.0, (2.0 * g * c)[None], c[None])
    out = variogram.fit_anisotropic(vm.hx, vm.hy, vm.gamma[0], vm.count[0], "exponential", nugget=0.1)
    assert abs(out["major_range"] / 6000.0 - 1) <= 1e-8 and abs(out["minor_range"] / 2500.0 - 1) <= 1e-8
    assert abs(out["azimuth"] - 160.0) <= 1e-8 * 180.0 and abs(out["sill"] / 1.2 - 1) <= 1e-8


def _lattice_map(params, T=4, H=12, W=12, few=()):
    """A 3 x 3 lattice of exact exponential window tables (params[a][b] = (major, minor, azimuth)); windows in `few` hold 10 pairs."""
    hx, hy, counts = _offset_table(6, 6, 500.0, 500.0)
    S, C = np.zeros((3, 3) + hx.shape), np.zeros((3, 3) + hx.shape, dtype=np.int64)
    for a in range(3):
        for b in range(3):
            g = _exact_gamma(hx, hy, counts, "exponential", *params[a][b], 1.0, 0.0, None)
            c = counts.astype(np.int64)
            if (a, b) in few:
                c = np.zeros_like(c)
                c[[1, 2, 3, 4, 5], [7, 8, 9, 10, 11]] = 2                                    # five offsets, all in one direction
            S[a, b], C[a, b] = np.where(c > 0, 2.0 * g * c, 0.0), c
    xx, yy = vc.grid_of(H, W, 500.0, 500.0)
    whole_g = _exact_gamma(hx, hy, counts, "exponential", 8000.0, 8000.0, 0.0, 1.0, 0.0, None)
    whole_c = counts.astype(np.int64) * 9
    return vl.local_map(xx, yy, T, 0, (6, 6), S, C, (np.where(whole_c > 0, 2.0 * whole_g * whole_c, 0.0), whole_c))


def test_fit_local_falls_back_to_the_whole_field_and_expands_nearest():
    from mcmc_gpu_amd import interpolate, variogram
    params = [[(6000.0 + 500.0 * (3 * a + b), 3000.0, 10.0 + 20.0 * (3 * a + b)) for b in range(3)] for a in range(3)]
    lm = _lattice_map(params, few=[(0, 1), (2, 2)])
    out = variogram.fit_local(lm, "exponential", min_pairs=500)
    expect = np.ones((3, 3), dtype=bool)
    expect[0, 1] = expect[2, 2] = False
    np.testing.assert_array_equal(out.fitted, expect)
    assert set(out) == {"major_range", "minor_range", "azimuth", "sill", "nugget", "vtype"}
    for key in ("major_range", "minor_range", "azimuth", "sill"):
        assert out[key].shape == (12, 12) and np.isfinite(out[key]).all()
    for a in range(3):
        for b in range(3):
            block = (slice(4 * a, 4 * a + 4), slice(4 * b, 4 * b + 4))
            major, minor, az = params[a][b] if expect[a, b] else (8000.0, 8000.0, 0.0)      # the whole field's table is isotropic
            np.testing.assert_allclose(out["major_range"][block], major, rtol=1e-8)
            np.testing.assert_allclose(out["minor_range"][block], minor, rtol=1e-8)
            np.testing.assert_allclose(out["azimuth"][block], az, rtol=0, atol=1e-8 * 180.0)
            assert np.all(out["major_range"][block] == out["major_range"][block][0, 0])     # nearest: constant per tile
    assert np.all(out["azimuth"][0:4, 4:8] == 0.0)
    # a window with enough pairs whose offsets lie in one direction: the fit fails, and it falls back too
    out2 = variogram.fit_local(lm, "exponential", min_pairs=5)
    np.testing.assert_array_equal(out2.fitted, expect)
    xx, yy = vc.grid_of(12, 12, 500.0, 500.0)
    interpolate._sanity_checks(xx, yy, np.zeros((12, 12)), out, 1e3, 16, "ok", np.ones((12, 12), dtype=bool))
    assert interpolate._local_table(out, (12, 12)).shape == (144, 6)


def test_fit_local_bilinear_interpolates_between_tile_centres_and_the_azimuth_through_zero():
    from mcmc_gpu_amd import variogram
    params = [[(6000.0 + 1000.0 * b + 300.0 * a, 3000.0, (170.0, 10.0, 30.0)[b]) for b in range(3)] for a in range(3)]
    lm = _lattice_map(params, H=12, W=11)                    # the last tile column is ragged: 3 cells, centre at column 9
    out = variogram.fit_local(lm, "exponential", expand="bilinear")
    assert out.fitted.all() and out["major_range"].shape == (12, 11)
    cj, ci = np.array([1.5, 5.5, 9.0]), np.array([1.5, 5.5, 9.5])
    P = np.array([[p[0] for p in row] for row in params])
    expect = np.stack([np.interp(np.arange(11), cj, row) for row in P])
    expect = np.stack([np.interp(np.arange(12), ci, expect[:, j]) for j in range(11)], axis=1)
    np.testing.assert_allclose(out["major_range"], expect, rtol=1e-8)
    assert np.all(out["major_range"][:2, 0] == out["major_range"][0, 0]) and np.all(out["major_range"][10:, 10] == out["major_range"][11, 10])
    np.testing.assert_allclose(out["minor_range"], 3000.0, rtol=1e-8)
    az = out["azimuth"][0]
    assert np.all((az >= 0.0) & (az < 180.0))
    np.testing.assert_allclose(az[:2], 170.0, atol=1e-6)                                     # constant outside the outermost centres
    between = az[2:6]                                                                        # columns 2 .. 5 lie between 170 and 10 degrees
    folded = (between + 90.0) % 180.0 - 90.0                                                 # to (-90, 90]
    assert np.all(np.abs(folded) <= 10.0 + 1e-6), between                                    # through 0, not through 90
    assert np.all(np.diff(folded) > 0)
    assert folded[1] < 0.0 < folded[2] and abs(folded[1] + folded[2]) < 1e-6                 # columns 3 and 4 mirror each other about 0
    np.testing.assert_allclose(az[9:], 30.0, atol=1e-6)


def _inside(half):
    """The windows (k = 1) wholly inside a half: tile columns 0 .. 2 on the left, 5 .. 7 on the right (64 columns = 4 tiles each)."""
    return (slice(None), slice(0, 3)) if half == 0 else (slice(None), slice(5, 8))


def test_two_regime_field_estimator_finds_both_regimes():
    """Conditions on the estimator, on the checker's tables, before the device sees the field: per half the median azimuth of the
    windows wholly inside lies within 15 degrees of the regime's, and the median major / minor exceeds 2."""
    fit = vl.two_regime_fit()
    assert fit.fitted.all() and fit.fitted.shape == (8, 8)
    az = np.array([[w["azimuth"] for w in row] for row in fit.windows])
    ratio = np.array([[w["major_range"] / w["minor_range"] for w in row] for row in fit.windows])
    for half, want in enumerate(vl.TWO["az"]):
        got, r = float(np.median(az[_inside(half)])), float(np.median(ratio[_inside(half)]))
        print("half", half, "median azimuth", got, "median major / minor", r)
        assert abs((got - want + 90.0) % 180.0 - 90.0) <= 15.0
        assert r > 2.0
    for key in ("major_range", "minor_range", "azimuth", "sill"):
        assert fit[key].shape == (128, 128) and np.isfinite(fit[key]).all()


def test_fairness_bar_of_the_end_to_end_test():
    """The bar is measured against the checker, never against the device; at most 5 % of the fitted windows may drop out of the
    azimuth comparison, and the bar stays far below anything a wrong table could hide behind."""
    bar, keep = vl.fairness_bar()
    fitted = vl.two_regime_fit().fitted
    assert (~keep & fitted).sum() <= 0.05 * fitted.sum()
    assert all(0.0 <= b < 1e-8 for b in bar.values()), bar
