"""GPU: the local variogram maps (gsm_variogram_local, csrc/variogram_local_kernel.hip; variogram.local_variogram_map, fit_local,
local_variograms) against the NumPy checker of tests/variogram_local_common.py, which takes each pair's tile from the midpoint
rule, sums with math.fsum and knows nothing of lanes, parities or segments.

Tolerance (derived, not tuned): variogram_common.assert_within_bound, |dev - exact| <= (n + 3) 2^-53 exact with n the entry's own
count -- any summation order of n non-negative terms of three roundings each, so it covers the tile pass and the window pass
alike.  Counts are asserted equal, and an entry with count 0 is exactly 0.0.

Cases (variogram_local_common.CASES), values N(300, 50) with 30 % of the cells NaN unless stated, drawn independently per field:
    ragged 37 x 70,  T 8,  k 0 and 1, mi 9,  mj 40,  3 fields   ragged last tiles; 81 column offsets (more than one lane group,
                                                                both parities); mi + 1 no multiple of the row block
    odd    23 x 19,  T 5,  k 2,       mi 22, mj 18,  2 fields   odd tile size; half-cell midpoints; offsets out to the grid's
                                                                extent; windows clipped on every side
    one    24 x 20,  T 64, k 0,       mi 8,  mj 8,   3 fields   one tile >= the grid
    thin    4 x 260, T 16, k 1,       mi 3,  mj 100, 2 fields   H < T; 17 tile columns (five workgroups of four, the last with
                                                                one); long column offsets
    tile2  12 x 12,  T 2,  k 1,       mi 5,  mj 5,   2 fields   offsets longer than a tile: both ends of a pair outside its
                                                                midpoint tile
    lines  48 x 48,  T 16, k 0 and 1, mi 10, mj 10,  2 fields   values on every 6th row and three columns only, plus a mask:
                                                                empty (tile, offset) entries (k 0 shows them; the windows of
                                                                k 1 add them away)"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import variogram_common as vc
import variogram_local_common as vl

pytestmark = pytest.mark.gpu


def _device_tables(f, mask, mi, mj, T, k):
    """gsm_variogram_local through the C ABI on fields [R, H, W]: (sum, count) [R, Ty, Tx, mi + 1, 2 mj + 1]."""
    import torch
    from mcmc_gpu_amd.engine import GsmEngine, _ptr
    R, H, W = f.shape
    Ty, Tx = vl.lattice(H, W, T)
    eng = GsmEngine(H, W, 1)
    try:
        d_f = torch.as_tensor(np.ascontiguousarray(f)).to(eng.dev)
        d_m = None if mask is None else torch.as_tensor(np.ascontiguousarray(mask, dtype=np.uint8)).to(eng.dev)
        d_s = torch.full((R, Ty, Tx, mi + 1, 2 * mj + 1), -1.0, dtype=torch.float64, device=eng.dev)
        d_c = torch.full((R, Ty, Tx, mi + 1, 2 * mj + 1), -1, dtype=torch.int64, device=eng.dev)
        eng._check(eng.lib.gsm_variogram_local(eng.h, _ptr(d_f), R, _ptr(d_m), mi, mj, T, k, _ptr(d_s), _ptr(d_c), eng._stream()))
        torch.cuda.synchronize()
        return d_s.cpu().numpy(), d_c.cpu().numpy()
    finally:
        eng.close()


@functools.lru_cache(maxsize=None)
def _device(tag, k):
    _, _, T, _, mi, mj, _ = vl.CASES[tag]
    f, mask = vl.case(tag)
    return _device_tables(f, mask, mi, mj, T, k)


@pytest.mark.parametrize("tag,k", vl.RUNS)
def test_tables_equal_the_checker(tag, k):
    s, c = _device(tag, k)
    ref_s, ref_c = vl.reference(tag, k)
    assert s.shape == ref_s.shape and c.dtype == np.int64
    np.testing.assert_array_equal(c, ref_c)
    vc.assert_within_bound(s, ref_s, c)
    assert np.all(s[c == 0] == 0.0)
    mj = vl.CASES[tag][5]
    assert np.all(c[..., 0, :mj + 1] == 0)                                                   # (0, dj <= 0) is defined as zero
    assert (tag, k) != ("lines", 0) or (c == 0).mean() > 0.1                                 # empty (tile, offset) entries beyond (0, dj <= 0)


@pytest.mark.parametrize("tag", ["ragged", "one"])
def test_tiles_add_up_to_the_global_map(tag):
    """Against the shipped kernel: the k = 0 tables summed over the tiles give gsm_variogram_map's counts exactly and its sums
    within the bound of both sides; with one tile >= the grid the table itself does."""
    import torch
    from mcmc_gpu_amd.engine import GsmEngine, _ptr
    H, W, T, _, mi, mj, R = vl.CASES[tag]
    f, mask = vl.case(tag)
    s, c = _device(tag, 0)
    eng = GsmEngine(H, W, 1)
    try:
        d_f = torch.as_tensor(np.ascontiguousarray(f)).to(eng.dev)
        d_s = torch.empty((R, mi + 1, 2 * mj + 1), dtype=torch.float64, device=eng.dev)
        d_c = torch.empty((R, mi + 1, 2 * mj + 1), dtype=torch.int64, device=eng.dev)
        eng._check(eng.lib.gsm_variogram_map(eng.h, _ptr(d_f), R, C.c_void_p(0), mi, mj, 0, _ptr(d_s), _ptr(d_c), eng._stream()))
        torch.cuda.synchronize()
        gs, gc = d_s.cpu().numpy(), d_c.cpu().numpy()
    finally:
        eng.close()
    if tag == "one":
        assert s.shape[1:3] == (1, 1)
    flat = s.reshape(R, -1, (mi + 1) * (2 * mj + 1))
    ts = np.array([[math.fsum(col) for col in x.T] for x in flat]).reshape(gs.shape)          # the tiles' sums added exactly, rounded once
    np.testing.assert_array_equal(c.sum(axis=(1, 2)), gc)
    # the global map is within (n + 3) u of the exact sum; every tile's sum is within (n_t + 3) u of its own, n_t <= n, and the
    # exact sum of those is rounded once: within (n + 4) u.  Between the two sides: (2 n + 8) u, second-order terms included
    err, bound = np.abs(ts - gs), (2.0 * gc + 8.0) * vc.U * gs
    print("worst error / bound:", float(np.max(err / np.where(bound > 0, bound, 1.0))))
    assert np.all(err <= bound)


def test_same_call_twice_batch_row_and_mask_are_bit_identical():
    _, _, T, _, mi, mj, R = vl.CASES["ragged"]
    f, _ = vl.case("ragged")
    for k in (0, 1):
        a = _device("ragged", k)
        b = _device_tables(f, None, mi, mj, T, k)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        one = _device_tables(f[2:3], None, mi, mj, T, k)
        assert one[0][0].tobytes() == a[0][2].tobytes() and one[1][0].tobytes() == a[1][2].tobytes()
    # a mask equals the same cells set to NaN
    lines, mask = vl.case("lines")
    _, _, T, _, mi, mj, _ = vl.CASES["lines"]
    a = _device("lines", 1)
    b = _device_tables(np.where(mask[None], lines, np.nan), None, mi, mj, T, 1)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert a[1].sum() < _device_tables(lines, None, mi, mj, T, 1)[1].sum()


def test_local_variogram_map_equals_the_c_abi_and_slicing_changes_nothing():
    import torch
    from mcmc_gpu_amd import variogram
    H, W, T, _, mi, mj, R = vl.CASES["ragged"]
    f, _ = vl.case("ragged")
    maxlag = 500.0 * mj + 250.0
    xx, yy = vc.grid_of(H, W, 500.0, -maxlag / (mi + 0.5))
    whole = variogram.local_variogram_map(xx, yy, f, maxlag, T, half_window=1)
    ref = _device("ragged", 1)
    assert whole.sum.shape == (R, 5, 9, mi + 1, 2 * mj + 1) and whole.xc.shape == whole.yc.shape == (5, 9)
    assert whole.sum.tobytes() == ref[0].tobytes() and whole.count.tobytes() == ref[1].tobytes()
    sliced = variogram.local_variogram_map(xx, yy, torch.as_tensor(np.ascontiguousarray(f)).cuda(), maxlag, T, half_window=1, _fields_per_part=2)
    for name in ("sum", "count", "gamma", "total_sum", "total_count"):
        assert getattr(sliced, name).tobytes() == getattr(whole, name).tobytes(), name
    np.testing.assert_array_equal(whole.total_count, vl.tiles_of("ragged")[1].sum(axis=(1, 2)))
    np.testing.assert_array_equal(whole.xc[0], 1000.0 + 500.0 * np.array([3.5, 11.5, 19.5, 27.5, 35.5, 43.5, 51.5, 59.5, 66.5]))
    np.testing.assert_array_equal(whole.dj[0], np.arange(-mj, mj + 1))
    with np.errstate(invalid="ignore", divide="ignore"):
        np.testing.assert_array_equal(whole.gamma, np.where(whole.count > 0, whole.sum / (2.0 * whole.count), np.nan))


def test_c_abi_refusals_write_nothing():
    import torch
    from mcmc_gpu_amd.engine import GsmEngine, _ptr
    from mcmc_gpu_amd._lib import GsmError
    H, W, T, _, mi, mj, R = vl.CASES["one"]
    f, _ = vl.case("one")
    T = 8
    Ty, Tx = vl.lattice(H, W, T)
    eng = GsmEngine(H, W, 1)
    try:
        d_f = torch.as_tensor(np.ascontiguousarray(f)).to(eng.dev)
        d_s = torch.full((R, Ty, Tx, mi + 1, 2 * mj + 1), -1.0, dtype=torch.float64, device=eng.dev)
        d_c = torch.full((R, Ty, Tx, mi + 1, 2 * mj + 1), -1, dtype=torch.int64, device=eng.dev)
        null = C.c_void_p(0)

        def call(fields=_ptr(d_f), n=R, a=mi, b=mj, tile=T, k=1, s=_ptr(d_s), c=_ptr(d_c)):
            return eng.lib.gsm_variogram_local(eng.h, fields, n, null, a, b, tile, k, s, c, eng._stream())

        refused = [(dict(fields=null), -1), (dict(s=null), -1), (dict(c=null), -1), (dict(n=0), -1), (dict(a=-1), -1), (dict(b=-1), -1),
                   (dict(tile=1), -1), (dict(k=-1), -1),                                     # GSM_E_ARG
                   (dict(a=1 << 20, b=1 << 20, tile=2), -4),                                 # more than 2^31 entries per field
                   (dict(a=(1 << 20) + 1), -4)]                                              # GSM_E_UNSUPPORTED
        for bad, code in refused:
            assert call(**bad) == code, bad
            assert "gsm_variogram_local" in eng.lib.gsm_last_error(eng.h).decode()
            with pytest.raises(GsmError, match="gsm_variogram_local"):
                eng._check(call(**bad))
        torch.cuda.synchronize()
        assert torch.all(d_s == -1.0) and torch.all(d_c == -1)                               # a refused call writes nothing
        eng._check(call())                                                                   # a valid call afterwards succeeds
        torch.cuda.synchronize()
        s, c = d_s.cpu().numpy(), d_c.cpu().numpy()
    finally:
        eng.close()
    ref = [vl.windows(*vl.tile_tables(z, mi, mj, T), 1) for z in f]
    np.testing.assert_array_equal(c, np.array([k for _, k in ref]))
    vc.assert_within_bound(s, np.array([k for k, _ in ref]), c)


def test_local_variograms_end_to_end_fits_equal_the_fits_of_the_checker_tables():
    """The two-regime field (128 x 128 at 500 m, T 16, k 1, offsets within 10 cells, exponential): local_variograms on the device
    returns maps of the grid's shape without NaN that interpolate.krige_scores accepts, and every window's fitted parameters
    equal fit_local on the checker's tables within the bar of variogram_local_common.fairness_bar (measured on the checker)."""
    from mcmc_gpu_amd import interpolate, variogram
    xx, yy, field = vl.two_regime()
    t = vl.TWO
    ref = vl.two_regime_fit()
    bar, keep = vl.fairness_bar()
    got = variogram.local_variograms(np.array(xx), np.array(yy), np.array(field), t["vtype"], t["m"] * t["dx"] + 1.0, t["T"],
                                     half_window=t["k"], normal_score=False)
    np.testing.assert_array_equal(got.fitted, ref.fitted)
    change = vl.window_change(got.windows, ref.windows)
    for p in vl.PARAMS:
        worst = float(np.max(change[p][keep & ref.fitted] if p == "azimuth" else change[p]))
        print(p, "largest change", worst, "bar", bar[p])
        assert worst <= bar[p], p
    for key in ("major_range", "minor_range", "azimuth", "sill"):
        assert got[key].shape == field.shape and np.isfinite(got[key]).all()
        if key != "azimuth":
            np.testing.assert_allclose(got[key], ref[key], rtol=1e-9)
    az = np.array([[w["azimuth"] for w in row] for row in got.windows])
    assert abs(np.median(az[:, :3]) - 30.0) <= 15.0 and abs(np.median(az[:, 5:]) - 120.0) <= 15.0
    # the maps go straight into the kriging kernels
    rng = np.random.default_rng(9)
    grid = np.full(field.shape, np.nan)
    at = rng.choice(field.size, 400, replace=False)
    grid.ravel()[at] = field.ravel()[at]
    est, var, nn = interpolate.krige_scores(np.array(xx), np.array(yy), grid, got, radius=10e3, num_points=8, quiet=True)
    assert est.shape == field.shape and np.isfinite(est).all() and np.all(var >= 0.0) and nn.max() <= 8
