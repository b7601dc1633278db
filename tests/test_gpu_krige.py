"""GPU: mcmc_gpu_amd.interpolate.krige / krige_scores (gsm_krige_grid, csrc/krige_grid_kernel.hip) against golden F15 -- the
reference's interpolate.krige (scripts/make_fixtures_krige.py) -- and, on the grids F15 leaves out (interp_sgs_common.geometry,
a 256 x 256 grid), against the CPU helper that F15 pins bit for bit (tests/krige_common.py, tests/test_krige_host.py), run with
the device's rule for equidistant candidates.  Bounds: the project's standing ones for this solver against numpy.linalg.lstsq
(test_gpu_interp_sgs.py)."""
import functools
from pathlib import Path

import numpy as np
import pytest

import interp_sgs_common as ic
import krige_common as kc

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
CASES = ic.geometry()
# G3d: G3 (rows half as far apart as columns, 48 points) with a value at every second row and column.  Kriging conditions on
# the measured values only, so on G3's own flight lines (5 rows, 7 columns apart) no cell finds six values in every octant
# (39 neighbours at most, where sequential simulation fills the octants with earlier cells); here 48-row systems are solved.
CASES["G3d"] = (*CASES["G3"][:2], np.where(ic._lines(48, 40, 2, 2), ic.field(48, 40, 23), np.nan), *CASES["G3"][3:])


def _clip(var):
    return np.where(var < 0, 0, var)


def _assert_cells(dev, ref_n, ref_est, ref_var, sill):
    """Per-cell results of the device (estimate, signed variance, neighbour count) against a reference's."""
    est, var, n = dev
    np.testing.assert_array_equal(n, ref_n)
    np.testing.assert_allclose(est, ref_est, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(var, ref_var, rtol=1e-7, atol=1e-9 * sill)
    np.testing.assert_allclose(np.sqrt(_clip(var)), np.sqrt(_clip(ref_var)), rtol=0, atol=1e-8)


def _assert_maps(got, exp, grid):
    """krige's two maps in data units against the expected ones."""
    span = float(np.nanmax(grid) - np.nanmin(grid))
    cond = ~np.isnan(grid)
    for a, b in zip(got, exp):
        assert a.shape == grid.shape
        np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-6 * span, equal_nan=True)
        assert np.array_equal(a[cond], b[cond])                                          # conditioning cells: bit for bit


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_krige_equals_reference_fixture(tag):
    from mcmc_gpu_amd import interpolate
    xx, yy, grid, cases = ic.small()
    vario, kw, _ = cases[tag]
    kw = kc.krige_kw(kw)
    g = np.load(GOLD / f"f15{tag}_krige.npz", allow_pickle=False)
    plan = kc.plan_of(xx, yy, grid, vario, kw)
    cells = interpolate._krige_cells(plan)
    _assert_cells(interpolate._krige_run(plan), g["n"], g["est_var"][:, 0], g["est_var"][:, 1], vario["sill"])
    est_ns, var_ns, n = interpolate.krige_scores(xx, yy, grid, vario, **kw)
    np.testing.assert_array_equal(n.ravel()[cells], g["n"])
    assert n.dtype == np.int32 and n.sum() == g["n"].astype(np.int64).sum()              # 0 where no system was solved
    np.testing.assert_array_equal(np.isnan(est_ns), np.isnan(g["est_ns"]))
    np.testing.assert_allclose(est_ns, g["est_ns"], rtol=1e-9, atol=1e-12, equal_nan=True)
    assert np.all(var_ns >= 0.0)
    np.testing.assert_allclose(np.sqrt(var_ns), g["std_ns"], rtol=0, atol=1e-8)
    assert np.array_equal(est_ns[plan.cond], g["est_ns"][plan.cond])
    _assert_maps(interpolate.krige(xx, yy, grid, vario, **kw), (g["est"], g["std"]), grid)


@functools.lru_cache(maxsize=None)
def _cpu(cid):
    xx, yy, grid, vario, kw, _ = CASES[cid]
    plan = kc.plan_of(xx, yy, grid, vario, kw)
    return kc.krige_scores_cpu(xx, yy, plan.grid_ns, dict(vario), kw["radius"], kw["num_points"], kw["ktype"],
                               sim_mask=kw.get("sim_mask"), stable_ties=True)


@pytest.mark.parametrize("cid", sorted(CASES))
def test_krige_equals_cpu_helper_on_geometry_cases(cid):
    from mcmc_gpu_amd import interpolate
    xx, yy, grid, vario, kw, _ = CASES[cid]
    kw = kc.krige_kw(kw)
    est_ns, var, tr, radii = _cpu(cid)
    if cid == "G5":                                                                      # what the case is there for
        assert tr[:, 2].min() == 1 and (radii == 10e3 + 200e3).any() and radii.max() == 10e3 + 400e3
    if cid == "G3":
        assert tr[:, 2].max() > 32 and radii.max() == kw["radius"]
    if cid == "G3d":
        assert tr[:, 2].max() == 48
    if cid == "G7":
        assert radii.max() > kw["radius"]
    plan = kc.plan_of(xx, yy, grid, vario, kw)
    np.testing.assert_array_equal(interpolate._krige_cells(plan), tr[:, 0] * plan.W + tr[:, 1])
    _assert_cells(interpolate._krige_run(plan), tr[:, 2], tr[:, 3], tr[:, 4], vario["sill"])
    _assert_maps(interpolate.krige(xx, yy, grid, vario, **kw), interpolate._data_maps(plan, est_ns, _clip(var)), grid)


def test_launch_geometry_changes_no_bit():
    from mcmc_gpu_amd import interpolate
    xx, yy, grid, cases = ic.small()
    vario, kw, _ = cases["a"]
    full = interpolate.krige_scores(xx, yy, grid, vario, **kw)
    again = interpolate.krige_scores(xx, yy, grid, vario, **kw)
    win = np.zeros(grid.shape, bool)
    win[10:17, 12:21] = True                                                             # 7 x 9 cells inside the data gap
    assert not (win & ~np.isnan(grid)).any()
    part = interpolate.krige_scores(xx, yy, grid, vario, sim_mask=win, **kw)
    for f, a, p in zip(full, again, part):
        assert np.array_equal(f, a, equal_nan=True)
        assert np.array_equal(f[win], p[win])
    assert np.all(part[2][~win] == 0) and np.all(part[2][win] >= 1)
    assert np.isnan(part[0][~win & np.isnan(grid)]).all()


def _small_plan():
    xx, yy, grid, cases = ic.small()
    vario, kw, _ = cases["a"]
    return kc.plan_of(xx, yy, grid, vario, kw)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_lag_table_too_small_raises(monkeypatch):
    from mcmc_gpu_amd import interpolate, _lib
    good = interpolate._krige_run(_small_plan())
    with monkeypatch.context() as m:
        m.setattr(interpolate, "_lag_extents", lambda plan, eng, torch: (1, 1))
        with pytest.raises(_lib.GsmError, match="lag covariance table"):
            interpolate._krige_run(_small_plan())
    assert _same(interpolate._krige_run(_small_plan()), good)


def test_listed_cell_holding_a_value_raises():
    from mcmc_gpu_amd import interpolate, _lib
    plan = _small_plan()
    good = interpolate._krige_run(plan)
    cells = interpolate._krige_cells(plan).copy()
    assert plan.cond[0, 0]
    cells[7] = 0                                                                         # cell (0, 0) is conditioning data
    with pytest.raises(_lib.GsmError, match="holding a value"):
        interpolate._krige_run(plan, cells)
    assert _same(interpolate._krige_run(_small_plan()), good)
    cells[7] = plan.H * plan.W                                                           # one past the grid
    with pytest.raises(_lib.GsmError, match="outside the grid"):
        interpolate._krige_run(plan, cells)
    assert _same(interpolate._krige_run(_small_plan()), good)


def test_whole_grid_at_size():
    """The 256 x 256 grid of test_gpu_interp_sgs.test_whole_grid_at_size_with_bounds: 48 neighbours within 30 km at 500 m, a
    30 x 40 km hole in the data."""
    from mcmc_gpu_amd import interpolate
    H = W = 256
    xx, yy = np.meshgrid(np.arange(W) * 500.0, np.arange(H) * 500.0)
    bed = ic.field(H, W, 5)
    cond = np.zeros((H, W), bool)
    cond[::12, :] = True
    cond[:, ::20] = True
    cond[100:160, 60:140] = False
    grid = np.where(cond, bed, np.nan)
    vario = dict(major_range=20e3, minor_range=20e3, azimuth=0.0, sill=1.0, nugget=0.0, vtype="Matern", s=1.5)
    kw = dict(radius=30e3, num_points=48, ktype="ok")
    sim, std = interpolate.krige(xx, yy, grid, vario, **kw)
    assert sim.shape == std.shape == (H, W) and np.isfinite(sim).all() and np.isfinite(std).all()
    assert sim.min() >= np.nanmin(grid) and sim.max() <= np.nanmax(grid)                 # the transformer clips
    plan = kc.plan_of(xx, yy, grid, vario, kw)
    assert np.array_equal(sim[cond], interpolate._inverse(plan, plan.grid_ns)[cond])    # the reference's round trip
    cells = interpolate._krige_cells(plan)
    est, var, n = interpolate._krige_run(plan)
    assert cells.size == (~cond).sum() and n.min() >= 1 and n.max() == 48
    est_ns, var_ns, _ = interpolate._score_maps(plan, cells, est, var, n)
    _assert_maps((sim, std), interpolate._data_maps(plan, est_ns, var_ns), grid)         # the public call is this run
    rng = np.random.default_rng(0)
    hole = np.zeros((H, W), bool)
    hole[100:160, 60:140] = True
    pick = np.sort(np.concatenate([rng.choice(np.flatnonzero(hole & ~cond), 100, replace=False),
                                   rng.choice(np.flatnonzero(~hole & ~cond), 100, replace=False)]))
    _, _, tr, _ = kc.krige_scores_cpu(xx, yy, plan.grid_ns, dict(vario), kw["radius"], kw["num_points"], kw["ktype"],
                                      stable_ties=True, cells=pick)
    at = np.searchsorted(cells, pick)
    assert np.array_equal(cells[at], pick) and np.array_equal(tr[:, 0] * W + tr[:, 1], pick)
    _assert_cells((est[at], var[at], n[at]), tr[:, 2], tr[:, 3], tr[:, 4], vario["sill"])
