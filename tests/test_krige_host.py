"""not gpu: the host side of mcmc_gpu_amd.interpolate.krige.  The CPU helper of tests/krige_common.py against golden F15 (the
reference's interpolate.krige, scripts/make_fixtures_krige.py) -- equality, not a tolerance: this pins the helper that
tests/test_gpu_krige.py compares the device with on grids the fixtures do not hold.  Then the library's new entry point, the
finishing step (a pure function of the per-cell results) and the argument errors."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import interp_sgs_common as ic
import krige_common as kc

GOLD = Path(__file__).resolve().parent / "golden"
pytest.importorskip("scipy.spatial")
pytest.importorskip("sklearn.preprocessing")


def _case(tag):
    xx, yy, grid, cases = ic.small()
    vario, kw, _ = cases[tag]
    return xx, yy, grid, vario, kc.krige_kw(kw), np.load(GOLD / f"f15{tag}_krige.npz", allow_pickle=False)


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_cpu_helper_reproduces_krige_fixture(tag):
    from mcmc_gpu_amd import interpolate
    xx, yy, grid, vario, kw, g = _case(tag)
    plan = kc.plan_of(xx, yy, grid, vario, kw)
    est_ns, var, tr, _ = kc.krige_scores_cpu(xx, yy, plan.grid_ns, dict(vario), kw["radius"], kw["num_points"], kw["ktype"],
                                             sim_mask=kw.get("sim_mask"))
    cells = interpolate._krige_cells(plan)
    np.testing.assert_array_equal(tr[:, 0] * plan.W + tr[:, 1], cells)                  # C order of the cells without a value
    np.testing.assert_array_equal(tr[:, 2], g["n"])
    np.testing.assert_array_equal(tr[:, 3:], g["est_var"])
    assert tr[:, 2].min() == 1 and tr[:, 2].max() == kw["num_points"]                   # widened searches and full systems
    std_ns = np.sqrt(np.where(var < 0, 0, var))
    np.testing.assert_array_equal(est_ns, g["est_ns"])
    np.testing.assert_array_equal(std_ns, g["std_ns"])
    est, std = interpolate._data_maps(plan, est_ns, np.where(var < 0, 0, var))
    np.testing.assert_array_equal(est, g["est"])
    np.testing.assert_array_equal(std, g["std"])
    # the same through the product's own finishing step
    e2, v2, n2 = interpolate._score_maps(plan, cells, tr[:, 3], tr[:, 4], tr[:, 2].astype(np.int32))
    np.testing.assert_array_equal(e2, g["est_ns"])
    np.testing.assert_array_equal(np.sqrt(v2), g["std_ns"])
    np.testing.assert_array_equal(n2.ravel()[cells], g["n"])
    assert n2.sum() == g["n"].astype(np.int64).sum()


def test_library_declares_and_exports_gsm_krige_grid():
    from mcmc_gpu_amd import _lib
    assert "krige_grid_kernel.hip" in _lib.SOURCES and (_lib.CSRC / "krige_grid_kernel.hip").exists()
    assert "gsm_krige_grid" in _lib.declared_symbols()
    lib = _lib.load()
    assert hasattr(lib, "gsm_krige_grid") and len(lib.gsm_krige_grid.argtypes) == 17
    out = subprocess.run(["strings", "-n", "6", str(_lib.LIB_PATH)], capture_output=True, text=True).stdout
    assert "krige_grid_kernel" in out                                                    # the kernel is in the gfx950 code object
    from mcmc_gpu_amd import interpolate
    assert {"krige", "krige_scores", "sgs", "sgs_many"} <= set(interpolate.__all__)


def _toy_plan():
    from mcmc_gpu_amd import interpolate
    xx, yy, grid, vario, kw, _ = _case("c")
    plan = kc.plan_of(xx, yy, grid, vario, kw)
    return interpolate, plan, interpolate._krige_cells(plan), grid, kw["sim_mask"]


def test_finish_clips_a_negative_variance_to_sd_zero():
    interpolate, plan, cells, grid, _ = _toy_plan()
    est = np.linspace(-1.0, 1.0, cells.size)
    var = np.full(cells.size, 0.25)
    var[::3] = -1e-9
    est_ns, var_ns, n_map = interpolate._score_maps(plan, cells, est, var, np.full(cells.size, 7, dtype=np.int32))
    assert np.all(var_ns.ravel()[cells[::3]] == 0.0) and np.all(var_ns.ravel()[cells[1::3]] == 0.25)
    assert np.all(var_ns >= 0.0)
    _, std = interpolate._data_maps(plan, est_ns, var_ns)
    median = plan.nst.inverse_transform(np.zeros((1, 1)))[0, 0]                          # the quantile whose score is sd = 0
    assert np.all(std.ravel()[cells[::3]] == median) and np.all(std.ravel()[cells[1::3]] > median)
    assert np.all(std[plan.cond] == median)
    assert n_map.dtype == np.int32 and np.all(n_map.ravel()[cells] == 7) and n_map.sum() == 7 * cells.size


def test_finish_leaves_nan_outside_sim_mask_and_keeps_the_data_round_trip():
    interpolate, plan, cells, grid, sim_mask = _toy_plan()
    est_ns, var_ns, n_map = interpolate._score_maps(plan, cells, np.zeros(cells.size), np.ones(cells.size),
                                                    np.ones(cells.size, dtype=np.int32))
    sim, std = interpolate._data_maps(plan, est_ns, var_ns)
    outside = ~sim_mask & np.isnan(grid)
    assert outside.any() and np.isnan(sim[outside]).all() and np.isnan(est_ns[outside]).all()
    assert np.all(n_map[outside] == 0) and np.all(var_ns[outside] == 0.0)
    assert np.isfinite(sim[sim_mask | plan.cond]).all() and np.isfinite(std).all()
    # conditioning cells: the transformer's round trip of the data, untouched by the finishing step
    assert np.array_equal(sim[plan.cond], interpolate._inverse(plan, plan.grid_ns)[plan.cond])
    np.testing.assert_allclose(sim[plan.cond], grid[plan.cond], rtol=0, atol=1e-6 * float(np.nanmax(grid) - np.nanmin(grid)))
    assert np.array_equal(est_ns[plan.cond], plan.grid_ns[plan.cond])


def test_argument_errors_follow_the_reference():
    from mcmc_gpu_amd import interpolate
    xx, yy, grid, vario, kw, _ = _case("a")
    for fn in (interpolate.krige, interpolate.krige_scores):
        run = lambda **o: fn(**{**dict(xx=xx, yy=yy, grid=grid, variogram=vario, radius=3000.0, num_points=16), **o})
        cases = [
            (dict(ktype="uk"), ValueError, "ktype must be 'ok' or 'sk'"),
            (dict(variogram={k: v for k, v in vario.items() if k not in ("sill", "azimuth")}), ValueError, "Variogram missing azimuth, sill"),
            (dict(grid=grid[:, :-1]), ValueError, "xx, yy, and grid must have same shape"),
            (dict(xx=xx[0]), ValueError, "xx must be a 2D NumPy array"),
            (dict(sim_mask=np.ones((3, 3), bool)), ValueError, "sim_mask shape must be same as grid"),
            (dict(radius="far"), ValueError, "radius must be a number"),
            (dict(stencil=np.ones((5, 5))), NotImplementedError, "stencil"),
            (dict(variogram={**vario, "sill": np.ones(grid.shape)}), NotImplementedError, "scalar variogram"),
            (dict(num_points=4), NotImplementedError, "num_points"),
            (dict(grid=np.full(grid.shape, np.nan)), ValueError, "no conditioning value"),
        ]
        for over, exc, msg in cases:
            with pytest.raises(exc, match=msg):
                run(**over)
        with pytest.raises(TypeError):
            run(bounds=(0.0, 1.0))                                                       # krige has no bounds, as in the reference
