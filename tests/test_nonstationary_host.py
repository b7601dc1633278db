"""not gpu: non-stationary interpolate.sgs / interpolate.krige on the host side.

The CPU restatement with a variogram per cell (tests/nonstationary_common.py, assembled from oracle/sgs_oracle.py) against
goldens F16 and F17 -- the unmodified reference's interpolate.sgs and interpolate.krige with every variogram parameter a map
(scripts/make_fixtures_nonstationary.py).  Equality, not a tolerance: this pins what tests/test_gpu_nonstationary.py compares
the device with on the grids the fixtures leave out.  Then interpolate._Plan's per-cell table against
oracle/mcmc_oracle.rotation_matrix, bit for bit, and the refusals that need no device."""
import json
from pathlib import Path

import numpy as np
import pytest

import mcmc_oracle as orc
import nonstationary_common as nc

GOLD = Path(__file__).resolve().parent / "golden"
pytest.importorskip("scipy.stats")
pytest.importorskip("sklearn.preprocessing")


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_restatement_reproduces_nonstationary_sgs_fixture(tag):
    from mcmc_gpu_amd import interpolate
    xx, yy, grid, cases = nc.small()
    vario, kw, seeds = cases[tag]
    g = np.load(GOLD / f"f16{tag}_nonstationary.npz", allow_pickle=False)
    plan = nc.plan_of(xx, yy, grid, vario, kw)
    for s in seeds:
        rng = np.random.default_rng(s)
        trace = []
        out = nc.sgs_local(xx, yy, plan.grid_ns, vario, kw["radius"], kw["num_points"], kw["ktype"], sim_mask=kw.get("sim_mask"),
                           rng=rng, trace=trace, bounds=plan.bounds)
        tr = np.array(trace)
        assert rng.bit_generator.state == json.loads(str(g[f"{s}_state"]))
        assert np.array_equal(out, g[f"{s}_ns"], equal_nan=True)
        assert np.array_equal(interpolate._inverse(plan, out), g[f"{s}_sim"], equal_nan=True)
        assert np.array_equal(tr[:, 0] * xx.shape[1] + tr[:, 1], g[f"{s}_cells"])
        assert np.array_equal(tr[:, 2], g[f"{s}_n"])
        assert np.array_equal(tr[:, 3:5], g[f"{s}_est_var"])
        assert tag == "c" or tr[:, 5].max() > kw["radius"]                 # the data gap: some search widens (c's mask and 4 km radius: none)


@pytest.mark.parametrize("tag", nc.KRIGE_TAGS)
def test_restatement_reproduces_nonstationary_krige_fixture(tag):
    from mcmc_gpu_amd import interpolate
    xx, yy, grid, cases = nc.small()
    vario, kw, _ = cases[tag]
    g = np.load(GOLD / f"f17{tag}_krige_nonstationary.npz", allow_pickle=False)
    plan = nc.plan_of(xx, yy, grid, vario, kw, bounds=False)
    est_ns, var, tr = nc.krige_local(xx, yy, plan.grid_ns, vario, kw["radius"], kw["num_points"], kw["ktype"],
                                     sim_mask=kw.get("sim_mask"))
    assert np.array_equal(tr[:, 0] * plan.W + tr[:, 1], interpolate._krige_cells(plan))
    assert np.array_equal(tr[:, 2], g["n"]) and np.array_equal(tr[:, 3:], g["est_var"])
    var = np.where(var < 0, 0, var)
    assert np.array_equal(est_ns, g["est_ns"], equal_nan=True) and np.array_equal(np.sqrt(var), g["std_ns"])
    est, std = interpolate._data_maps(plan, est_ns, var)
    assert np.array_equal(est, g["est"], equal_nan=True) and np.array_equal(std, g["std"], equal_nan=True)


def _expected_table(vario, shape):
    H, W = shape
    full = {k: (v if isinstance(v, np.ndarray) else np.full(shape, v)) for k, v in vario.items() if k != "vtype"}
    exp = np.empty((H * W, 6))
    for i in range(H):
        for j in range(W):
            R = orc.rotation_matrix(full["azimuth"][i, j], full["major_range"][i, j], full["minor_range"][i, j])
            exp[i * W + j] = (R[0, 0], R[0, 1], R[1, 0], R[1, 1], full["sill"][i, j], full["nugget"][i, j])
    return exp


@pytest.mark.parametrize("tag", ["a", "c"])
def test_plan_table_equals_rotation_matrix_cell_by_cell(tag):
    xx, yy, grid, cases = nc.small()
    vario, kw, _ = cases[tag]
    plan = nc.plan_of(xx, yy, grid, vario, kw)
    assert plan.local.shape == (grid.size, 6) and plan.local.dtype == np.float64 and plan.local.flags.c_contiguous
    assert np.array_equal(plan.local, _expected_table(vario, grid.shape))


def test_plan_table_broadcasts_numbers_and_scalar_calls_have_no_table():
    xx, yy, grid, cases = nc.small()
    vario, kw, _ = cases["a"]
    mixed = dict(vario, azimuth=37.5, nugget=0, minor_range=4100)          # ints and floats among the maps
    plan = nc.plan_of(xx, yy, grid, mixed, kw)
    assert np.array_equal(plan.local, _expected_table(mixed, grid.shape))
    spelled = {k: (v if isinstance(v, (np.ndarray, str)) else np.full(grid.shape, float(v))) for k, v in mixed.items()}
    assert np.array_equal(nc.plan_of(xx, yy, grid, spelled, kw).local, plan.local)
    scalar = dict(major_range=8000.0, minor_range=5000.0, azimuth=30.0, sill=1.0, nugget=0.0, vtype="Exponential")
    assert nc.plan_of(xx, yy, grid, scalar, kw).local is None


def test_nan_is_an_error_only_inside_sim_mask():
    xx, yy, grid, cases = nc.small()
    vario, kw, _ = cases["c"]
    mask = kw["sim_mask"]
    holed = dict(vario, sill=np.where(mask, vario["sill"], np.nan), major_range=np.where(mask, vario["major_range"], np.nan))
    plan = nc.plan_of(xx, yy, grid, holed, kw)
    inside = mask.ravel()
    assert np.array_equal(plan.local[inside], nc.plan_of(xx, yy, grid, vario, kw).local[inside])
    assert np.isnan(plan.local[~inside][:, [0, 2, 4]]).all()
    bad = vario["nugget"].copy()
    bad[10, 12] = np.nan
    assert mask[10, 12]
    with pytest.raises(ValueError, match="nugget contains NaN in sim_mask"):
        nc.plan_of(xx, yy, grid, dict(vario, nugget=bad), kw)
    with pytest.raises(ValueError, match="nugget contains NaN"):
        nc.plan_of(xx, yy, grid, dict(vario, nugget=bad), dict(kw, sim_mask=None))


def test_matern_with_a_map_and_a_wrongly_shaped_map_are_refused():
    xx, yy, grid, cases = nc.small()
    vario, kw, _ = cases["a"]
    with pytest.raises(NotImplementedError, match="Bessel K"):
        nc.plan_of(xx, yy, grid, dict(vario, vtype="Matern", s=1.5), kw)
    with pytest.raises(NotImplementedError, match="Bessel K"):
        nc.plan_of(xx, yy, grid, dict(major_range=6000.0, minor_range=6000.0, azimuth=0.0, sill=vario["sill"], nugget=0.0,
                                     vtype="matern", s=1.5), kw)
    with pytest.raises(ValueError, match="shape"):
        nc.plan_of(xx, yy, grid, dict(vario, sill=vario["sill"][:, :-1]), kw)
    with pytest.raises(ValueError, match="shape"):
        nc.plan_of(xx, yy, grid, dict(vario, azimuth=vario["azimuth"].ravel()), kw)
