"""GPU: non-stationary interpolate.sgs / sgs_many / krige / krige_scores -- variogram parameters as maps of the grid's shape, the
per-cell-variogram kernels behind gsm_sgs_grid_local and gsm_krige_grid_local (csrc/sgs_search.h's LocalCov).

  1. against goldens F16 and F17: the unmodified reference with every parameter a map (scripts/make_fixtures_nonstationary.py);
  2. against the CPU restatement that those goldens pin bit for bit (tests/nonstationary_common.py,
     tests/test_nonstationary_host.py) on grids the goldens leave out: descending axes, cells far from square, 48-point
     systems, systems of one neighbour after two widenings; run with the device's rule for equidistant candidates;
  3. constant maps against the scalar call of the same variogram (in-kernel covariance against the host's table);
  4. batching, segments and number / map mixes change no bit;
  5. refusals.
Bounds: those of test_gpu_interp_sgs.py and test_gpu_krige.py, the variance's absolute term scaled with the largest sill of
the maps.  Every visited cell is compared."""
import ctypes as C
import functools
import json
from pathlib import Path

import numpy as np
import pytest

import nonstationary_common as nc

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
GEOM = nc.geometry()


def _sill_max(vario):
    return float(np.max(vario["sill"]))


def _clip(var):
    return np.where(var < 0, 0, var)


def _assert_sgs_realisation(plan, grid, sill, ns, path, t, ref_cells, ref_n, ref_est, ref_var, ref_ns):
    """One realisation of the device (normal scores, path, trace) against a reference's, every visited cell."""
    np.testing.assert_array_equal(path, ref_cells)                                                   # visiting order
    solved = t[:, 0] >= 0                                            # cells whose bounds coincide solve no system on the device
    if plan.bounds is not None:
        lo, hi = plan.bounds
        np.testing.assert_array_equal(~solved, (lo.ravel() == hi.ravel())[path])
    else:
        assert solved.all()
    np.testing.assert_array_equal(t[solved, 0], ref_n[solved])                                       # neighbour counts
    np.testing.assert_allclose(t[solved, 1], ref_est[solved], rtol=1e-9, atol=1e-12)                 # kriging estimates
    np.testing.assert_allclose(t[solved, 2], ref_var[solved], rtol=1e-7, atol=1e-9 * sill)           # |kriging variances|
    np.testing.assert_array_equal(np.isnan(ns), np.isnan(ref_ns))
    np.testing.assert_allclose(ns, ref_ns, rtol=0, atol=1e-8, equal_nan=True)                        # normal scores
    cond = ~np.isnan(grid)
    assert np.array_equal(ns[cond], ref_ns[cond])                                                    # conditioning cells: bit for bit


def _assert_krige_cells(dev, ref_n, ref_est, ref_var, sill):
    est, var, n = dev
    np.testing.assert_array_equal(n, ref_n)
    np.testing.assert_allclose(est, ref_est, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(var, ref_var, rtol=1e-7, atol=1e-9 * sill)
    np.testing.assert_allclose(np.sqrt(_clip(var)), np.sqrt(_clip(ref_var)), rtol=0, atol=1e-8)


def _assert_maps(got, exp, grid):
    span = float(np.nanmax(grid) - np.nanmin(grid))
    cond = ~np.isnan(grid)
    for a, b in zip(got, exp):
        assert a.shape == grid.shape
        np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-6 * span, equal_nan=True)
        assert np.array_equal(a[cond], b[cond])


# ---- 1. the reference's own outputs ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_sgs_equals_reference_fixture(tag):
    from mcmc_gpu_amd import interpolate
    xx, yy, grid, cases = nc.small()
    vario, kw, seeds = cases[tag]
    g = np.load(GOLD / f"f16{tag}_nonstationary.npz", allow_pickle=False)
    plan = nc.plan_of(xx, yy, grid, vario, kw)
    rngs = [np.random.default_rng(s) for s in seeds]
    ns, (paths, tr) = interpolate._run(plan, rngs, trace=True)
    sim = interpolate._inverse(plan, ns)
    off = np.concatenate([[0], np.cumsum([p.size for p in paths])])
    span = float(np.nanmax(grid) - np.nanmin(grid))
    cond = ~np.isnan(grid)
    for r, s in enumerate(seeds):
        assert json.loads(str(g[f"{s}_state"])) == rngs[r].bit_generator.state                       # generator state
        ev = g[f"{s}_est_var"]
        _assert_sgs_realisation(plan, grid, _sill_max(vario), ns[r], paths[r], tr[off[r]:off[r + 1]], g[f"{s}_cells"],
                                g[f"{s}_n"].astype(np.float64), ev[:, 0], ev[:, 1], g[f"{s}_ns"])
        np.testing.assert_allclose(sim[r], g[f"{s}_sim"], rtol=0, atol=1e-6 * span, equal_nan=True)  # returned maps
        assert np.array_equal(sim[r][cond], g[f"{s}_sim"][cond])
        if plan.bounds is not None:
            deg = (plan.bounds[0] == plan.bounds[1]) & ~np.isnan(g[f"{s}_ns"]) & ~cond
            assert deg.any() and np.array_equal(sim[r][deg], g[f"{s}_sim"][deg])
    public = interpolate.sgs(xx, yy, grid, vario, seed=seeds[0], **kw)                               # the public entry is this run
    assert np.array_equal(public, sim[0], equal_nan=True)


@pytest.mark.parametrize("tag", nc.KRIGE_TAGS)
def test_krige_equals_reference_fixture(tag):
    from mcmc_gpu_amd import interpolate
    xx, yy, grid, cases = nc.small()
    vario, kw, _ = cases[tag]
    kw = {k: v for k, v in kw.items() if k != "bounds"}
    g = np.load(GOLD / f"f17{tag}_krige_nonstationary.npz", allow_pickle=False)
    plan = nc.plan_of(xx, yy, grid, vario, kw)
    cells = interpolate._krige_cells(plan)
    assert cells.size == g["n"].size
    _assert_krige_cells(interpolate._krige_run(plan), g["n"], g["est_var"][:, 0], g["est_var"][:, 1], _sill_max(vario))
    est_ns, var_ns, n = interpolate.krige_scores(xx, yy, grid, vario, **kw)
    np.testing.assert_array_equal(n.ravel()[cells], g["n"])
    assert n.dtype == np.int32 and n.sum() == g["n"].astype(np.int64).sum()
    np.testing.assert_array_equal(np.isnan(est_ns), np.isnan(g["est_ns"]))
    np.testing.assert_allclose(est_ns, g["est_ns"], rtol=1e-9, atol=1e-12, equal_nan=True)
    assert np.all(var_ns >= 0.0)                                                                     # clipped as the reference clips
    np.testing.assert_allclose(np.sqrt(var_ns), g["std_ns"], rtol=0, atol=1e-8)
    assert np.array_equal(est_ns[plan.cond], g["est_ns"][plan.cond])
    _assert_maps(interpolate.krige(xx, yy, grid, vario, **kw), (g["est"], g["std"]), grid)


# ---- 2. the CPU restatement on other geometries ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cpu_sgs(cid):
    xx, yy, grid, vario, kw, seeds = GEOM[cid]
    plan = nc.plan_of(xx, yy, grid, vario, kw)
    runs = {}
    for s in seeds:
        rng = np.random.default_rng(s)
        trace = []
        out = nc.sgs_local(xx, yy, plan.grid_ns, vario, kw["radius"], kw["num_points"], kw["ktype"], sim_mask=kw.get("sim_mask"),
                           rng=rng, trace=trace, bounds=plan.bounds, stable_ties=True)
        runs[s] = (out, np.array(trace), rng.bit_generator.state)
    return runs


@pytest.mark.parametrize("cid", sorted(GEOM))
def test_sgs_equals_cpu_restatement_on_geometry_cases(cid):
    from mcmc_gpu_amd import interpolate
    xx, yy, grid, vario, kw, seeds = GEOM[cid]
    ref = _cpu_sgs(cid)
    n_all = np.concatenate([ref[s][1][:, 2] for s in seeds])
    rad = np.concatenate([ref[s][1][:, 5] for s in seeds])
    if cid == "G1":                                                                  # what each case is here for
        assert yy[0, 0] > yy[1, 0] and rad.max() > kw["radius"]
    if cid == "G3":
        assert n_all.max() == 48
    if cid == "G4":
        assert n_all.max() == 16 and yy[0, 0] > yy[1, 0]
    if cid == "G5":
        assert n_all.min() == 1 and rad.max() >= 10e3 + 200e3
    plan = nc.plan_of(xx, yy, grid, vario, kw)
    rngs = [np.random.default_rng(s) for s in seeds]
    ns, (paths, tr) = interpolate._run(plan, rngs, trace=True)
    off = np.concatenate([[0], np.cumsum([p.size for p in paths])])
    for r, s in enumerate(seeds):
        out, t, state = ref[s]
        assert rngs[r].bit_generator.state == state
        _assert_sgs_realisation(plan, grid, _sill_max(vario), ns[r], paths[r], tr[off[r]:off[r + 1]], t[:, 0] * plan.W + t[:, 1],
                                t[:, 2], t[:, 3], t[:, 4], out)


@pytest.mark.parametrize("cid", ["G1", "G5"])
def test_krige_equals_cpu_restatement_on_geometry_cases(cid):
    from mcmc_gpu_amd import interpolate
    xx, yy, grid, vario, kw, _ = GEOM[cid]
    kw = {k: v for k, v in kw.items() if k != "bounds"}
    plan = nc.plan_of(xx, yy, grid, vario, kw)
    est_ns, var, tr = nc.krige_local(xx, yy, plan.grid_ns, vario, kw["radius"], kw["num_points"], kw["ktype"], stable_ties=True)
    np.testing.assert_array_equal(interpolate._krige_cells(plan), tr[:, 0] * plan.W + tr[:, 1])
    _assert_krige_cells(interpolate._krige_run(plan), tr[:, 2], tr[:, 3], tr[:, 4], _sill_max(vario))
    _assert_maps(interpolate.krige(xx, yy, grid, vario, **kw), interpolate._data_maps(plan, est_ns, _clip(var)), grid)


# ---- 3. constant maps against the scalar call ------------------------------------------------------------------------------------
SCALAR = {
    "exponential": (dict(major_range=7000.0, minor_range=4000.0, azimuth=35.0, sill=1.1, nugget=0.05, vtype="Exponential"), "a"),
    "spherical": (dict(major_range=7000.0, minor_range=4000.0, azimuth=35.0, sill=1.1, nugget=0.05, vtype="Spherical"), "b"),
    "gaussian": (dict(major_range=1750.0, minor_range=1000.0, azimuth=35.0, sill=1.1, nugget=0.05, vtype="Gaussian"), "c"),
}


@pytest.mark.parametrize("model", sorted(SCALAR))
def test_constant_maps_equal_the_scalar_call(model):
    from mcmc_gpu_amd import interpolate
    xx, yy, grid, cases = nc.small()
    scalar, tag = SCALAR[model]
    _, kw, seeds = cases[tag]
    maps = {k: (v if k == "vtype" else np.full(grid.shape, v)) for k, v in scalar.items()}
    p_s, p_m = nc.plan_of(xx, yy, grid, scalar, kw), nc.plan_of(xx, yy, grid, maps, kw)
    assert p_s.local is None and p_m.local is not None
    ns_s, (path_s, tr_s) = interpolate._run(p_s, [np.random.default_rng(seeds[0])], trace=True)
    ns_m, (path_m, tr_m) = interpolate._run(p_m, [np.random.default_rng(seeds[0])], trace=True)
    _assert_sgs_realisation(p_m, grid, scalar["sill"], ns_m[0], path_m[0], tr_m, path_s[0], tr_s[:, 0], tr_s[:, 1], tr_s[:, 2], ns_s[0])
    kkw = {k: v for k, v in kw.items() if k != "bounds"}
    k_s, k_m = nc.plan_of(xx, yy, grid, scalar, kkw), nc.plan_of(xx, yy, grid, maps, kkw)
    est, var, n = interpolate._krige_run(k_s)
    _assert_krige_cells(interpolate._krige_run(k_m), n, est, var, scalar["sill"])


# ---- 4. batching, segments, mixes ------------------------------------------------------------------------------------------------
def test_sgs_many_rows_segments_and_mixes_change_no_bit():
    from mcmc_gpu_amd import interpolate
    xx, yy, grid, cases = nc.small()
    vario, kw, _ = cases["b"]                                                        # bounds on
    g_many, g_one = np.random.default_rng(99), np.random.default_rng(99)
    many = interpolate.sgs_many(xx, yy, grid, vario, [21, g_many, 5, g_many], **kw)
    one = np.stack([interpolate.sgs(xx, yy, grid, vario, seed=s, **kw) for s in (21, g_one, 5, g_one)])
    assert np.array_equal(many, one, equal_nan=True)
    assert g_many.bit_generator.state == g_one.bit_generator.state
    seg64 = interpolate.sgs_many(xx, yy, grid, vario, [21, 99, 5], segment_cells=64, **kw)
    seg320 = interpolate.sgs_many(xx, yy, grid, vario, [21, 99, 5], segment_cells=320, **kw)
    assert np.array_equal(seg64, seg320, equal_nan=True) and np.array_equal(seg64[0], many[0], equal_nan=True)
    # numbers among the maps are broadcast: the same call as with every parameter spelled out as a map
    mixed = dict(vario, azimuth=40.0, nugget=0.03)
    spelled = dict(vario, azimuth=np.full(grid.shape, 40.0), nugget=np.full(grid.shape, 0.03))
    a = interpolate.sgs(xx, yy, grid, mixed, seed=21, **kw)
    b = interpolate.sgs(xx, yy, grid, spelled, seed=21, **kw)
    assert np.array_equal(a, b, equal_nan=True) and not np.array_equal(a, many[0], equal_nan=True)
    kkw = {k: v for k, v in kw.items() if k != "bounds"}
    for x, y in zip(interpolate.krige_scores(xx, yy, grid, mixed, **kkw), interpolate.krige_scores(xx, yy, grid, spelled, **kkw)):
        assert np.array_equal(x, y, equal_nan=True)


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals():
    import torch
    from mcmc_gpu_amd import interpolate, _lib
    from mcmc_gpu_amd.engine import GsmEngine
    xx, yy, grid, cases = nc.small()
    vario, kw, _ = cases["a"]
    with pytest.raises(NotImplementedError, match="Bessel K"):
        interpolate.sgs(xx, yy, grid, dict(vario, vtype="Matern", s=1.5), seed=1, **kw)
    with pytest.raises(NotImplementedError, match="Bessel K"):
        interpolate.krige(xx, yy, grid, dict(vario, vtype="Matern", s=1.5), **kw)
    with pytest.raises(ValueError, match="shape"):
        interpolate.sgs_many(xx, yy, grid, dict(vario, sill=vario["sill"][:-1]), [1], **kw)
    with pytest.raises(ValueError, match="shape"):
        interpolate.krige_scores(xx, yy, grid, dict(vario, major_range=vario["major_range"].T), **kw)
    # the C entry points: a model the kernels do not evaluate
    plan = nc.plan_of(xx, yy, grid, vario, kw)
    H, W = grid.shape
    eng = GsmEngine(H, W, 1)
    try:
        f64 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(eng.dev)
        ptr = lambda t: C.c_void_p(t.data_ptr())
        path, draws = plan.draws(np.random.default_rng(1))
        cells = interpolate._krige_cells(plan)
        d_grid, d_local, d_xs, d_ys, d_draw = f64(plan.grid_ns), f64(plan.local), f64(plan.xs), f64(plan.ys), f64(draws)
        d_path, d_cells = torch.as_tensor(path).to(eng.dev), torch.as_tensor(cells).to(eng.dev)
        d_off = torch.as_tensor(np.array([0, path.size], dtype=np.int64)).to(eng.dev)
        d_est, d_var = torch.empty(cells.size, dtype=torch.float64, device=eng.dev), torch.empty(cells.size, dtype=torch.float64, device=eng.dev)
        d_n = torch.empty(cells.size, dtype=torch.int32, device=eng.dev)
        before = d_grid.clone()
        for vtype in (3, -1, 7):                                                     # GSM_VTYPE_MATERN and two that are no model
            with torch.cuda.device(eng.dev):
                rc = eng.lib.gsm_sgs_grid_local(eng.h, ptr(d_grid), ptr(d_path), ptr(d_off), int(path.size), ptr(d_draw), None, None, 0,
                                                ptr(d_xs), ptr(d_ys), ptr(d_local), vtype, 6, 3000.0, 16, 64, None, eng._stream())
                assert rc == -4                                                      # GSM_E_UNSUPPORTED
                with pytest.raises(_lib.GsmError, match="vtype"):
                    eng._check(rc)
                rc = eng.lib.gsm_krige_grid_local(eng.h, ptr(d_grid), ptr(d_cells), int(cells.size), ptr(d_xs), ptr(d_ys), ptr(d_local),
                                                  vtype, 6, 3000.0, 16, ptr(d_est), ptr(d_var), ptr(d_n), eng._stream())
                assert rc == -4
                with pytest.raises(_lib.GsmError, match="vtype"):
                    eng._check(rc)
        assert torch.equal(torch.isnan(d_grid), torch.isnan(before))                 # nothing ran
    finally:
        eng.close()
