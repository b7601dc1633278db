"""GPU: mcmc_gpu_amd.interpolate (gsm_sgs_grid, csrc/sgs_grid_kernel.hip) against golden F14 -- the unmodified reference's
interpolate.sgs (scripts/make_fixtures_interp_sgs.py) -- with the block path's tolerances (test_gpu_sgs.py), and at size."""
import json
from pathlib import Path

import numpy as np
import pytest

import interp_sgs_common as ic

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"


def _case(tag):
    xx, yy, grid, cases = (ic.t2_like() if tag == "d" else ic.small())
    vario, kw, seeds = cases[tag]
    return xx, yy, grid, vario, kw, seeds, np.load(GOLD / f"f14{tag}_interp_sgs.npz", allow_pickle=False)


def _plan(xx, yy, grid, vario, kw):
    from mcmc_gpu_amd import interpolate
    return interpolate._Plan(xx, yy, grid, vario, kw["radius"], kw["num_points"], kw["ktype"], kw.get("sim_mask"), None, None,
                             kw.get("bounds"))


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_interpolate_sgs_equals_reference_trace(tag):
    from mcmc_gpu_amd import interpolate
    xx, yy, grid, vario, kw, seeds, g = _case(tag)
    plan = _plan(xx, yy, grid, vario, kw)
    rngs = [np.random.default_rng(s) for s in seeds]
    ns, (paths, tr) = interpolate._run(plan, rngs, trace=True)
    sim = interpolate._inverse(plan, ns)
    off = np.concatenate([[0], np.cumsum([p.size for p in paths])])
    cond = ~np.isnan(grid)
    span = float(np.nanmax(grid) - np.nanmin(grid))
    for r, s in enumerate(seeds):
        assert json.loads(str(g[f"{s}_state"])) == rngs[r].bit_generator.state
        np.testing.assert_array_equal(paths[r], g[f"{s}_cells"])
        t = tr[off[r]:off[r + 1]]
        solved = t[:, 0] >= 0                                            # cells whose bounds coincide solve no system here
        if plan.bounds is not None:
            lo, hi = plan.bounds
            np.testing.assert_array_equal(~solved, (lo.ravel() == hi.ravel())[paths[r]])
        ref_n, ref_ev = g[f"{s}_n"].astype(np.float64), g[f"{s}_est_var"]
        np.testing.assert_array_equal(t[solved, 0], ref_n[solved])                                   # neighbour counts
        np.testing.assert_allclose(t[solved, 1], ref_ev[solved, 0], rtol=1e-9, atol=1e-12)           # kriging estimates
        np.testing.assert_allclose(t[solved, 2], ref_ev[solved, 1], rtol=1e-7, atol=1e-9 * vario["sill"])
        ref_ns = g[f"{s}_ns"]
        np.testing.assert_array_equal(np.isnan(ns[r]), np.isnan(ref_ns))
        np.testing.assert_allclose(ns[r], ref_ns, rtol=0, atol=1e-8, equal_nan=True)                # normal scores
        np.testing.assert_allclose(sim[r], g[f"{s}_sim"], rtol=0, atol=1e-6 * span, equal_nan=True)  # returned maps
        assert np.array_equal(ns[r][cond], ref_ns[cond]) and np.array_equal(sim[r][cond], g[f"{s}_sim"][cond])
        if plan.bounds is not None:
            deg = (plan.bounds[0] == plan.bounds[1]) & ~np.isnan(ref_ns) & ~cond
            assert deg.any() or tag == "c"
            assert np.array_equal(sim[r][deg], g[f"{s}_sim"][deg])


def test_t2_like_case_equals_reference_outputs():
    from mcmc_gpu_amd import interpolate
    xx, yy, grid, vario, kw, seeds, g = _case("d")
    rng = np.random.default_rng(seeds[0])
    out = interpolate.sgs(xx, yy, grid, vario, seed=rng, **kw)
    span = float(np.nanmax(grid) - np.nanmin(grid))
    np.testing.assert_allclose(out, g[f"{seeds[0]}_sim"], rtol=0, atol=1e-6 * span)
    assert json.loads(str(g[f"{seeds[0]}_state"])) == rng.bit_generator.state


def test_sgs_many_rows_equal_single_calls_and_segments_change_nothing():
    from mcmc_gpu_amd import interpolate
    xx, yy, grid, vario, kw, _, _ = _case("b")
    g_many, g_one = np.random.default_rng(99), np.random.default_rng(99)
    many = interpolate.sgs_many(xx, yy, grid, vario, [21, g_many, 5, g_many], **kw)
    one = np.stack([interpolate.sgs(xx, yy, grid, vario, seed=s, **kw) for s in (21, g_one, 5, g_one)])
    assert np.array_equal(many, one, equal_nan=True)
    assert g_many.bit_generator.state == g_one.bit_generator.state
    seg = interpolate.sgs_many(xx, yy, grid, vario, [21, 99, 5, 7], segment_cells=64, **kw)
    auto = interpolate.sgs_many(xx, yy, grid, vario, [21, 99, 5, 7], **kw)
    assert np.array_equal(seg, auto, equal_nan=True) and np.array_equal(seg[0], many[0], equal_nan=True)


def test_truncated_draw_outside_scipys_domain_raises():
    from mcmc_gpu_amd import interpolate, _lib
    xx, yy, grid, vario, kw, _, _ = _case("b")
    lower = np.full(grid.shape, np.nanquantile(grid, 0.6))
    upper = np.full(grid.shape, np.nanquantile(grid, 0.4))                 # upper < lower inside the data range: a >= b
    with pytest.raises(_lib.GsmError, match="truncated-normal"):
        interpolate.sgs(xx, yy, grid, vario, seed=1, **{**kw, "bounds": (lower, upper)})


def test_whole_grid_at_size_with_bounds():
    """256 x 256 cells x 16 realisations, 48 neighbours within 30 km at 500 m, bounds on -- far beyond the 1024-cell window of
    mcmc_gpu_amd.sgs.sgs."""
    from mcmc_gpu_amd import interpolate
    H = W = 256
    xx, yy = np.meshgrid(np.arange(W) * 500.0, np.arange(H) * 500.0)
    bed = ic.field(H, W, 5)
    cond = np.zeros((H, W), bool)
    cond[::12, :] = True
    cond[:, ::20] = True
    cond[100:160, 60:140] = False                                          # a 30 x 40 km hole
    grid = np.where(cond, bed, np.nan)
    lower = float(np.nanmin(grid)) - 50.0
    upper = bed + 300.0 * (1.0 + 0.5 * np.sin(xx / 20e3))
    vario = dict(major_range=20e3, minor_range=20e3, azimuth=0.0, sill=1.0, nugget=0.0, vtype="Matern", s=1.5)
    out = interpolate.sgs_many(xx, yy, grid, vario, list(range(16)), radius=30e3, num_points=48, bounds=(lower, upper))
    assert out.shape == (16, H, W)
    assert not np.isnan(out).any()
    plan = _plan(xx, yy, grid, vario, dict(radius=30e3, num_points=48, ktype="ok", bounds=(lower, upper)))
    assert np.all(out[:, cond] == interpolate._inverse(plan, plan.grid_ns)[cond])    # conditioning cells: the reference's round trip
    ns = plan.nst.transform(out.reshape(-1, 1)).reshape(out.shape)
    lo, hi = plan.bounds
    assert np.all(out <= np.maximum(upper, np.nanmax(grid)) + 1e-6 * float(np.nanmax(grid) - np.nanmin(grid)))
    assert np.all(ns >= lo - 1e-6) and np.all(ns <= hi + 1e-6)
    assert np.std(out[:, ~cond], axis=0).mean() > 0.0                       # the realisations differ
