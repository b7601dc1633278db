"""Non-stationary interpolate.sgs / interpolate.krige: every variogram parameter a map of the grid's shape (the reference's
local_vario, gstatsMCMC/gstatsim_custom/interpolate.py:56-62, :141-147).

Inputs of goldens F16 (scripts/make_fixtures_nonstationary.py: interpolate.sgs) and F17 (the same script: interpolate.krige),
rebuilt here so that the fixture files hold outputs only, and the CPU restatement of both cell loops with a variogram per cell,
assembled from oracle/sgs_oracle.py (neighbors, make_circle_stencil, ok_solve, sk_solve) exactly as oracle/sgs_oracle.sgs and
tests/krige_common.krige_scores_cpu assemble the stationary ones.  tests/test_nonstationary_host.py pins the restatement bit
for bit to the fixtures; tests/test_gpu_nonstationary.py compares the device with it on the grids the fixtures leave out."""
import warnings

import numpy as np

import interp_sgs_common as ic
import sgs_oracle as so

def fields(H, W, range_scale=1.0):
    """Smooth parameter maps, i = row, j = column: ranges of 5-9 km by 3-5.5 km that grow across the grid, the major axis turning
    from 10 to 130 degrees, sill 0.8-1.2, nugget 0.02-0.07."""
    i, j = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return dict(major_range=(5000 + 4000 * j / (W - 1) + 7.3 * i) * range_scale,
                minor_range=(3000 + 2500 * i / (H - 1) + 3.1 * j) * range_scale,
                azimuth=10 + 120 * (i + 2 * j) / (H + 2 * W),
                sill=0.8 + 0.4 * j / (W - 1),
                nugget=0.02 + 0.05 * i / (H - 1))


def vario_of(H, W, vtype, range_scale=1.0):
    return dict(fields(H, W, range_scale), vtype=vtype)


def small():
    """interp_sgs_common.small()'s 40 x 44 tie-free grid (a data gap wider than the radius: the search widens) under the
    parameter maps.  tag -> (variogram, keyword arguments, seeds):
        a  exponential, ordinary kriging, 16 points, two seeds
        b  spherical, ordinary kriging, 24 points, small()'s bounds (truncated draws, lower == upper cells)
        c  gaussian, simple kriging, 8 points, a sim_mask, ranges x 0.25 (the reference's gaussian model puts no nugget on the
           diagonal: at the full ranges its systems are near singular and lstsq's answer is no reference)"""
    xx, yy, grid, cases = ic.small()
    H, W = grid.shape
    kw_b, kw_c = cases["b"][1], cases["c"][1]
    return xx, yy, grid, {
        "a": (vario_of(H, W, "Exponential"), dict(radius=3000.0, num_points=16, ktype="ok"), [11, 12]),
        "b": (vario_of(H, W, "Spherical"), dict(radius=3000.0, num_points=24, ktype="ok", bounds=kw_b["bounds"]), [21]),
        "c": (vario_of(H, W, "Gaussian", 0.25), dict(radius=4000.0, num_points=8, ktype="sk", sim_mask=kw_c["sim_mask"]), [31]),
    }


KRIGE_TAGS = ("a", "c")      # golden F17: interpolate.krige on cases a and c of small() (bounds: krige has none)


def geometry():
    """Four grids of interp_sgs_common.geometry() under the parameter maps (computed for each grid's own H and W), for the
    device against the CPU restatement.  id -> (xx, yy, grid, variogram, keyword arguments, seeds):
        G1  y descending, square cells (distance ties), bounds: the sign of dy under a rotated R
        G3  48 points, rows 250 m apart
        G4  20 points, rows 1000 m apart, y descending; spherical, simple kriging
        G5  data in one corner of a 240 km grid: systems of one neighbour, two widenings; simple kriging.  Cells of 5 km, ten
            times the others': the ranges are multiplied by ten so that they span as many cells as elsewhere
    No gaussian model: see small()."""
    g = ic.geometry()
    out = {}
    for cid, vtype, ktype, scale in (("G1", "Exponential", "ok", 1.0), ("G3", "Exponential", "ok", 1.0),
                                     ("G4", "Spherical", "sk", 1.0), ("G5", "Exponential", "sk", 10.0)):
        xx, yy, grid, _, kw, seeds = g[cid]
        out[cid] = (xx, yy, grid, vario_of(*grid.shape, vtype, scale), dict(kw, ktype=ktype), seeds[:2] if cid == "G1" else seeds[:1])
    return out


def plan_of(xx, yy, grid, vario, kw, bounds=True):
    from mcmc_gpu_amd import interpolate
    return interpolate._Plan(xx, yy, grid, vario, kw["radius"], kw["num_points"], kw["ktype"], kw.get("sim_mask"), None, None,
                             kw.get("bounds") if bounds else None)


def local_vario(vario, i, j):
    """interpolate.py:142-147."""
    return {k: (v if k == "vtype" else v[i, j]) for k, v in vario.items()}


def _search(i, j, ii, jj, xx, yy, out_grid, cond_msk, radius, num_points, stencil):
    """The neighbour search with the reference's radius widening (interpolate.py:150-157).  Returns (neighbours, radius reached)."""
    nearest, rad, stenc = np.array([]), radius, stencil
    while nearest.shape[0] == 0:
        nearest = so.neighbors(i, j, ii, jj, xx, yy, out_grid, cond_msk, rad, num_points, stencil=stenc)
        if nearest.shape[0] > 0:
            break
        rad += 100e3
        stenc, _, _ = so.make_circle_stencil(xx[0, :], rad)
    return nearest, rad


def sgs_local(xx, yy, grid, vario, radius, num_points, ktype, sim_mask=None, rng=None, trace=None, bounds=None, stable_ties=False):
    """oracle/sgs_oracle.sgs with a variogram per cell: `vario` holds a map of the grid's shape for every parameter.  `grid` and
    `bounds` in normal-score space (interpolate._Plan's grid_ns and bounds).  trace (a list) receives (i, j, n, est, |var|, radius
    reached) per simulated cell.  stable_ties: equidistant candidates in ascending (row, column), the device's rule."""
    if bounds is not None:
        from scipy.stats import truncnorm
        lower, upper = bounds
    cond_msk = ~np.isnan(grid)
    out_grid = grid.copy()
    if sim_mask is None:
        sim_mask = np.full(xx.shape, True)
    ii, jj = np.meshgrid(np.arange(xx.shape[0]), np.arange(xx.shape[1]), indexing="ij")
    inds = np.array([ii[sim_mask].flatten(), jj[sim_mask].flatten()]).T
    global_mean = np.mean(out_grid[cond_msk])
    stencil, _, _ = so.make_circle_stencil(xx[0, :], radius)
    rng.shuffle(inds)
    saved = so.STABLE_TIES
    so.STABLE_TIES = bool(stable_ties)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for i, j in inds:
                if cond_msk[i, j]:
                    continue
                lv = local_vario(vario, i, j)
                nearest, rad = _search(i, j, ii, jj, xx, yy, out_grid, cond_msk, radius, num_points, stencil)
                if ktype == "ok":
                    est, var = so.ok_solve((xx[i, j], yy[i, j]), nearest, lv, None)
                else:
                    est, var = so.sk_solve((xx[i, j], yy[i, j]), nearest, lv, global_mean, None)
                var = np.abs(var)
                if bounds is None:
                    out_grid[i, j] = rng.normal(est, np.sqrt(var), 1)[0]
                elif lower[i, j] == upper[i, j]:
                    out_grid[i, j] = lower[i, j]
                else:
                    sd = np.sqrt(var)
                    out_grid[i, j] = truncnorm.rvs((lower[i, j] - est) / sd, (upper[i, j] - est) / sd, loc=est, scale=sd, size=1,
                                                   random_state=rng)[0]
                cond_msk[i, j] = True
                if trace is not None:
                    trace.append((int(i), int(j), int(nearest.shape[0]), float(est), float(var), float(rad)))
    finally:
        so.STABLE_TIES = saved
    return out_grid


def krige_local(xx, yy, grid, vario, radius, num_points, ktype, sim_mask=None, stable_ties=False):
    """tests/krige_common.krige_scores_cpu with a variogram per cell.  Returns (est_ns [H, W], var [H, W] unclipped,
    trace [cells, (i, j, n, est, var)])."""
    cond_msk = ~np.isnan(grid)
    out_grid = grid.copy()
    var_grid = np.zeros(grid.shape)
    if sim_mask is None:
        sim_mask = np.full(xx.shape, True)
    ii, jj = np.meshgrid(np.arange(xx.shape[0]), np.arange(xx.shape[1]), indexing="ij")
    inds = np.array([ii[sim_mask].flatten(), jj[sim_mask].flatten()]).T
    global_mean = np.mean(out_grid[cond_msk])
    stencil, _, _ = so.make_circle_stencil(xx[0, :], radius)
    trace = []
    saved = so.STABLE_TIES
    so.STABLE_TIES = bool(stable_ties)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for i, j in inds:
                if cond_msk[i, j]:
                    continue
                lv = local_vario(vario, i, j)
                nearest, _ = _search(i, j, ii, jj, xx, yy, out_grid, cond_msk, radius, num_points, stencil)
                if ktype == "ok":
                    est, var = so.ok_solve((xx[i, j], yy[i, j]), nearest, lv)
                else:
                    est, var = so.sk_solve((xx[i, j], yy[i, j]), nearest, lv, global_mean)
                out_grid[i, j] = est                                         # cond_msk stays: later cells never see it
                var_grid[i, j] = var
                trace.append((int(i), int(j), int(nearest.shape[0]), float(est), float(var)))
    finally:
        so.STABLE_TIES = saved
    return out_grid, var_grid, np.array(trace, dtype=np.float64).reshape(-1, 5)
