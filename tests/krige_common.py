"""CPU kriging of a whole grid in normal-score space, assembled from oracle/sgs_oracle.py (neighbors, make_circle_stencil, ok_solve,
sk_solve): the cell loop of interpolate.krige (gstatsMCMC/gstatsim_custom/interpolate.py:46-83).  Pinned bit for bit to the
reference's krige by golden F15 (scripts/make_fixtures_krige.py, tests/test_krige_host.py); tests/test_gpu_krige.py compares the
device with it on the grids F15 leaves out."""
import warnings

import numpy as np

import sgs_oracle as so


def krige_scores_cpu(xx, yy, grid_ns, vario, radius, num_points, ktype, sim_mask=None, stable_ties=False, cells=None):
    """Returns (est_ns [H, W], var [H, W] unclipped, trace [cells, (i, j, n, est, var)], radius reached per cell).  Cells: those of
    sim_mask without a value in C order, or the flat indices `cells`.  stable_ties: equidistant candidates in ascending (row,
    column), the device's rule (the reference's argsort is unstable there)."""
    H, W = grid_ns.shape
    cond_msk = ~np.isnan(grid_ns)
    out_grid = grid_ns.copy()
    var_grid = np.zeros(grid_ns.shape)
    if sim_mask is None:
        sim_mask = np.full(xx.shape, True)
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    if cells is None:
        inds = np.array([ii[sim_mask].flatten(), jj[sim_mask].flatten()]).T
    else:
        inds = np.array([np.asarray(cells) // W, np.asarray(cells) % W]).T
    global_mean = np.mean(out_grid[cond_msk])
    stencil0, _, _ = so.make_circle_stencil(xx[0, :], radius)
    trace, radii = [], []
    saved = so.STABLE_TIES
    so.STABLE_TIES = bool(stable_ties)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for i, j in inds:
                if cond_msk[i, j]:
                    continue
                nearest = np.array([])
                rad, stenc = radius, stencil0
                while nearest.shape[0] == 0:                                 # interpolate.py:65-71
                    nearest = so.neighbors(i, j, ii, jj, xx, yy, out_grid, cond_msk, rad, num_points, stencil=stenc)
                    if nearest.shape[0] > 0:
                        break
                    rad += 100e3
                    stenc, _, _ = so.make_circle_stencil(xx[0, :], rad)
                if ktype == "ok":
                    est, var = so.ok_solve((xx[i, j], yy[i, j]), nearest, vario)
                else:
                    est, var = so.sk_solve((xx[i, j], yy[i, j]), nearest, vario, global_mean)
                out_grid[i, j] = est                                         # cond_msk stays: later cells never see it
                var_grid[i, j] = var
                trace.append((int(i), int(j), int(nearest.shape[0]), float(est), float(var)))
                radii.append(float(rad))
    finally:
        so.STABLE_TIES = saved
    return out_grid, var_grid, np.array(trace, dtype=np.float64).reshape(-1, 5), np.array(radii)


def plan_of(xx, yy, grid, vario, kw):
    """interpolate._Plan of a case of interp_sgs_common (bounds dropped: krige has none)."""
    from mcmc_gpu_amd import interpolate
    return interpolate._Plan(xx, yy, grid, vario, kw["radius"], kw["num_points"], kw["ktype"], kw.get("sim_mask"), None, None, None)


def krige_kw(kw):
    return {k: v for k, v in kw.items() if k != "bounds"}
