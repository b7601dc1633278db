"""Cases of the kriging cross-validation tests (tests/test_krige_cv_host.py, tests/test_gpu_krige_cv.py) and a CPU restatement of
a hold-out built only from what the tests already have: the hold-out of target t is a copy of the grid with NaN at t and at
every cell the predicate excludes, handed to krige_common.krige_scores_cpu with the device's tie rule.

The predicate of gsm_krige_cv (include/gsm.h): cell c conditions target t when it holds a value, is not t, is not of t's fold
(t in a fold at all: label >= 0), and is farther from t than exclude_radius (where that is > 0)."""
import functools

import numpy as np

import interp_sgs_common as ic
import krige_common as kc

EXP = dict(major_range=8000.0, minor_range=5000.0, azimuth=30.0, sill=1.0, nugget=0.0, vtype="Exponential")
# four tables for one call (exponential, gaussian, spherical, Matern) and the three models of the per-cell form.  The gaussian
# range is three cells: the reference's gaussian model has no nugget on the diagonal, longer ranges give near-singular systems
MODELS = [
    dict(major_range=6000.0, minor_range=4000.0, azimuth=20.0, sill=1.0, nugget=0.0, vtype="Exponential"),
    dict(major_range=1500.0, minor_range=1500.0, azimuth=0.0, sill=0.9, nugget=0.0, vtype="Gaussian"),
    dict(major_range=7000.0, minor_range=7000.0, azimuth=0.0, sill=1.1, nugget=0.0, vtype="Spherical"),
    dict(major_range=6000.0, minor_range=6000.0, azimuth=0.0, sill=1.0, nugget=0.0, vtype="Matern", s=1.5),
]


def lines_grid(seed=41):
    """40 x 36 square cells of 500 m with data on every 6th row (lines) and on ~5 % of the other cells: the smallest layout in
    which line neighbours dominate, a buffer of 2-3 cells changes the neighbour set of most targets, and a block fold empties
    whole octants."""
    H, W = 40, 36
    xx, yy = ic._mesh(H, W, 500.0, 500.0)
    cond = np.zeros((H, W), bool)
    cond[::6, :] = True
    cond |= np.random.default_rng(seed).random((H, W)) < 0.05
    return xx, yy, np.where(cond, ic.field(H, W, seed), np.nan)


@functools.lru_cache(maxsize=None)
def cases():
    """id -> dict(xx, yy, grid, vario, kw, ex).  The geometry grids of test_gpu_krige.py (square cells with descending y, both
    axes descending, descending x, rows half and twice as far apart as the columns) and the lines grid.  ex: the exclusion radius
    of the case's buffered hold-out, 2.5 columns, or 2.6 where 2.5 is a lattice distance of the grid (rows half as far apart:
    5 rows)."""
    g = ic.geometry()
    out = {}
    for cid, ex in (("G1", 1250.0), ("G2", 1250.0), ("G8", 1250.0), ("G3", 1300.0), ("G4", 1250.0)):
        xx, yy, grid, vario, kw, _ = g[cid]
        kw = {k: v for k, v in kw.items() if k in ("radius", "num_points", "ktype")}
        out[cid] = dict(xx=xx, yy=yy, grid=grid, vario=vario, kw=kw, ex=ex)
    xx, yy, grid = lines_grid()
    out["L"] = dict(xx=xx, yy=yy, grid=grid, vario=EXP, kw=dict(radius=3000.0, num_points=16, ktype="ok"), ex=1250.0)
    return out


def lattice_distances(xs, ys):
    """Every distance between two cells of the grid, sorted (the distinct values of sqrt((m dx)^2 + (n dy)^2))."""
    dx, dy = abs(xs[1] - xs[0]), abs(ys[1] - ys[0])
    m, n = np.meshgrid(np.arange(xs.size) * dx, np.arange(ys.size) * dy)
    return np.unique(np.sqrt(m * m + n * n))


def no_tie(xs, ys, ex, rel=1e-9):
    """True when no lattice distance of the grid lies within `rel` relative of ex: `d <= ex` then has one answer whether or not
    dx dx + dy dy is contracted into a fused multiply-add or the coordinates carry rounding."""
    d = lattice_distances(np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64))
    return bool(np.all(np.abs(d - ex) > rel * ex))


def excluded(xs, ys, cond, t, fold=None, ex=0.0):
    """bool [H, W]: the cells the hold-out of target t (flat index) takes away, t itself included.  The distance is the
    kernel's expression, sqrt((x0 - xs[j])^2 + (y0 - ys[i])^2)."""
    H, W = cond.shape
    i0, j0 = divmod(int(t), W)
    out = np.zeros((H, W), bool)
    out[i0, j0] = True
    if fold is not None and fold.reshape(H, W)[i0, j0] >= 0:
        out |= fold.reshape(H, W) == fold.reshape(H, W)[i0, j0]
    if ex > 0:
        ddx, ddy = xs[j0] - xs[None, :], ys[i0] - ys[:, None]
        out |= np.sqrt(ddx * ddx + ddy * ddy) <= ex
    return out


def held_out(grid_ns, xs, ys, t, fold=None, ex=0.0):
    """A copy of grid_ns with NaN at every cell excluded(...) names."""
    g = grid_ns.copy()
    g[excluded(xs, ys, ~np.isnan(grid_ns), t, fold, ex)] = np.nan
    return g


def cv_cpu(xx, yy, grid_ns, vario, kw, targets, fold=None, ex=0.0):
    """(n, est, var) per target from krige_scores_cpu on the target's own held-out copy of the grid.  Ordinary kriging only:
    the helper takes the global mean of simple kriging from the grid it is given, the device from all data."""
    assert kw["ktype"] == "ok"
    xs, ys = xx[0, :], yy[:, 0]
    rows = []
    for t in targets:
        _, _, tr, _ = kc.krige_scores_cpu(xx, yy, held_out(grid_ns, xs, ys, t, fold, ex), dict(vario), kw["radius"], kw["num_points"],
                                          kw["ktype"], stable_ties=True, cells=[int(t)])
        rows.append(tr[0, 2:5])
    rows = np.array(rows).reshape(-1, 3)
    return rows[:, 0].astype(np.int32), rows[:, 1], rows[:, 2]


def pick_targets(cond, count=40):
    """About `count` data cells (flat indices, ascending), chosen by rule: the grid's corners and border cells that hold data,
    cells with fewer than two data cells among their four neighbours (off the lines, or at a line's end next to the empty
    region), and every k-th of the rest."""
    H, W = cond.shape
    flat = np.flatnonzero(cond)
    i, j = flat // W, flat % W
    pad = np.pad(cond, 1)
    nb = (pad[:-2, 1:-1].astype(int) + pad[2:, 1:-1] + pad[1:-1, :-2] + pad[1:-1, 2:])[cond]
    corner = ((i == 0) | (i == H - 1)) & ((j == 0) | (j == W - 1))
    border = (i == 0) | (i == H - 1) | (j == 0) | (j == W - 1)
    chosen = list(flat[corner]) + list(flat[border & ~corner][::7]) + list(flat[(nb < 2) & ~border][:12])
    rest = np.setdiff1d(flat, chosen)
    chosen += list(rest[::max(1, rest.size // max(1, count - len(chosen)))])
    return np.unique(np.array(chosen, dtype=np.int32))[:count + 8]


# ---- interpolate.cross_validate end to end ------------------------------------------------------------------------------------------
E2E_TRUE = dict(major_range=5000.0, minor_range=5000.0, azimuth=0.0, sill=1.0, nugget=0.0, vtype="Exponential")
E2E_WRONG = dict(E2E_TRUE, major_range=500.0, minor_range=500.0)                      # the range tenfold too short
E2E_KW = dict(radius=5000.0, num_points=16, ktype="ok")
# Seeds 1 .. 6 all show both orderings in the CPU restatement (test_krige_cv_host.py asserts them for this one); seed 2 by the
# widest margins: RMSE 0.560 (true model, leave-one-out), 0.761 (range tenfold short), 0.854 (true model, 2.5-cell buffer)
E2E_SEED = 2
E2E_EX = 1250.0


def cpu_sgs(xx, yy, grid, vario, seed=None, **kw):
    """interpolate.sgs restated with the CPU oracle: the package's transformer around sgs_oracle.sgs with the device's tie rule."""
    import sgs_oracle as so
    from mcmc_gpu_amd import interpolate
    plan = kc.plan_of(xx, yy, grid, vario, kw)
    so.STABLE_TIES = True
    try:
        out = so.sgs(xx, yy, plan.grid_ns, dict(vario), kw["radius"], kw["num_points"], kw["ktype"], rng=np.random.default_rng(seed))
    finally:
        so.STABLE_TIES = False
    return interpolate._inverse(plan, out)


def e2e_data(simulate, seed=E2E_SEED):
    """(xx, yy, grid): a field simulated from E2E_TRUE -- simulate(xx, yy, grid0, variogram, seed=..., **E2E_KW) is
    interpolate.sgs, or the CPU oracle's restatement of it -- around 30 scattered values, and sampled on the layout of
    lines_grid (lines six rows apart and ~5 % scattered cells)."""
    xx, yy, layout = lines_grid()
    H, W = layout.shape
    r = np.random.default_rng(1000 + seed)
    grid0 = np.full((H, W), np.nan)
    at = r.choice(H * W, 30, replace=False)
    grid0.ravel()[at] = -400.0 + 100.0 * r.standard_normal(30)
    truth = simulate(xx, yy, grid0, dict(E2E_TRUE), seed=seed, **E2E_KW)
    return xx, yy, np.where(np.isnan(layout), np.nan, truth)
