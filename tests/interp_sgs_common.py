"""Inputs of golden F14 (scripts/make_fixtures_interp_sgs.py): synthetic tie-free grids for interpolate.sgs, rebuilt here so that
the fixture files hold outputs only."""
import numpy as np

from sgs_common import TIE_FREE_DY


def field(H, W, seed):
    """A smooth synthetic bed (m) on an H x W grid."""
    r = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    f = np.zeros((H, W))
    for _ in range(6):
        kx, ky, ph, a = r.uniform(0.02, 0.15), r.uniform(0.02, 0.15), r.uniform(0, 2 * np.pi), r.uniform(50, 150)
        f += a * np.sin(kx * j + ky * i + ph)
    return f - 400.0 + r.normal(0.0, 5.0, (H, W))


def small():
    """Cases a-c: 40 x 44 cells, conditioning lines with a gap of ~13 x 15 km (wider than the radius: the search widens)."""
    H, W = 40, 44
    xx, yy = np.meshgrid(np.arange(W) * 500.0, np.arange(H) * TIE_FREE_DY)
    cond = np.zeros((H, W), bool)
    cond[::5, :] = True
    cond[:, ::7] = True
    cond[8:34, 10:40] = False
    grid = np.where(cond, field(H, W, 14), np.nan)
    lo = float(np.nanmin(grid)) - 25.0                    # below the data: transforms to the lowest score
    up = np.full((H, W), float(np.nanmax(grid)) + 50.0)
    up[:, :W // 3] = np.nanquantile(grid, 0.7)            # binds where the estimate is high
    up[30:36, 2:9] = lo - 10.0                            # below the data too: lower == upper in score space
    sim_mask = np.zeros((H, W), bool)
    sim_mask[4:36, 6:40] = True
    cases = {
        "a": (dict(major_range=6000.0, minor_range=6000.0, azimuth=0.0, sill=1.0, nugget=0.0, vtype="Matern", s=1.5),
              dict(radius=3000.0, num_points=16, ktype="ok"), [11, 12]),
        "b": (dict(major_range=8000.0, minor_range=5000.0, azimuth=30.0, sill=1.0, nugget=0.0, vtype="Exponential"),
              dict(radius=3000.0, num_points=24, ktype="ok", bounds=(lo, up)), [21, 22]),
        "c": (dict(major_range=7000.0, minor_range=7000.0, azimuth=0.0, sill=1.0, nugget=0.0, vtype="Spherical"),
              dict(radius=4000.0, num_points=16, ktype="sk", sim_mask=sim_mask, bounds=(lo, up)), [31]),
    }
    return xx, yy, grid, cases


def t2_like():
    """Case d: 96 x 96 cells, 48 neighbours within 10 km, bounds as T2_StatisticalAnalysis.ipynb sets them (a floor below the
    data, a surface map above it)."""
    H = W = 96
    xx, yy = np.meshgrid(np.arange(W) * 500.0, np.arange(H) * TIE_FREE_DY)
    bed = field(H, W, 15)
    cond = np.zeros((H, W), bool)
    cond[::6, :] = True
    cond[:, ::9] = True
    grid = np.where(cond, bed, np.nan)
    surf = bed + 600.0 + 50.0 * np.cos(xx / 9000.0)
    vario = dict(major_range=15000.0, minor_range=15000.0, azimuth=0.0, sill=1.0, nugget=0.0, vtype="Matern", s=1.5)
    kw = dict(radius=10e3, num_points=48, ktype="ok", bounds=(float(np.nanmin(grid)) - 100.0, surf))
    return xx, yy, grid, {"d": (vario, kw, [41])}


def _lines(H, W, a, b):
    cond = np.zeros((H, W), bool)
    cond[::a, :] = True
    cond[:, ::b] = True
    return cond


def _mesh(H, W, dx, dy, x_desc=False, y_desc=False):
    x, y = np.arange(W) * dx, np.arange(H) * dy
    return np.meshgrid(x[::-1].copy() if x_desc else x, y[::-1].copy() if y_desc else y)


def geometry():
    """Grids golden F14 leaves out, for tests against the CPU oracle (test_gpu_interp_sgs_geometry.py): square cells (distance
    ties everywhere), descending axes (north-up rasters), cells far from square, several widenings of the radius, the
    reference's default arguments (a 200-ring window), num_points that is no multiple of 8, a window that clips the rows
    before the radius does.  id -> (xx, yy, grid, variogram, keyword arguments, seeds); seed 5 is the realisation on which
    each case's reason for being here is asserted."""
    exp_aniso = dict(major_range=8000.0, minor_range=5000.0, azimuth=30.0, sill=1.0, nugget=0.0, vtype="Exponential")
    matern = dict(major_range=6000.0, minor_range=6000.0, azimuth=0.0, sill=1.0, nugget=0.0, vtype="Matern", s=1.5)
    exp_far = dict(major_range=60e3, minor_range=60e3, azimuth=0.0, sill=1.0, nugget=0.0, vtype="Exponential")
    out = {}
    # G1, G2, G8: F14's 40 x 44 layout (conditioning lines with a gap wider than the radius) on square cells
    H, W = 40, 44
    cond = _lines(H, W, 5, 7)
    cond[8:34, 10:40] = False
    grid = np.where(cond, field(H, W, 21), np.nan)
    lo = float(np.nanmin(grid)) - 25.0                    # the bounds of small()'s case b
    up = np.full((H, W), float(np.nanmax(grid)) + 50.0)
    up[:, :W // 3] = np.nanquantile(grid, 0.7)
    up[30:36, 2:9] = lo - 10.0
    sim_mask = np.zeros((H, W), bool)
    sim_mask[4:36, 6:40] = True
    out["G1"] = (*_mesh(H, W, 500.0, 500.0, y_desc=True), grid, exp_aniso,
                 dict(radius=3000.0, num_points=24, ktype="ok", bounds=(lo, up)), [5, 6, 7])
    out["G2"] = (*_mesh(H, W, 500.0, 500.0, x_desc=True, y_desc=True), grid, matern,
                 dict(radius=3000.0, num_points=16, ktype="sk", sim_mask=sim_mask), [5, 6])
    out["G8"] = (*_mesh(H, W, 500.0, 500.0, x_desc=True), grid,
                 dict(major_range=7000.0, minor_range=7000.0, azimuth=0.0, sill=1.0, nugget=0.0, vtype="Spherical"),
                 dict(radius=4000.0, num_points=8, ktype="ok"), [5, 6])
    # G3: rows half as far apart as columns -- the +-hw-cell window ends at 1.5 km in y, the radius at 3 km
    H, W = 48, 40
    out["G3"] = (*_mesh(H, W, 500.0, 250.0), np.where(_lines(H, W, 5, 7), field(H, W, 23), np.nan), exp_aniso,
                 dict(radius=3000.0, num_points=48, ktype="ok"), [5, 6])
    # G4: rows twice as far apart as columns, y descending, 20 points = 2 per octant
    H, W = 36, 60
    out["G4"] = (*_mesh(H, W, 500.0, 1000.0, y_desc=True), np.where(_lines(H, W, 5, 7), field(H, W, 24), np.nan), matern,
                 dict(radius=4000.0, num_points=20, ktype="ok"), [5, 6])
    # G5: data in one corner of a 240 km grid, radius 10 km: up to two widenings, systems of one neighbour
    H = W = 48
    cond = np.zeros((H, W), bool)
    cond[:4, :4] = True
    out["G5"] = (*_mesh(H, W, 5000.0, 5037.0), np.where(cond, field(H, W, 25), np.nan), exp_far,
                 dict(radius=10e3, num_points=16, ktype="ok"), [5, 6, 7])
    # G6: the reference's default radius and num_points: a 200-ring window, neighbours beyond 64 rings
    H = W = 100
    cond = np.zeros((H, W), bool)
    cond[0, ::3] = True
    cond[::4, 0] = True
    out["G6"] = (*_mesh(H, W, 500.0, TIE_FREE_DY), np.where(cond, field(H, W, 26), np.nan), exp_far,
                 dict(radius=100e3, num_points=20, ktype="ok"), [5])
    # G7: data rows 4 km apart in y but 16 rows apart: inside the radius, outside the window -- searches come back empty and widen
    H, W = 97, 64
    cond = np.zeros((H, W), bool)
    cond[::16, ::3] = True
    out["G7"] = (*_mesh(H, W, 500.0, 250.0), np.where(cond, field(H, W, 27), np.nan),
                 dict(major_range=6000.0, minor_range=6000.0, azimuth=0.0, sill=1.0, nugget=0.0, vtype="Exponential"),
                 dict(radius=3000.0, num_points=16, ktype="ok"), [5, 6])
    return out


def _oracle_run(xx, yy, grid_ns, vario, kw, seed, bounds):
    """(normal scores, trace [cells, (i, j, n, est, var)], generator state) of the CPU helper with the device's tie rule."""
    import warnings
    import sgs_oracle as so
    rng = np.random.default_rng(seed)
    trace = []
    so.STABLE_TIES = True
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = so.sgs(xx, yy, grid_ns, dict(vario), kw["radius"], kw["num_points"], kw["ktype"], rng=rng, trace=trace, bounds=bounds)
    finally:
        so.STABLE_TIES = False
    return out, np.array(trace), rng.bit_generator.state


_REGIMES = None


def regimes():
    """A 24 x 24 whole-grid case whose bounded draws run through the regimes of truncnorm.h that F14 / F16 and geometry() leave
    at moderate bounds: standardised a >= 6, b <= -6 and b - a <= 1e-3 (tests/test_interp_sgs_host.py counts them in the
    helper's trace).  Tie-free spacing, 16 neighbours, conditioning lines every 6 rows and 8 columns.

    The bounds are given in normal-score space (plan.bounds is set directly) and are built from the helper's own estimates.
    The kriging variance of a cell depends on the path alone, so an unbounded run gives every sd.  A target T = that run's
    estimate + k sd, k in +-[8, 30] for two thirds of the cells, is then pinned by intervals [T, T + 1e-6 sd], and the second
    run's estimates say where T stands among them: cells with (T - est) / sd >= 7 get T as lower bound (no upper bound, or one
    1e-8 .. 1e-4 sd above), cells with <= -7 the mirror image, the others intervals of 1e-8 .. 5e-4 sd.  Every interval keeps
    its cell within a fraction of an sd of T, so the third run -- the case -- meets nearly the second one's estimates.
    Returns dict(xx, yy, grid, vario, kw, seed, plan, out, trace, state): plan with the bounds, then the helper's run."""
    global _REGIMES
    if _REGIMES is not None:
        return _REGIMES
    from mcmc_gpu_amd import interpolate
    H = W = 24
    xx, yy = np.meshgrid(np.arange(W) * 500.0, np.arange(H) * TIE_FREE_DY)
    grid = np.where(_lines(H, W, 6, 8), field(H, W, 31), np.nan)
    vario = dict(major_range=6000.0, minor_range=6000.0, azimuth=0.0, sill=1.0, nugget=0.0, vtype="Exponential")
    kw = dict(radius=3000.0, num_points=16, ktype="ok")
    seed = 5
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                 # 156 conditioning values: fewer than the transformer's 500 quantiles
        plan = interpolate._Plan(xx, yy, grid, vario, kw["radius"], kw["num_points"], kw["ktype"], None, None, None, None)
    _, tr, _ = _oracle_run(xx, yy, plan.grid_ns, vario, kw, seed, None)
    ci, cj = tr[:, 0].astype(int), tr[:, 1].astype(int)
    r = np.random.default_rng(32)
    k = np.where(r.random(ci.size) < 2 / 3, np.where(r.random(ci.size) < 0.5, 1.0, -1.0) * r.uniform(8.0, 30.0, ci.size), r.uniform(-2.0, 2.0, ci.size))
    sd = np.full((H, W), np.nan)
    T = np.full((H, W), np.nan)
    sd[ci, cj] = np.sqrt(tr[:, 4])
    T[ci, cj] = tr[:, 3] + k * sd[ci, cj]
    sim = ~np.isnan(T)
    lo, hi = np.where(sim, T, 0.0), np.where(sim, T + 1e-6 * sd, 1.0)
    _, tr, _ = _oracle_run(xx, yy, plan.grid_ns, vario, kw, seed, (lo, hi))
    assert np.array_equal(tr[:, 0], ci) and np.array_equal(tr[:, 1], cj)                  # the path does not depend on the bounds
    a2 = (T[ci, cj] - tr[:, 3]) / sd[ci, cj]
    narrow = 10.0 ** r.uniform(-8.0, -4.0, ci.size) * sd[ci, cj]
    open_end = r.random(ci.size) < 0.5
    t = T[ci, cj]
    lo_c = np.where(a2 <= -7.0, np.where(open_end, -np.inf, t - narrow), t)
    hi_c = np.where(a2 <= -7.0, t, np.where(a2 >= 7.0, np.where(open_end, np.inf, t + narrow), t + 5.0 * narrow))
    lo[ci, cj], hi[ci, cj] = lo_c, hi_c
    plan.bounds = (np.ascontiguousarray(lo), np.ascontiguousarray(hi))
    out, tr, state = _oracle_run(xx, yy, plan.grid_ns, vario, kw, seed, plan.bounds)
    _REGIMES = dict(xx=xx, yy=yy, grid=grid, vario=vario, kw=kw, seed=seed, plan=plan, out=out, trace=tr, state=state)
    return _REGIMES
