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
