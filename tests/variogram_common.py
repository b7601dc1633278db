"""NumPy checker of mcmc_gpu_amd.variogram, independent of the offset formulation: brute force over ALL pairs of cells, the
separation of a pair taken from the cells' coordinates (np.hypot of the coordinate differences), sums with math.fsum.  From the
same pair list it also makes the offset map that gsm_variogram_map returns.  Shared by tests/test_variogram_host.py (CPU) and
tests/test_gpu_variogram.py; the cases and their inputs are made once per process."""
import functools
import math

import numpy as np

U = 2.0 ** -53

# tag: (H, W, dx, dy, maxlag, n_lags, R) -- what each exercises is in tests/test_gpu_variogram.py
CASES = {
    "base": (24, 20, 500.0, 500.0, 4300.0, 7, 3),
    "wide": (17, 70, 500.0, -500.0, 6100.0, 9, 3),
    "rect": (21, 19, 400.0, -650.0, 5100.0, 8, 3),
    "far": (9, 13, 500.0, 500.0, 20e3, 6, 3),
    "cols": (12, 150, 500.0, 500.0, 3300.0, 5, 2),
    "tiles": (12, 150, 500.0, 500.0, 35200.0, 7, 2),
    "shift": (4, 260, 500.0, 500.0, 104900.0, 7, 2),
}


def grid_of(H, W, dx, dy, x0=1000.0, y0=-2000.0):
    return np.meshgrid(x0 + dx * np.arange(W), y0 + dy * np.arange(H))


@functools.lru_cache(maxsize=None)
def case(tag):
    """(xx, yy, fields [R, H, W], maxlag, n_lags): values N(300, 50), 30 % of the cells NaN, drawn independently per field."""
    H, W, dx, dy, maxlag, n_lags, R = CASES[tag]
    rng = np.random.default_rng(sorted(CASES).index(tag) + 77)
    xx, yy = grid_of(H, W, dx, dy)
    f = rng.normal(300.0, 50.0, (R, H, W))
    f[rng.random((R, H, W)) < 0.3] = np.nan
    for a in (xx, yy, f):
        a.setflags(write=False)
    return xx, yy, f, maxlag, n_lags


def edges_of(maxlag, n_lags):
    return np.linspace(0.0, maxlag, n_lags + 1)[1:]


def assert_edge_margin(xx, yy, maxlag, edges):
    """No offset of the grid lies within 1e-6 * maxlag of a bin edge: then the coordinate-based checker and the offset-based
    product cannot put a pair into different bins for reasons that are not bugs."""
    H, W = xx.shape
    dx, dy = xx[0, 1] - xx[0, 0], yy[1, 0] - yy[0, 0]
    d = np.hypot(np.arange(W)[None, :] * dx, np.arange(H)[:, None] * dy).ravel()
    gap = np.abs(d[:, None] - np.asarray(edges)[None, :]).min()
    assert gap > 1e-6 * maxlag, gap


def _pairs(xx, yy, z, mask):
    """Every unordered pair (p, q), p < q in row-major order, of cells that hold a value: index arrays and squared difference."""
    ok = np.isfinite(z)
    if mask is not None:
        ok &= np.asarray(mask) != 0
    cells = np.flatnonzero(ok.ravel())
    p, q = np.triu_indices(cells.size, k=1)
    p, q = cells[p], cells[q]
    zf = z.ravel()
    d = zf[p] - zf[q]
    return p, q, d * d


def _direction_ok(hx, hy, azimuth, tolerance):
    ang = np.degrees(np.arctan2(hy, hx)) - azimuth
    ang = ang - 180.0 * np.round(ang / 180.0)                 # to (-90, 90]: directions modulo 180 degrees
    return np.abs(ang) <= tolerance


def experimental(xx, yy, z, edges, azimuth=None, tolerance=22.5, mask=None):
    """All-pairs experimental variogram of one field: (gamma [n], counts [n]); bin k holds edges[k-1] < dist <= edges[k]."""
    p, q, sq = _pairs(xx, yy, z, mask)
    xf, yf = xx.ravel(), yy.ravel()
    hx, hy = xf[q] - xf[p], yf[q] - yf[p]
    dist = np.hypot(hx, hy)
    keep = np.ones(dist.size, bool) if azimuth is None else _direction_ok(hx, hy, azimuth, tolerance)
    lo = np.concatenate([[0.0], edges[:-1]])
    gamma, counts = np.full(len(edges), np.nan), np.zeros(len(edges), dtype=np.int64)
    for k in range(len(edges)):
        sel = keep & (dist > lo[k]) & (dist <= edges[k])
        counts[k] = int(sel.sum())
        if counts[k]:
            gamma[k] = math.fsum(sq[sel]) / (2.0 * counts[k])
    return gamma, counts


def offset_map(z, mi, mj, mask=None):
    """The variogram map of one field from the all-pairs list: (sum, count) [mi + 1, 2 mj + 1].  With p < q in row-major order
    the row offset is >= 0 and a pair of one row has a positive column offset: the half plane of the product, (0, dj <= 0) empty."""
    H, W = z.shape
    p, q, sq = _pairs(None, None, z, mask)
    di, dj = q // W - p // W, q % W - p % W
    s, c = np.zeros((mi + 1, 2 * mj + 1)), np.zeros((mi + 1, 2 * mj + 1), dtype=np.int64)
    keep = (di <= mi) & (np.abs(dj) <= mj)
    key = di[keep] * (2 * mj + 1) + dj[keep] + mj
    order = np.argsort(key, kind="stable")
    key, sq = key[order], sq[keep][order]
    cuts = np.flatnonzero(np.diff(key)) + 1
    for k, terms in zip(key[np.concatenate([[0], cuts])] if key.size else [], np.split(sq, cuts)):
        s.ravel()[k] = math.fsum(terms)
        c.ravel()[k] = terms.size
    return s, c


@functools.lru_cache(maxsize=None)
def reference(tag):
    """Per field of a case: the all-pairs isotropic variogram and the offset map at the product's extents."""
    from mcmc_gpu_amd import variogram
    xx, yy, f, maxlag, n_lags = case(tag)
    H, W, dx, dy = CASES[tag][:4]
    edges = edges_of(maxlag, n_lags)
    mi, mj = variogram.offset_extents(H, W, dx, dy, maxlag)
    iso = [experimental(xx, yy, z, edges) for z in f]
    maps = [offset_map(z, mi, mj) for z in f]
    return (np.array([g for g, _ in iso]), np.array([c for _, c in iso]), np.array([s for s, _ in maps]), np.array([c for _, c in maps]))


def assert_within_bound(dev, ref, n):
    """|dev - exact| <= (n + 3) 2^-53 exact: n non-negative terms of three roundings each, in any order.  n: the device's count."""
    dev, ref, n = np.asarray(dev, dtype=np.float64), np.asarray(ref, dtype=np.float64), np.asarray(n)
    np.testing.assert_array_equal(np.isnan(dev), np.isnan(ref))
    ok = ~np.isnan(ref)
    err, bound = np.abs(dev[ok] - ref[ok]), (n[ok] + 3) * U * ref[ok]
    print("worst error / bound:", float(np.max(err / np.where(bound > 0, bound, 1.0), initial=0.0)))
    assert np.all(err <= bound), (err.max(), bound.min())
