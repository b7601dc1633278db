"""Experimental variograms of gridded fields on the device, and the model fit that closes the loop to interpolate.sgs / krige.

The reference makes its variograms with scikit-gstat from scattered points: gstatsim_custom.utilities.variograms
(utilities.py:72-113) for the `variogram` dict of interpolate.sgs, MCMC.fit_variogram (MCMC.py:257-355) for the chains, and a
variogram of final beds against the data as its check of spatial structure.  Every field of this package lives on an
axis-aligned uniform grid, where the separation of two cells is a function of their integer offset (di, dj) alone.  The device
therefore makes one small table per field -- the VARIOGRAM MAP: per offset the sum of squared differences and the number of
pairs (gsm_variogram_map, csrc/variogram_kernel.hip) -- and every binning (isotropic, directional, any edges) is host
arithmetic on a few thousand offsets.  Many fields (chains, realisations) go through in one call.

    variogram_map   the map of one field or a batch of fields
    experimental    Matheron's estimator per distance bin, optionally directional and in normal scores
    fit             a covariance model of sgs.cov_norm fitted to an experimental variogram (host)
    variograms      utilities.variograms's arguments and return tuple, plus `device`

The reference's SGS and kriging take every variogram parameter per cell (local_vario, interpolate.py:56-62, :141-147) and the
reference has nothing that estimates such maps.  Here the device makes the variogram map per WINDOW of tiles in one pass over the
pairs (gsm_variogram_local, csrc/variogram_local_kernel.hip), and an anisotropic model is fitted to each window's table:

    local_variogram_map   the map of every window of tiles, of one field or a batch
    fit_anisotropic       major and minor range, azimuth and sill fitted to a 2-D offset table (host); also for a VariogramMap
    fit_local             fit_anisotropic per window, expanded to [H, W] parameter maps (host)
    local_variograms      the three in one call: the `variogram` dict of interpolate.sgs / krige with parameter maps

Conventions.  scikit-gstat is not available where this package is built and tested, so its binning and fitting conventions
cannot be pinned by a test; the ones stated in `experimental` and `fit` are this package's own.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from .sgs import _axes, cov_norm

__all__ = ["VariogramMap", "variogram_map", "bin_map", "experimental", "fit", "variograms", "LocalVariogramMap", "LocalVariogram",
           "local_variogram_map", "fit_anisotropic", "fit_local", "local_variograms"]


@dataclass
class VariogramMap:
    """The offsets of the half plane di in [0, mi], dj in [-mj, mj] as [mi + 1, 2 mj + 1] arrays -- di, dj, the separation
    vector hx = dj dx, hy = di dy and its length dist -- and per field [R, mi + 1, 2 mj + 1]: sum of squared differences,
    count of pairs (int64) and gamma = sum / (2 count), NaN where count == 0.  The entries (0, dj <= 0) are empty: (0, -dj)
    holds the same pairs."""
    di: np.ndarray
    dj: np.ndarray
    hx: np.ndarray
    hy: np.ndarray
    dist: np.ndarray
    sum: np.ndarray
    count: np.ndarray
    gamma: np.ndarray


def _fields3(fields, shape):
    nd = fields.ndim
    if nd not in (2, 3) or tuple(fields.shape[-2:]) != tuple(shape):
        raise ValueError(f"fields must be [H, W] or [R, H, W] with the grid's shape {tuple(shape)}, got {tuple(fields.shape)}")
    return fields.reshape((-1,) + tuple(shape))


def offset_extents(H, W, dx, dy, maxlag):
    """(mi, mj): the row and column offsets within maxlag, at most H - 1 and W - 1."""
    if not maxlag > 0:
        raise ValueError("maxlag must be positive")
    return min(H - 1, int(math.floor(maxlag / abs(dy)))), min(W - 1, int(math.floor(maxlag / abs(dx))))


def _offsets(mi, mj, dx, dy):
    di, dj = np.meshgrid(np.arange(mi + 1), np.arange(-mj, mj + 1), indexing="ij")
    hx, hy = dj * dx, di * dy
    return di, dj, hx, hy, np.hypot(hx, hy)


def variogram_map(xx, yy, fields, maxlag, mask=None, device=None, _rows_per_part=None):
    """The variogram map of `fields` ([H, W], or [R, H, W] for R fields on the same grid; a NumPy array or a torch tensor, which
    may already be on the device) for every offset within maxlag along each axis: mi = min(H - 1, floor(maxlag / |dy|)) rows,
    mj = min(W - 1, floor(maxlag / |dx|)) columns.  NaN (or an infinity) marks a missing cell; `mask` ([H, W], optional) is
    shared by all fields and a False / 0 there makes the cell count as missing.  xx, yy: the cell coordinates, [H, W], axis-aligned
    with uniform spacing (either axis may descend, cells need not be square).  Returns a VariogramMap.
    Sums are fp64 and bit-reproducible: the same call twice gives the same bits, and row r of a batched call gives the bits of
    the call on fields[r] alone.  A large batch is sent in slices sized from the free device memory; slicing changes nothing."""
    import torch
    from .engine import GsmEngine, _ptr
    xx, yy = np.asarray(xx, dtype=np.float64), np.asarray(yy, dtype=np.float64)
    if xx.ndim != 2 or xx.shape != yy.shape:
        raise ValueError("xx and yy must be 2D arrays of the same shape")
    H, W = xx.shape
    if H < 3 or W < 3:
        raise ValueError(f"the grid must have at least 3 rows and 3 columns, got {(H, W)}")
    _, _, dx, dy = _axes(xx, yy)
    on_device = isinstance(fields, torch.Tensor)
    f3 = _fields3(fields if on_device else np.asarray(fields, dtype=np.float64), (H, W))
    R = f3.shape[0]
    if R < 1:
        raise ValueError("fields holds no field")
    if mask is not None:
        mask = np.asarray(mask)
        if mask.shape != (H, W):
            raise ValueError(f"mask must have the grid's shape {(H, W)}, got {mask.shape}")
    mi, mj = offset_extents(H, W, dx, dy, maxlag)
    n_off = (mi + 1) * (2 * mj + 1)
    s_out = np.empty((R, mi + 1, 2 * mj + 1), dtype=np.float64)
    c_out = np.empty((R, mi + 1, 2 * mj + 1), dtype=np.int64)
    eng = GsmEngine(H, W, 1, device)
    try:
        dev = eng.dev
        d_mask = None if mask is None else torch.as_tensor(np.ascontiguousarray(mask != 0, dtype=np.uint8)).to(dev)
        # a slice's own arrays: the fields (counted also when they are already on the device) and the two tables.  The library
        # adds its partials, at most 256 MiB or one field's; half of the free memory leaves room for them
        per_field = 8 * H * W + 16 * n_off
        step = max(1, min(R, (torch.cuda.mem_get_info(dev)[0] // 2) // per_field))
        with torch.cuda.device(dev):
            for r0 in range(0, R, step):
                part = f3[r0:r0 + step]
                d_f = (part if on_device else torch.as_tensor(np.ascontiguousarray(part))).to(device=dev, dtype=torch.float64).contiguous()
                n = int(d_f.shape[0])
                d_s = torch.empty((n, mi + 1, 2 * mj + 1), dtype=torch.float64, device=dev)
                d_c = torch.empty((n, mi + 1, 2 * mj + 1), dtype=torch.int64, device=dev)
                eng._check(eng.lib.gsm_variogram_map(eng.h, _ptr(d_f), n, _ptr(d_mask), mi, mj, int(_rows_per_part or 0), _ptr(d_s),
                                                     _ptr(d_c), eng._stream()))
                s_out[r0:r0 + n] = d_s.cpu().numpy()
                c_out[r0:r0 + n] = d_c.cpu().numpy()
    finally:
        eng.close()
    return _result(mi, mj, dx, dy, s_out, c_out)


def _result(mi, mj, dx, dy, s, c):
    with np.errstate(invalid="ignore", divide="ignore"):
        gamma = np.where(c > 0, s / (2.0 * c), np.nan)
    return VariogramMap(*_offsets(mi, mj, dx, dy), s, c, gamma)


def bin_edges(bin_func, maxlag, n_lags):
    """Upper bin edges: 'even' -> linspace(0, maxlag, n_lags + 1)[1:]; a sequence is taken as the upper edges themselves."""
    if isinstance(bin_func, str):
        if bin_func != "even":
            raise NotImplementedError("bin_func must be 'even' or a sequence of upper bin edges")
        return np.linspace(0.0, float(maxlag), int(n_lags) + 1)[1:]
    edges = np.asarray(bin_func, dtype=np.float64)
    if edges.ndim != 1 or edges.size < 1 or not (np.all(np.diff(edges) > 0) and edges[0] > 0):
        raise ValueError("bin edges must be a 1D ascending sequence of positive upper edges")
    return edges


def direction_filter(hx, hy, azimuth, tolerance):
    """True for the offsets whose direction lies within `tolerance` degrees of `azimuth` (degrees counter-clockwise from +x, the
    angle of sgs.rotation_matrix's major axis), directions taken modulo 180 degrees."""
    ang = np.degrees(np.arctan2(hy, hx))
    d = np.abs((ang - float(azimuth) + 90.0) % 180.0 - 90.0)
    return d <= float(tolerance)


def bin_map(vmap, edges, azimuth=None, tolerance=22.5):
    """Matheron's estimator per bin from a VariogramMap: offset (di, dj) belongs to bin k iff edges[k-1] < dist <= edges[k]
    (edges[-1] := 0), offsets beyond the last edge are dropped; gamma[r, k] = sum of the bin's sums / (2 * its count), NaN for
    an empty bin.  Returns (gamma [R, n], counts [R, n] int64)."""
    edges = np.asarray(edges, dtype=np.float64)
    dist = vmap.dist.ravel()
    k = np.searchsorted(edges, dist, side="left")             # first k with dist <= edges[k]
    keep = (dist > 0) & (k < edges.size)
    if azimuth is not None:
        keep &= direction_filter(vmap.hx.ravel(), vmap.hy.ravel(), azimuth, tolerance)
    R = vmap.sum.shape[0]
    s = vmap.sum.reshape(R, -1)[:, keep]
    c = vmap.count.reshape(R, -1)[:, keep]
    sums = np.zeros((R, edges.size))
    counts = np.zeros((R, edges.size), dtype=np.int64)
    for b in range(edges.size):
        sel = k[keep] == b
        sums[:, b] = [math.fsum(row) for row in s[:, sel]]
        counts[:, b] = c[:, sel].sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        gamma = np.where(counts > 0, sums / (2.0 * counts), np.nan)
    return gamma, counts


def _normal_scores(f3):
    """utilities.gaussian_transformation (utilities.py:7-25) on every field: the transformer is fitted on the first field's
    finite values and applied to all finite values."""
    from sklearn.preprocessing import QuantileTransformer
    ok = np.isfinite(f3)
    if not ok[0].any():
        raise ValueError("the first field holds no finite value to fit the normal-score transform on")
    nst = QuantileTransformer(n_quantiles=500, output_distribution="normal").fit(f3[0][ok[0]].reshape(-1, 1))
    out = np.full(f3.shape, np.nan)
    np.place(out, ok, nst.transform(f3[ok].reshape(-1, 1)).squeeze(axis=1))
    return out


def experimental(xx, yy, fields, maxlag=100e3, n_lags=70, bin_func='even', azimuth=None, tolerance=22.5, mask=None,
                 normal_score=False, device=None):
    """Experimental variogram (Matheron's estimator) of one field [H, W] or of R fields [R, H, W] on the grid (xx, yy):
    returns (bins [n], gamma [R, n], counts [R, n]).  The pair sums come from the device (variogram_map); the binning is host
    arithmetic on the offset table.
    Bins: `bins` are UPPER edges.  bin_func='even': linspace(0, maxlag, n_lags + 1)[1:]; a sequence is taken as the upper edges
    (n_lags is then ignored and maxlag is its last edge).  A pair at separation d belongs to bin k iff bins[k-1] < d <= bins[k]
    (0 < d <= bins[0] for the first); pairs beyond the last edge are dropped; an empty bin has gamma NaN and count 0.
    scikit-gstat, which the reference uses, is not available to pin this convention: it is this package's own.
    azimuth (degrees, the convention of sgs.rotation_matrix: counter-clockwise from +x) with tolerance keeps only the pairs
    whose direction lies within `tolerance` degrees of it, directions modulo 180.
    normal_score=True first transforms all finite values with QuantileTransformer(n_quantiles=500,
    output_distribution='normal') fitted, per call, on the first field's finite values (utilities.gaussian_transformation).
    mask, device: as variogram_map."""
    edges = bin_edges(bin_func, maxlag, n_lags)
    if normal_score:
        import torch
        if isinstance(fields, torch.Tensor):
            fields = fields.detach().cpu().numpy()
        fields = np.asarray(fields, dtype=np.float64)
        shape = np.shape(xx)
        fields = _normal_scores(_fields3(fields, shape))
    vmap = variogram_map(xx, yy, fields, float(edges[-1]), mask=mask, device=device)
    gamma, counts = bin_map(vmap, edges, azimuth, tolerance)
    return edges, gamma, counts


def model_gamma(h, vtype, rng, sill, nugget=0.0, s=None):
    """gamma(h) = nugget + (sill - nugget) - cov_norm(h / rng, ...): the variogram of the covariance the kriging kernels
    evaluate.  Spherical: cov_norm returns `sill - 1` beyond the range (a quirk that is the correct 0 only for sill = 1, the
    normal-score case); here gamma is the plateau `sill` there, so that a fit is decided by the model on h <= range."""
    h = np.asarray(h, dtype=np.float64)
    hn = h / rng
    c = cov_norm(hn, vtype, sill, nugget, s)
    if vtype.lower() == "spherical":
        c = np.where(hn > 1, 0.0, c)
    return nugget + (sill - nugget) - c


def _polish(f, h, g, w, p, lo, hi, rel_step=1e-4):
    """Gauss-Newton steps on curve_fit's answer until the step is at rounding level.  An optimiser that accepts a step only when
    the cost falls stops where cost differences drown in rounding, at about sqrt(eps) of the parameters; the stationary point of
    the normal equations is located to about eps, so that two variograms that differ in the last bits give fits that do too.
    The Jacobian is a central difference with a wide relative step: smooth in the parameters, with rounding noise of 1e-12.
    A step that leaves the bounds or is not finite ends the polish with the last accepted parameters."""
    p = np.array(p, dtype=np.float64)
    for _ in range(100):
        r = (f(h, *p) - g) * w
        J = np.empty((h.size, p.size))
        for k in range(p.size):
            e = np.zeros(p.size)
            e[k] = rel_step * p[k]
            J[:, k] = (f(h, *(p + e)) - f(h, *(p - e))) / (2.0 * e[k]) * w
        d = np.linalg.lstsq(J, -r, rcond=None)[0]
        q = p + d
        if not np.all(np.isfinite(q)) or np.any(q <= lo) or np.any(q >= hi):
            break
        p = q
        if np.max(np.abs(d / p)) < 1e-14:
            break
    return p


def fit(bins, gamma, counts, vtype, nugget=0.0, s=None):
    """Fit range and sill (and Matern's smoothness when s is None) of model_gamma to one experimental variogram by least
    squares weighted by the pair counts (scipy.optimize.curve_fit, sigma = 1 / sqrt(count), then Gauss-Newton steps down to
    rounding level: _polish); the nugget is held at `nugget`.
    Lags are the upper bin edges; empty bins (NaN gamma or count 0) are left out.  The model is sgs.cov_norm's, so a fitted
    model is exactly the one the kriging kernels evaluate (spherical: on h <= range, see model_gamma).
    Limitation: for a spherical fit with sill - nugget != 1 the result is not the model the kriging kernels evaluate beyond
    the range (they use cov_norm's `sill - 1` there) nor, through cov_norm's unscaled polynomial, one whose plateau is the sill;
    it is consistent for normal scores with nugget 0, where the sill is 1.
    Returns the `variogram` dict of interpolate.sgs / krige: major_range = minor_range = the fitted range, azimuth 0, sill,
    nugget, vtype, and s for Matern.  Conventions (lag at the bin's upper edge, weights) are this package's own."""
    from scipy.optimize import curve_fit
    vt = vtype.lower()
    if vt not in ("exponential", "gaussian", "spherical", "matern"):
        raise ValueError("vtype must be exponential, gaussian, spherical, or matern")
    h, g, c = (np.asarray(a, dtype=np.float64).ravel() for a in (bins, gamma, counts))
    if not (h.shape == g.shape == c.shape):
        raise ValueError("bins, gamma and counts must have the same length (one field's variogram)")
    ok = np.isfinite(g) & (c > 0)
    free_s = vt == "matern" and s is None
    if ok.sum() < (3 if free_s else 2):
        raise ValueError("too few non-empty bins to fit a variogram model")
    h, g, c = h[ok], g[ok], c[ok]
    p0 = [h.max() / 3.0, max(float(np.max(g)), nugget + 1e-12)] + ([1.5] if free_s else [])
    lo = [1e-9 * h.max(), nugget + 1e-12] + ([0.2] if free_s else [])
    hi = [np.inf, np.inf] + ([10.0] if free_s else [])
    f = (lambda x, r, sl, sm: model_gamma(x, vt, r, sl, nugget, sm)) if free_s else (lambda x, r, sl: model_gamma(x, vt, r, sl, nugget, s))
    w = np.sqrt(c)
    p, _ = curve_fit(f, h, g, p0=p0, sigma=1.0 / w, bounds=(lo, hi), x_scale="jac", max_nfev=5000)
    p = _polish(f, h, g, w, p, np.array(lo), np.array(hi))
    out = {"major_range": float(p[0]), "minor_range": float(p[0]), "azimuth": 0.0, "sill": float(p[1]), "nugget": float(nugget),
           "vtype": vt}
    if vt == "matern":
        out["s"] = float(p[2]) if free_s else float(s)
    return out


def variograms(xx, yy, grid, bin_func='even', maxlag=100e3, n_lags=70, covmodels=['gaussian', 'spherical', 'exponential', 'matern'],
               downsample=None, device=None):
    """gstatsim_custom.utilities.variograms (utilities.py:72-113) for gridded data: the normal-score transform of the
    conditioning values of `grid` (NaN where there is none), their isotropic experimental variogram on the device, and one
    fitted model per entry of covmodels.  Returns (vgrams, experimental, bins): vgrams[model] is the `variogram` dict that
    interpolate.sgs / krige take (the reference returns scikit-gstat's parameter lists), experimental the semivariance per bin
    (NaN for an empty bin), bins the upper edges.  `downsample` subsamples scattered points and has no meaning on a grid:
    anything but None raises NotImplementedError.  Binning and fit conventions: experimental, fit."""
    if downsample is not None:
        raise NotImplementedError("downsample subsamples scattered points; it has no gridded meaning (pass None)")
    grid = np.asarray(grid, dtype=np.float64)
    if grid.ndim != 2 or grid.shape != np.shape(xx) or grid.shape != np.shape(yy):
        raise ValueError("xx, yy, and grid must be 2D arrays of the same shape")
    bins, gamma, counts = experimental(xx, yy, grid, maxlag=maxlag, n_lags=n_lags, bin_func=bin_func, normal_score=True, device=device)
    vgrams = {m: fit(bins, gamma[0], counts[0], m) for m in covmodels}
    return vgrams, gamma[0], bins


# ---- local variogram maps and anisotropic fits per window ------------------------------------------------------------------------

@dataclass
class LocalVariogramMap:
    """VariogramMap's offset arrays (di, dj, hx, hy, dist, each [mi + 1, 2 mj + 1]), the lattice of tiles -- `tile` cells per
    side, Ty = ceil(H / tile) by Tx = ceil(W / tile), centres xc, yc [Ty, Tx] (the mean coordinate of a tile's cells, the ragged
    last tiles included) -- and per field and WINDOW [R, Ty, Tx, mi + 1, 2 mj + 1]: sum, count (int64), gamma = sum / (2 count),
    NaN where count == 0.  A pair belongs to the tile that holds its midpoint; the window of a tile is the (2 half_window + 1)^2
    tiles centred on it, clipped at the lattice's edge (half_window 0: the tile alone).  total_sum, total_count
    [R, mi + 1, 2 mj + 1]: the map of the whole field (gsm_variogram_map), which is also the sum of all tiles."""
    di: np.ndarray
    dj: np.ndarray
    hx: np.ndarray
    hy: np.ndarray
    dist: np.ndarray
    xc: np.ndarray
    yc: np.ndarray
    sum: np.ndarray
    count: np.ndarray
    gamma: np.ndarray
    total_sum: np.ndarray
    total_count: np.ndarray
    tile: int
    half_window: int
    shape: tuple


def _tile_centres(xs, ys, tile):
    """Mean coordinate of the cells of every tile: ([Ty], [Tx]) along y and x."""
    def centres(c):
        n = c.size
        return np.array([0.5 * (c[a] + c[min(a + tile, n) - 1]) for a in range(0, n, tile)])
    return centres(ys), centres(xs)


def _local_result(xs, ys, dx, dy, mi, mj, tile, half_window, s, c, total_s, total_c):
    yc, xc = _tile_centres(xs, ys, tile)
    xc2, yc2 = np.meshgrid(xc, yc)
    with np.errstate(invalid="ignore", divide="ignore"):
        gamma = np.where(c > 0, s / (2.0 * c), np.nan)
    return LocalVariogramMap(*_offsets(mi, mj, dx, dy), xc2, yc2, s, c, gamma, total_s, total_c, int(tile), int(half_window),
                             (ys.size, xs.size))


def local_variogram_map(xx, yy, fields, maxlag, tile, half_window=0, mask=None, device=None, _fields_per_part=None):
    """Variogram maps per window of tiles (gsm_variogram_local): `fields`, `maxlag`, `mask`, `device` and the grid as
    variogram_map; `tile` >= 2 cells per side of a tile, `half_window` >= 0 tiles on each side of a window's centre tile.
    Returns a LocalVariogramMap.  Every pair is counted once, in the tile of its midpoint, and a window adds its tiles' tables,
    so overlapping windows cost no pair work.  Bits as variogram_map: the same call twice gives the same bits, row r of a batch
    gives the bits of the call on fields[r] alone, and the slices a large batch is sent in change nothing."""
    import torch
    from .engine import GsmEngine, _ptr
    xx, yy = np.asarray(xx, dtype=np.float64), np.asarray(yy, dtype=np.float64)
    if xx.ndim != 2 or xx.shape != yy.shape:
        raise ValueError("xx and yy must be 2D arrays of the same shape")
    H, W = xx.shape
    if H < 3 or W < 3:
        raise ValueError(f"the grid must have at least 3 rows and 3 columns, got {(H, W)}")
    if int(tile) != tile or tile < 2:
        raise ValueError("tile must be an integer >= 2 (cells per side of a tile)")
    if int(half_window) != half_window or half_window < 0:
        raise ValueError("half_window must be an integer >= 0 (tiles on each side of a window's centre)")
    tile, half_window = int(tile), int(half_window)
    xs, ys, dx, dy = _axes(xx, yy)
    on_device = isinstance(fields, torch.Tensor)
    f3 = _fields3(fields if on_device else np.asarray(fields, dtype=np.float64), (H, W))
    R = f3.shape[0]
    if R < 1:
        raise ValueError("fields holds no field")
    if mask is not None:
        mask = np.asarray(mask)
        if mask.shape != (H, W):
            raise ValueError(f"mask must have the grid's shape {(H, W)}, got {mask.shape}")
    mi, mj = offset_extents(H, W, dx, dy, maxlag)
    Ty, Tx = -(-H // tile), -(-W // tile)
    table = (mi + 1, 2 * mj + 1)
    n_off = table[0] * table[1]
    s_out = np.empty((R, Ty, Tx) + table, dtype=np.float64)
    c_out = np.empty((R, Ty, Tx) + table, dtype=np.int64)
    ts_out = np.empty((R,) + table, dtype=np.float64)
    tc_out = np.empty((R,) + table, dtype=np.int64)
    eng = GsmEngine(H, W, 1, device)
    try:
        dev = eng.dev
        d_mask = None if mask is None else torch.as_tensor(np.ascontiguousarray(mask != 0, dtype=np.uint8)).to(dev)
        # a slice's own arrays: the fields (counted also when they are already on the device), the window tables and the whole
        # field's.  The library adds its tile tables, at most 1 GiB or one field's; half of the free memory leaves room for them
        per_field = 8 * H * W + 16 * n_off * (Ty * Tx + 1)
        step = int(_fields_per_part or max(1, min(R, (torch.cuda.mem_get_info(dev)[0] // 2) // per_field)))
        with torch.cuda.device(dev):
            for r0 in range(0, R, step):
                part = f3[r0:r0 + step]
                d_f = (part if on_device else torch.as_tensor(np.ascontiguousarray(part))).to(device=dev, dtype=torch.float64).contiguous()
                n = int(d_f.shape[0])
                d_s = torch.empty((n, Ty, Tx) + table, dtype=torch.float64, device=dev)
                d_c = torch.empty((n, Ty, Tx) + table, dtype=torch.int64, device=dev)
                d_ts = torch.empty((n,) + table, dtype=torch.float64, device=dev)
                d_tc = torch.empty((n,) + table, dtype=torch.int64, device=dev)
                eng._check(eng.lib.gsm_variogram_local(eng.h, _ptr(d_f), n, _ptr(d_mask), mi, mj, tile, half_window, _ptr(d_s), _ptr(d_c),
                                                       eng._stream()))
                eng._check(eng.lib.gsm_variogram_map(eng.h, _ptr(d_f), n, _ptr(d_mask), mi, mj, 0, _ptr(d_ts), _ptr(d_tc), eng._stream()))
                s_out[r0:r0 + n] = d_s.cpu().numpy()
                c_out[r0:r0 + n] = d_c.cpu().numpy()
                ts_out[r0:r0 + n] = d_ts.cpu().numpy()
                tc_out[r0:r0 + n] = d_tc.cpu().numpy()
    finally:
        eng.close()
    return _local_result(xs, ys, dx, dy, mi, mj, tile, half_window, s_out, c_out, ts_out, tc_out)


_VTYPES = ("exponential", "gaussian", "spherical", "matern")


def _aniso_gamma(hx, hy, q, vt, nugget, s):
    """model_gamma at |h . R| with M = R R^T = [[a, b], [b, c]] and q = (a, b, c, sill): |h . R|^2 = a hx^2 + 2 b hx hy + c hy^2."""
    a, b, c, sill = q
    return model_gamma(np.sqrt(np.maximum(a * hx * hx + 2.0 * b * hx * hy + c * hy * hy, 0.0)), vt, 1.0, sill, nugget, s)


def _aniso_polish(hx, hy, g, w, q, vt, nugget, s, rel_step=1e-4):
    """_polish for the anisotropic model, on q = (a, b, c, sill) of _aniso_gamma: Gauss-Newton steps until the step is at rounding
    level.  The central difference's step is relative to sqrt(a c) for the three entries of M (b may be zero) and to the sill.  A
    step that is not finite, leaves the positive-definite matrices or the sills above the nugget ends the polish with the last
    accepted q.  With residuals that are not zero (any measured table) the steps stop shrinking at about 1e-12, where the
    difference quotient's rounding noise times the residual takes over; the polish ends there instead of wandering on."""
    q = np.array(q, dtype=np.float64)
    last = np.inf
    for _ in range(100):
        scale = np.array([math.sqrt(q[0] * q[2])] * 3 + [q[3]])
        r = (_aniso_gamma(hx, hy, q, vt, nugget, s) - g) * w
        J = np.empty((g.size, 4))
        for k in range(4):
            e = np.zeros(4)
            e[k] = rel_step * scale[k]
            J[:, k] = (_aniso_gamma(hx, hy, q + e, vt, nugget, s) - _aniso_gamma(hx, hy, q - e, vt, nugget, s)) / (2.0 * e[k]) * w
        d = np.linalg.lstsq(J, -r, rcond=None)[0]
        p = q + d
        if not np.all(np.isfinite(p)) or p[0] <= 0 or p[2] <= 0 or p[0] * p[2] - p[1] * p[1] <= 0 or p[3] <= nugget:
            break
        q = p
        step = float(np.max(np.abs(d) / scale))
        if step < 1e-14 or (step < 1e-10 and step >= last):
            break
        last = step
    return q


def fit_anisotropic(hx, hy, gamma, counts, vtype, nugget=0.0, s=None, _start=None):
    """The anisotropic counterpart of `fit`: major_range >= minor_range, azimuth in [0, 180) and sill of model_gamma(|h . R|, ...)
    fitted to one table of offsets -- hx, hy, gamma, counts of the same shape, e.g. a VariogramMap's hx, hy, gamma[r], count[r] or
    one window of a LocalVariogramMap -- by least squares weighted with the pair counts; the nugget (and Matern's s, required)
    are held.  R is sgs.rotation_matrix's and the lag multiplies it from the left, as the kriging kernels do.
    The fit runs on the symmetric positive-definite M = R R^T through its Cholesky factor (three numbers: no angle that wraps
    around, no swap of the two ranges), then Gauss-Newton steps down to rounding (_aniso_polish); ranges and azimuth are read
    from M's eigen-decomposition: eigenvalues 1 / range^2, the major axis along the eigenvector of the smaller one.  When the
    ranges agree to 1e-9 relative they are returned equal with azimuth 0.0.  Empty offsets (NaN gamma or count 0) are left out.
    Returns the `variogram` dict of interpolate.sgs / krige.  Spherical: the limitation stated in `fit`."""
    from scipy.optimize import least_squares
    vt = vtype.lower()
    if vt not in _VTYPES:
        raise ValueError("vtype must be exponential, gaussian, spherical, or matern")
    if vt == "matern" and s is None:
        raise ValueError("a Matern fit of an offset table holds the smoothness: pass s")
    hx, hy, g, c = (np.asarray(a, dtype=np.float64).ravel() for a in (hx, hy, gamma, counts))
    if not (hx.shape == hy.shape == g.shape == c.shape):
        raise ValueError("hx, hy, gamma and counts must have the same shape (one table of offsets)")
    ok = np.isfinite(g) & (c > 0)
    if ok.sum() < 4 or np.linalg.matrix_rank(np.stack([hx[ok] ** 2, hx[ok] * hy[ok], hy[ok] ** 2], axis=1)) < 3:
        raise ValueError("too few non-empty offsets to fit an anisotropic variogram model (four, in three directions)")
    hx, hy, g, w = hx[ok], hy[ok], g[ok], np.sqrt(c[ok])
    if _start is None:
        def unpack(p):
            l0, l1, l2, sill = p
            return np.array([l0 * l0, l0 * l1, l1 * l1 + l2 * l2, sill])
        r0 = np.hypot(hx, hy).max() / 3.0
        p0 = [1.0 / r0, 0.0, 1.0 / r0, max(float(np.max(g)), nugget + 1e-9)]
        out = least_squares(lambda p: (_aniso_gamma(hx, hy, unpack(p), vt, nugget, s) - g) * w, p0, x_scale="jac", xtol=1e-15,
                            ftol=1e-15, gtol=1e-15, max_nfev=5000)
        q = unpack(out.x)
    else:
        q = np.asarray(_start, dtype=np.float64)
    if not np.all(np.isfinite(q)) or q[0] <= 0 or q[2] <= 0 or q[0] * q[2] - q[1] * q[1] <= 0 or q[3] <= nugget:
        raise ValueError("the anisotropic fit left the admissible models (M positive definite, sill above the nugget)")
    q = _aniso_polish(hx, hy, g, w, q, vt, nugget, s)
    ev, evec = np.linalg.eigh(np.array([[q[0], q[1]], [q[1], q[2]]]))
    major, minor = 1.0 / math.sqrt(ev[0]), 1.0 / math.sqrt(ev[1])
    azimuth = math.degrees(math.atan2(evec[1, 0], evec[0, 0])) % 180.0
    if major - minor <= 1e-9 * major:
        minor, azimuth = major, 0.0
    out = {"major_range": float(major), "minor_range": float(minor), "azimuth": float(azimuth), "sill": float(q[3]),
           "nugget": float(nugget), "vtype": vt}
    if vt == "matern":
        out["s"] = float(s)
    return out


def _aniso_q(v):
    """(a, b, c, sill) of _aniso_gamma for a variogram dict."""
    th = math.radians(v["azimuth"])
    cs, sn = math.cos(th), math.sin(th)
    la, lb = 1.0 / v["major_range"] ** 2, 1.0 / v["minor_range"] ** 2
    return np.array([cs * cs * la + sn * sn * lb, cs * sn * (la - lb), sn * sn * la + cs * cs * lb, v["sill"]])


class LocalVariogram(dict):
    """The `variogram` dict of interpolate.sgs / krige with [H, W] parameter maps; `fitted` [Ty, Tx] bool says which windows
    carry their own fit (the others took the whole field's), `windows` [Ty, Tx] holds every window's fitted dict."""
    fitted = None
    windows = None


def _expand(P, shape, tile, how, angle=False):
    """A [Ty, Tx] lattice of window values as an [H, W] map.  'nearest': every cell takes its own tile's.  'bilinear': linear
    between the tile centres along each axis (in cell indices; the ragged last tiles have their own centres), constant outside
    the outermost centres; an angle (degrees, modulo 180) goes through cos 2 theta, sin 2 theta."""
    H, W = shape
    if how == "nearest":
        return np.ascontiguousarray(P[np.arange(H)[:, None] // tile, np.arange(W)[None, :] // tile], dtype=np.float64)
    if angle:
        th = np.radians(2.0 * P)
        cs, sn = _expand(np.cos(th), shape, tile, how), _expand(np.sin(th), shape, tile, how)
        return (0.5 * np.degrees(np.arctan2(sn, cs))) % 180.0
    ci, cj = _tile_centres(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64), tile)
    rows = np.stack([np.interp(np.arange(W), cj, P[a]) for a in range(P.shape[0])])              # [Ty, W]
    return np.ascontiguousarray(np.stack([np.interp(np.arange(H), ci, rows[:, b]) for b in range(W)], axis=1))


def fit_local(lmap, vtype, nugget=0.0, s=None, min_pairs=500, field=0, expand="nearest", _start=None):
    """fit_anisotropic on every window of a LocalVariogramMap (host), expanded to parameter maps of the grid's shape.
    A window with fewer than min_pairs pairs in all, or whose fit fails (too few offsets, or a fit that leaves the admissible
    models), takes the fit of the whole field's table, lmap.total_*; that fit failing is an error.
    expand: 'nearest' -- every cell takes the window centred on its own tile -- or 'bilinear' -- linear between the tile centres,
    the azimuth through cos 2 theta and sin 2 theta, constant outside the outermost centres.
    Returns a LocalVariogram: the dict interpolate.sgs / krige take as is, major_range, minor_range, azimuth, sill as [H, W] maps
    without NaN, nugget, vtype (and s) as given, with `fitted` [Ty, Tx] bool as an attribute.  _start ([Ty, Tx] fitted dicts, e.g.
    an earlier result's `windows`): the windows' Gauss-Newton steps start there and the global search is left out.  Parameter maps go with vtype
    exponential, gaussian or spherical there (interpolate._local_table); a Matern result serves as a table of fits."""
    if expand not in ("nearest", "bilinear"):
        raise ValueError("expand must be 'nearest' or 'bilinear'")
    R, Ty, Tx = lmap.count.shape[:3]
    if not 0 <= int(field) < R:
        raise ValueError(f"field must be in [0, {R})")
    with np.errstate(invalid="ignore", divide="ignore"):
        tg = np.where(lmap.total_count[field] > 0, lmap.total_sum[field] / (2.0 * lmap.total_count[field]), np.nan)
    whole = fit_anisotropic(lmap.hx, lmap.hy, tg, lmap.total_count[field], vtype, nugget, s)
    fitted = np.zeros((Ty, Tx), dtype=bool)
    windows = np.empty((Ty, Tx), dtype=object)
    for a in range(Ty):
        for b in range(Tx):
            windows[a, b] = whole
            if lmap.count[field, a, b].sum() < min_pairs:
                continue
            try:
                windows[a, b] = fit_anisotropic(lmap.hx, lmap.hy, lmap.gamma[field, a, b], lmap.count[field, a, b], vtype, nugget, s,
                                                _start=None if _start is None else _aniso_q(_start[a, b]))
                fitted[a, b] = True
            except (ValueError, np.linalg.LinAlgError):
                pass
    out = LocalVariogram()
    for key in ("major_range", "minor_range", "azimuth", "sill"):
        P = np.array([[windows[a, b][key] for b in range(Tx)] for a in range(Ty)], dtype=np.float64)
        out[key] = _expand(P, lmap.shape, lmap.tile, expand, angle=key == "azimuth")
    out["nugget"], out["vtype"] = float(nugget), whole["vtype"]
    if "s" in whole:
        out["s"] = whole["s"]
    out.fitted, out.windows = fitted, windows
    return out


def local_variograms(xx, yy, grid, vtype, maxlag, tile, half_window=1, normal_score=True, mask=None, device=None, **fit_kw):
    """Parameter maps for non-stationary interpolate.sgs / krige in one call: the normal-score transform of the conditioning
    values of `grid` (NaN where there is none) as `variograms` makes it (normal_score=False: the values as they are), their
    local_variogram_map on the device, and fit_local (fit_kw: nugget, s, min_pairs, expand).  Returns fit_local's LocalVariogram."""
    grid = np.asarray(grid, dtype=np.float64)
    if grid.ndim != 2 or grid.shape != np.shape(xx) or grid.shape != np.shape(yy):
        raise ValueError("xx, yy, and grid must be 2D arrays of the same shape")
    if "field" in fit_kw:
        raise TypeError("local_variograms fits its one grid: `field` is not an argument")
    values = _normal_scores(grid[None])[0] if normal_score else grid
    lmap = local_variogram_map(xx, yy, values, maxlag, tile, half_window, mask=mask, device=device)
    return fit_local(lmap, vtype, **fit_kw)
