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

Conventions.  scikit-gstat is not available where this package is built and tested, so its binning and fitting conventions
cannot be pinned by a test; the ones stated in `experimental` and `fit` are this package's own.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from .sgs import _axes, cov_norm

__all__ = ["VariogramMap", "variogram_map", "bin_map", "experimental", "fit", "variograms"]


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
