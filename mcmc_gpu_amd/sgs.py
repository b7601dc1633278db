"""Host-side mirror of the reference's SMALL-scale chain (gstatsMCMC/MCMC.py namespace):

    chain_sgs                      gstatsMCMC/MCMC.py:1445-1911   -> chain_sgs_gpu
    init_msc_chain_by_instance     gstatsMCMC/MCMC.py:402-431
    sgs / neighbors / ok_solve / sk_solve   MCMC.py:91-173, gstatsim_custom/neighbors.py:4-64, _krige.py:5-81  -> sgs, gsm_sgs_blocks (HIP)

Same class / setter names, argument meaning and return tuple as the reference.  Per iteration the host draws what the
reference draws from the chain's NumPy generator, in its order (block centre by rejection, block sizes, the shuffle of
the block's cells, one normal per simulated cell, the accept uniform -- none of which depends on the chain's state) and
the device does the work: the sequential Gaussian simulation of the block (octant search + ordinary kriging per cell),
the full-grid mass-conservation loss and thickness guard of the proposed bed, and the commit.  All chains of a call
share one libgsm_hip handle (run_many_sgs); chain_sgs_gpu.run is the one-chain case.

Normal-score transform (do_transform): the transformer is a caller-supplied object (scikit-learn's QuantileTransformer
in the reference's drivers).  Its transform / inverse_transform are called on the host once per iteration on the whole
map, exactly where the reference calls them (MCMC.py:1766, :1777); simulation and loss still run on the device.

Numerics: the kriging systems are solved by pivoted elimination on the device where the reference calls
numpy.linalg.lstsq, so simulated values agree with the CPU chain to ~1e-9 of the bed's scale, not bit for bit; accept
decisions are identical unless an accept uniform falls within that distance of its threshold.
Kept reference behaviour: the loop runs n_iter times and overwrites the record of the initial
state at index 0.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import sys
import time
from collections import namedtuple
from copy import deepcopy

import numpy as np

from ._lib import TAIL_QT_AUTO, TAIL_QT_OFF, TAIL_QT_ON

__all__ = ["chain_sgs_gpu", "init_msc_chain_by_instance", "run_many_sgs", "batch_plan", "sgs", "cov_norm", "lag_cov_table", "trend_of",
           "gaussian_weights", "check_groups", "slice_groups", "handoff", "fit_normal_scores", "quantile_probabilities"]


def gaussian_weights(sigma, truncate=4.0):
    """The weights of one axis of scipy.ndimage.gaussian_filter(order=0), in scipy's NumPy arithmetic
    (scipy/ndimage/_filters.py: gaussian_filter1d, _gaussian_kernel1d)."""
    sd = float(sigma)
    lw = int(float(truncate) * sd + 0.5)
    x = np.arange(-lw, lw + 1)
    phi = np.exp(-0.5 / (sd * sd) * x ** 2)
    return phi / phi.sum()


def trend_of(beds, sigma=10, truncate=4.0, device=None, mode="reflect"):
    """The trend the reference's driver takes off a large-scale bed before the small-scale chain,
    scipy.ndimage.gaussian_filter(bed, sigma) (smallScaleChain_multiprocessing.py:486), of one bed [H, W] or of a stack
    [n, H, W] (each bed filtered on its own: the stack axis is not an axis of the filter).  `sigma` is a number or a
    (rows, columns) pair; only mode='reflect', scipy's default, exists (ValueError otherwise).
    device=True: the HIP kernels (gsm_gaussian_filter), all beds in one call; raises without a GPU.
    device=False: scipy on the host, bed by bed.
    device=None (default): the HIP kernels when a GPU is visible, else scipy -- the pattern of MCMC_gpu.min_dist_from_mask:
    set-up code runs where there is no GPU.  The two agree to the rounding of their summation orders (gsm.h), not bit for bit.
    A device tensor is taken and returned as one (device path only); arrays come back as arrays."""
    if mode != "reflect":
        raise ValueError("trend_of: only mode='reflect' (scipy's default, the reference's) is implemented")
    sg = np.atleast_1d(np.asarray(sigma, dtype=np.float64))
    if sg.shape not in ((1,), (2,)) or not np.all(np.isfinite(sg)) or np.any(sg <= 0) or not (float(truncate) > 0):
        raise ValueError("trend_of: sigma must be a positive number or a pair of them, truncate positive")
    s0, s1 = (float(sg[0]), float(sg[-1]))
    import torch
    is_tensor = isinstance(beds, torch.Tensor)
    shape = tuple(beds.shape)
    if len(shape) not in (2, 3) or 0 in shape:
        raise ValueError("trend_of: beds must be one bed [H, W] or a stack [n, H, W]")
    if device is None:
        device = torch.cuda.is_available()
    if device:
        from .engine import GsmEngine
        w0, w1 = gaussian_weights(s0, truncate), gaussian_weights(s1, truncate)
        if max(w0.size, w1.size) // 2 > 128:
            raise ValueError("trend_of: truncate * sigma above 128 cells is more than gsm_gaussian_filter takes")
        x = beds if is_tensor else np.asarray(beds, dtype=np.float64)
        x3 = x.reshape((-1,) + shape[-2:])
        eng = GsmEngine(shape[-2], shape[-1], 1, device=x.device.index if is_tensor and x.is_cuda else None)      # raises RuntimeError without a GPU
        try:
            out = eng.gaussian_filter(x3, w0, w1).reshape(shape)
            return out if is_tensor else out.cpu().numpy()
        finally:
            eng.close()
    if is_tensor:
        raise ValueError("trend_of: a tensor goes through the device path (device=True)")
    from scipy.ndimage import gaussian_filter
    x = np.asarray(beds, dtype=np.float64)
    if x.ndim == 2:
        return gaussian_filter(x, sigma=(s0, s1), truncate=float(truncate), mode="reflect")
    return np.stack([gaussian_filter(b, sigma=(s0, s1), truncate=float(truncate), mode="reflect") for b in x])


def quantile_probabilities(n_quantiles):
    """The probabilities at which QuantileTransformer._dense_fit takes its quantiles, after the round trip scikit-learn and NumPy make:
    references_ * 100 (scikit-learn, to percent) / 100 (np.nanpercentile, back).  Not always references_ itself."""
    return (np.linspace(0, 1, int(n_quantiles), endpoint=True) * 100) / 100


def fit_normal_scores(fields, n_quantiles=1000, random_state=None, device=None, stack=False):
    """The normal-score transformers the reference's driver fits on a detrended bed,
        QuantileTransformer(n_quantiles, output_distribution='normal', subsample=None, random_state).fit(field.reshape(-1, 1))
    (smallScaleChain_multiprocessing.py:493-494), each field on its own.  `fields` is one field [H, W], a stack [n, H, W], or -- with
    stack=True, which tells the two 2-D readings apart -- a stack [n, cells] (the cells of a mask, say).
    Returns a list of n fitted scikit-learn QuantileTransformer objects (one field: a list of one).
    device=True: one gsm_qt_fit call for the whole stack; each object is an unfitted QuantileTransformer given n_quantiles_,
    references_, quantiles_ and n_features_in_.  The tables have the bits of scikit-learn's fit.  Raises without a GPU.
    device=False: scikit-learn's fit, field by field.
    device=None (default): the device when a GPU is visible, else scikit-learn (trend_of's rule).
    A device tensor is taken on the device path only.  NaN cells are left out of a field's fit, as scikit-learn leaves them out.
    ValueError: n_quantiles above the number of cells of a field (scikit-learn clips with a warning; the device holds one table
    length for all fields of a run), n_quantiles below 2, a field that holds +inf or -inf (scikit-learn's own refusal)."""
    import torch
    from sklearn.preprocessing import QuantileTransformer
    is_tensor = isinstance(fields, torch.Tensor)
    shape = tuple(fields.shape)
    if len(shape) not in (2, 3) or 0 in shape or (stack and len(shape) != 2):
        raise ValueError("fit_normal_scores: fields must be one field [H, W], a stack [n, H, W] or (stack=True) a stack [n, cells]")
    n = shape[0] if (stack or len(shape) == 3) else 1
    nq = int(n_quantiles)
    if nq < 2:
        raise ValueError("fit_normal_scores: n_quantiles must be at least 2")
    if device is None:
        device = torch.cuda.is_available()
    if not device and is_tensor:
        raise ValueError("fit_normal_scores: a tensor goes through the device path (device=True)")
    x = (fields if is_tensor else np.asarray(fields, dtype=np.float64)).reshape(n, -1)
    if nq > x.shape[1]:
        raise ValueError(f"fit_normal_scores: n_quantiles = {nq} is above the {x.shape[1]} cells of a field")
    make = lambda: QuantileTransformer(n_quantiles=nq, output_distribution='normal', subsample=None, random_state=random_state)
    if not device:
        if np.isinf(x).any():
            raise ValueError("fit_normal_scores: a field holds infinity")
        return [make().fit(f.reshape(-1, 1)) for f in x]
    from .engine import GsmEngine
    eng = GsmEngine(1, 1, 1, device=x.device.index if is_tensor and x.is_cuda else None)      # `cells` is the call's own: any handle serves
    try:
        quantiles, _, n_inf, _ = eng.qt_fit(x, quantile_probabilities(nq))
        quantiles, n_inf = quantiles.cpu().numpy(), n_inf.cpu().numpy()
    finally:
        eng.close()
    if n_inf.any():
        raise ValueError("fit_normal_scores: a field holds infinity")
    out = []
    for row in quantiles:
        t = make()
        t.n_quantiles_, t.references_, t.n_features_in_ = nq, np.linspace(0, 1, nq, endpoint=True), 1
        t.quantiles_ = np.ascontiguousarray(row.reshape(nq, 1))
        out.append(t)
    return out


def cov_norm(h, vtype, sill, nugget, s=None):
    """Covariance models of gstatsim_custom on normalised lag (covariance.py:4-28), incl. the spherical model's
    `sill - 1` beyond the range and Matern's h == 0 -> 1e-8 substitution (the input is not mutated here)."""
    vtype = vtype.lower()
    if vtype == "exponential":
        return (sill - nugget) * np.exp(-3 * h)
    if vtype == "gaussian":
        return (sill - nugget) * np.exp(-3 * np.square(h))
    if vtype == "spherical":
        c = sill - nugget - 1.5 * h + 0.5 * np.power(h, 3)
        return np.where(h > 1, sill - 1, c)
    if vtype == "matern":
        from scipy.special import gamma, kv
        sc = 0.45246434 * np.exp(-0.70449189 * s) + 1.7863836
        hh = np.where(h == 0.0, 1e-8, h)
        c = (sill - nugget) * 2 / gamma(s) * np.power(sc * hh * np.sqrt(s), s) * kv(s, 2 * sc * hh * np.sqrt(s))
        return np.where(np.isnan(c), sill - nugget, c)
    raise ValueError("vtype must be Exponential, Gaussian, Spherical or Matern")


def rotation_matrix(v: dict) -> np.ndarray:
    """Anisotropy rotation x scaling (make_rotation_matrix, _krige.py:83-103)."""
    th = (v["azimuth"] / 180.0) * np.pi
    return np.dot(np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]),
                  np.array([[1 / v["major_range"], 0], [0, 1 / v["minor_range"]]]))


def lag_cov_table(vario: dict, hw: int, dx: float, dy: float, mi: int | None = None, mj: int | None = None) -> np.ndarray:
    """Covariance at every integer lag (di, dj), |di| <= mi, |dj| <= mj (default 2 hw: two neighbours of one cell), between
    two cells of an axis-aligned grid with column spacing dx and row spacing dy (signed): what make_sigma / make_rho
    (_krige.py:105-143) evaluate pair by pair."""
    mi = 2 * int(hw) if mi is None else int(mi)
    mj = 2 * int(hw) if mj is None else int(mj)
    R = rotation_matrix(vario)
    di = np.arange(-mi, mi + 1)[:, None] * dy
    dj = np.arange(-mj, mj + 1)[None, :] * dx
    m0 = dj * R[0, 0] + di * R[1, 0]
    m1 = dj * R[0, 1] + di * R[1, 1]
    h = np.sqrt(m0 * m0 + m1 * m1)
    return np.ascontiguousarray(cov_norm(h, vario["vtype"], vario["sill"], vario["nugget"], vario.get("s")))


def _generator(seed):
    """utilities.get_random_generator (utilities.py:50-70)."""
    if seed is None:
        return np.random.default_rng()
    if isinstance(seed, int):
        return np.random.default_rng(seed=seed)
    if isinstance(seed, np.random.Generator):
        return seed
    raise ValueError("Seed should be an integer, a NumPy random Generator, or None")


def lag_extents(hw: int, H: int, W: int) -> tuple[int, int]:
    """Extents of the lag table handed to gsm_sgs_blocks: the whole grid while that stays small (4 M lags = 32 MiB), so that
    the radius-widening fallback (MCMC.py:150-156) finds every lag; else what a search window needs."""
    if (2 * H - 1) * (2 * W - 1) <= (1 << 22):
        return H - 1, W - 1
    return min(2 * int(hw), H - 1), min(2 * int(hw), W - 1)


def _axes(xx, yy):
    xs, ys = np.ascontiguousarray(xx[0, :], dtype=np.float64), np.ascontiguousarray(yy[:, 0], dtype=np.float64)
    if not (np.array_equal(xx, np.broadcast_to(xs[None, :], xx.shape)) and np.array_equal(yy, np.broadcast_to(ys[:, None], yy.shape))):
        raise NotImplementedError("the device SGS needs an axis-aligned grid (xx[i, j] = x[j], yy[i, j] = y[i])")
    dx, dy = xs[1] - xs[0], ys[1] - ys[0]
    if not (np.allclose(np.diff(xs), dx, rtol=1e-9, atol=0) and np.allclose(np.diff(ys), dy, rtol=1e-9, atol=0)):
        raise NotImplementedError("the device SGS needs uniform grid spacing")
    return xs, ys, float(dx), float(dy)


def sgs(xx, yy, grid, variogram, radius=100e3, num_points=20, ktype='ok', sim_mask=None, quiet=False, stencil=None, rcond=None,
        seed=None, device=None):
    """Sequential Gaussian simulation with ordinary ('ok') or simple ('sk') kriging -- the reference's module-level MCMC.sgs
    (MCMC.py:91-173 with _preprocess :42-88), same arguments and return value, executed by gsm_sgs_blocks.  The generator is
    consumed exactly as the reference consumes it: one shuffle of the cells of sim_mask, then one normal per simulated cell.
    Limits of the device path (NotImplementedError otherwise): the NaN cells to simulate lie within one window of at most 1024
    cells (the small-scale chain's blocks; MCMC.py:1762-1774), the circular search stencil and lstsq's default rcond,
    scalar variogram parameters, 8 <= num_points <= 48, an axis-aligned uniform grid."""
    import torch
    from .engine import GsmEngine, _ptr
    for name, a in (("xx", xx), ("yy", yy), ("grid", grid)):
        if not isinstance(a, np.ndarray) or a.ndim != 2:
            raise ValueError(f"{name} must be a 2D NumPy array")                  # _sanity_checks, interpolate.py:282-298
    if xx.shape != yy.shape or xx.shape != grid.shape:
        raise ValueError("xx, yy, and grid must have same shape")
    for key in ("major_range", "minor_range", "azimuth", "sill", "nugget", "vtype"):
        if key not in variogram:
            raise ValueError(f"Missing variogram parameter {key}")
    if variogram["vtype"].lower() == "matern" and "s" not in variogram:
        raise ValueError("Missing variogram parameter s for Matern covariance")
    if ktype not in ("ok", "sk"):
        raise ValueError("ktype must be 'ok' or 'sk'")
    if stencil is not None or rcond is not None:
        raise NotImplementedError("the device SGS searches the circular stencil and solves with lstsq's default cut-off (rcond=None)")
    if any(not isinstance(variogram[k], (int, float, np.integer, np.floating)) for k in variogram if k != "vtype"):
        raise NotImplementedError("the device SGS takes scalar variogram parameters (one covariance table per call)")
    if not 8 <= int(num_points) <= 48:
        raise NotImplementedError("the device SGS takes 8 <= num_points <= 48")
    rng = _generator(seed)
    grid = np.asarray(grid, dtype=np.float64)
    H, W = grid.shape
    cond_msk = ~np.isnan(grid)
    if sim_mask is None:
        sim_mask = np.full(xx.shape, True)
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    inds = np.array([ii[sim_mask].flatten(), jj[sim_mask].flatten()]).T
    global_mean = np.mean(grid[cond_msk])                                          # MCMC.py:81
    rng.shuffle(inds)                                                                 # MCMC.py:128
    need = ~cond_msk[inds[:, 0], inds[:, 1]] if inds.shape[0] else np.zeros(0, bool)
    todo = inds[need]
    out = grid.copy()
    if todo.shape[0] == 0:
        return out
    r0, r1, c0, c1 = int(todo[:, 0].min()), int(todo[:, 0].max()) + 1, int(todo[:, 1].min()), int(todo[:, 1].max()) + 1
    if (r1 - r0) * (c1 - c0) > 1024:
        raise NotImplementedError("the device SGS simulates one block: the cells to simulate must fit a window of at most 1024 cells")
    # listed cells: the cells to simulate in visiting order, then every other window cell that holds a value (conditioning data:
    # never simulated, seen by the search from the start); a window cell that stays NaN is not listed
    inside = np.zeros((H, W), bool); inside[r0:r1, c0:c1] = True
    todo_m = np.zeros((H, W), bool); todo_m[todo[:, 0], todo[:, 1]] = True
    rest = np.argwhere(inside & cond_msk & ~todo_m)
    cells = np.ascontiguousarray(np.concatenate([todo, rest]), dtype=np.int32)
    z = np.zeros(cells.shape[0])
    z[:todo.shape[0]] = rng.standard_normal(todo.shape[0])                           # rng.normal(est, sd, 1) = est + sd * normal, :165
    xs, ys, dx, dy = _axes(np.asarray(xx, dtype=np.float64), np.asarray(yy, dtype=np.float64))
    vario = {k: (variogram[k] if k == "vtype" else float(variogram[k])) for k in variogram}
    hw = int(math.ceil(float(radius) / abs(dx)))
    eng = GsmEngine(H, W, 1, device)
    try:
        dev, lib, h = eng.dev, eng.lib, eng.h
        f64 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
        i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
        mi, mj = lag_extents(hw, H, W)
        d_grid, d_xs, d_ys, d_lag = f64(grid[None]), f64(xs), f64(ys), f64(lag_cov_table(vario, hw, dx, dy, mi, mj))
        d_win, d_off, d_cells, d_z = i32([[r0, r1, c0, c1]]), i32([0, cells.shape[0]]), i32(cells), f64(z)
        d_gm = f64([global_mean])
        with torch.cuda.device(dev):
            eng._check(lib.gsm_sgs_set_kriging(h, 1 if ktype == "sk" else 0, _ptr(d_gm)))
            eng._check(lib.gsm_sgs_blocks(h, _ptr(d_grid), None, _ptr(d_win), _ptr(d_xs), _ptr(d_ys), _ptr(d_lag), mi, mj, hw, float(radius),
                                          int(num_points), float(vario["sill"]), _ptr(d_off), _ptr(d_cells), _ptr(d_z), int(cells.shape[0]),
                                          None, None, eng._stream()))
        out = d_grid[0].cpu().numpy()
    finally:
        eng.close()
    return out


class chain_sgs_gpu:
    """Small-scale (SGS block) Metropolis chain executed on the MI355X (reference chain_sgs, MCMC.py:1445-1911)."""

    def __init__(self, xx, yy, initial_bed, surf, velx, vely, dhdt, smb, cond_bed, data_mask, grounded_ice_mask, resolution):
        self.xx, self.yy = xx, yy
        self.initial_bed = initial_bed
        self.surf, self.velx, self.vely, self.dhdt, self.smb = surf, velx, vely, dhdt, smb
        self.cond_bed = cond_bed
        self.data_mask = data_mask
        self.grounded_ice_mask = grounded_ice_mask
        self.resolution = resolution
        self.loss_function_list = []
        self.sample_loc = None
        shp = initial_bed.shape
        if any(a.shape != shp for a in (surf, velx, vely, dhdt, smb, cond_bed, data_mask)):
            raise Exception('the shape of bed, surf, velx, vely, dhdt, smb, radar_bed, data_mask need to be same')
        self.do_transform = False
        self.nst_trans = None
        self.trend = None
        self.detrend_map = False

    # ---- setters shared with the large-scale chain (MCMC.py:849-872, :950-1018) ---------------------------------------
    def set_update_region(self, update_in_region, region_mask=[]):
        self.update_in_region = update_in_region
        if update_in_region is False:
            self.region_mask = np.full(self.xx.shape, 1)
        else:
            if np.shape(region_mask) != self.xx.shape:
                raise ValueError('the region_mask input is invalid. It has to be a 2D numpy array with the shape of the map')
            self.region_mask = region_mask

    def set_loss_type(self, sigma_mc=-1, massConvInRegion=True):
        self.mc_region_mask = self.region_mask if massConvInRegion else np.full(self.xx.shape, 1)
        self.sigma_mc = sigma_mc

    def set_sample_points_locations(self, loc):
        self.sample_loc = loc

    # ---- chain_sgs setters (MCMC.py:1466-1598) ------------------------------------------------------------------------
    def set_normal_transformation(self, nst_trans, do_transform=True):
        self.do_transform = do_transform
        self.nst_trans = nst_trans if do_transform else None

    def set_trend(self, trend=None, detrend_map=True):
        if detrend_map == True:  # noqa: E712
            if trend is None or len(trend) != len(self.xx) or trend.shape != self.xx.shape:
                raise ValueError('if detrend_map is set to True, then the trend of the topography, which is a 2D numpy array, must be provided')
            self.trend = trend
        else:
            self.trend = None
        self.detrend_map = detrend_map

    def set_variogram(self, vario_type, vario_range, vario_sill, vario_nugget, isotropic=True, vario_smoothness=None,
                      vario_azimuth=None):
        if vario_type in ('Gaussian', 'Exponential', 'Spherical'):
            pass
        elif vario_type == 'Matern':
            if (vario_smoothness is None) or (vario_smoothness <= 0):
                raise ValueError('vario_smoothness argument should be a positive float when the vario_type is Matern')
        else:
            raise ValueError('vario_type argument should be one of the following: Gaussian, Exponential, Spherical, or Matern')
        self.vario_type = vario_type
        if isotropic:
            self.vario_param = [0, vario_nugget, vario_range, vario_range, vario_sill, vario_type, vario_smoothness]
        else:
            if len(vario_range) != 2:
                raise ValueError("vario_range need to be a list with two floats to specifying for major range and minor range of the variogram when isotropic is set to False")
            self.vario_param = [vario_azimuth, vario_nugget, vario_range[0], vario_range[1], vario_sill, vario_type, vario_smoothness]

    def set_sgs_param(self, sgs_num_nearest_neighbors, sgs_searching_radius, sgs_rand_dropout_on=False, dropout_rate=0):
        if sgs_rand_dropout_on == False:  # noqa: E712
            dropout_rate = 0
        self.sgs_param = [sgs_num_nearest_neighbors, sgs_searching_radius, sgs_rand_dropout_on, dropout_rate]

    def set_block_sizes(self, block_min_x, block_max_x, block_min_y, block_max_y):
        self.block_min_x, self.block_min_y = block_min_x, block_min_y
        self.block_max_x, self.block_max_y = block_max_x, block_max_y

    def set_random_generator(self, rng_seed=None):
        if rng_seed is None:
            rng = np.random.default_rng()
        elif isinstance(rng_seed, (int, np.integer)):
            rng = np.random.default_rng(seed=int(rng_seed))
            self.rng_seed = int(rng_seed)
        elif isinstance(rng_seed, np.random.Generator):
            rng = rng_seed
        else:
            raise ValueError('Seed should be an integer, a NumPy random Generator, or None')
        self.rng = rng

    def set_rng_mode(self, mode):
        """'replay' (default): the draws come from chain.rng in the reference's order (MCMC.py:1750-1797) -- accept masks and
        beds follow the reference on the same seed.  'philox': the draws are made on the device from Philox4x32-10 counters
        keyed by the chain's seed (gsm_sgs_draw_philox) -- no host work per iteration; a chain of its own definition, restated
        by oracle/sgs_philox_oracle.py.  'pcg64': the draws of 'replay' -- chain.rng's own NumPy PCG64 stream, bit for bit -- made on
        the device (gsm_sgs_draw_pcg64): the reference's chain on the same seed without host work per iteration."""
        if mode not in ('replay', 'philox', 'pcg64'):
            raise ValueError("rng mode must be 'replay', 'pcg64' or 'philox'")
        self.rng_mode = mode
        self.philox_iter = 0

    def _philox_seed(self):
        seed = getattr(self, 'rng_seed', None)
        if seed is None:
            seed = int(self.rng.bit_generator.seed_seq.entropy) if hasattr(self.rng.bit_generator, 'seed_seq') else 0
        return int(seed) & 0xFFFFFFFFFFFFFFFF

    def loss(self, massConvResidual, dataDiff):
        loss_mc = np.nansum(np.square(massConvResidual[self.mc_region_mask == 1])) / (2 * self.sigma_mc ** 2)
        return loss_mc + 0, loss_mc, 0

    def _vario(self):
        vp = self.vario_param
        v = dict(azimuth=vp[0], nugget=vp[1], major_range=vp[2], minor_range=vp[3], sill=vp[4], vtype=vp[5])
        if vp[5] == 'Matern':
            v['s'] = vp[6]
        return v

    # ---- host draws of one iteration (MCMC.py:1747-1760, sgs :128, :165, run :1799) -------------------------------------
    def _draw_iteration(self, rng, cond_is_data):
        H, W = self.xx.shape
        while True:
            ix = rng.integers(low=0, high=H, size=1)[0]
            iy = rng.integers(low=0, high=W, size=1)[0]
            if self.region_mask[ix, iy] == 1:
                break
        bsx = rng.integers(low=self.block_min_x, high=self.block_max_x, size=1)[0]
        bsy = rng.integers(low=self.block_min_y, high=self.block_max_y, size=1)[0]
        r0 = max(0, int(ix - bsx / 2)); r1 = min(H, int(ix + bsx / 2))
        c0 = max(0, int(iy - bsy / 2)); c1 = min(W, int(iy + bsy / 2))
        ii, jj = np.meshgrid(np.arange(r0, r1), np.arange(c0, c1), indexing='ij')
        inds = np.array([ii.flatten(), jj.flatten()]).T
        rng.shuffle(inds)
        need = ~cond_is_data[inds[:, 0], inds[:, 1]] if inds.shape[0] else np.zeros(0, bool)
        z = np.zeros(inds.shape[0])
        if need.any():
            z[need] = rng.standard_normal(int(need.sum()))     # rng.normal(est, sd, 1) = est + sd * standard normal
        u = rng.random()
        return (ix, iy, bsx, bsy), (r0, r1, c0, c1), np.ascontiguousarray(inds, dtype=np.int32), z, u

    def run(self, n_iter, only_save_last_bed=False, info_per_iter=100, plot=True, progress_bar=True):
        """n_iter SGS-block Metropolis iterations from self.initial_bed; returns the reference's tuple (bed or bed_cache,
        loss_mc_cache, loss_data_cache, loss_cache, step_cache, resampled_times, blocks_cache[, sample_values])."""
        if not hasattr(self, 'rng'):
            self.set_random_generator(getattr(self, 'rng_seed', None))
        mode = getattr(self, 'rng_mode', 'replay')
        philox = mode == 'philox'
        out, _ = run_many_sgs(self, [self.initial_bed], [self.rng], n_iter, only_save_last_bed=only_save_last_bed,
                              info_per_iter=info_per_iter, progress_bar=progress_bar,
                              philox_seeds=[self._philox_seed()] if philox else None, philox_iter0=getattr(self, 'philox_iter', 0),
                              pcg64=(mode == 'pcg64'))
        if philox:
            self.philox_iter += int(n_iter)
        return out[0]


def host_draws(chain, rngs, cond_is_data, it0, kb, n):
    """The host draws of iterations it0 .. it0 + kb - 1 of n chains, packed for one gsm_sgs_iterate call.  Contract: chain c's
    generator rngs[c] is consumed for its kb iterations consecutively and the loop is chain-major -- what chain_sgs.run would
    consume chain by chain; the draws do not depend on the chains' state.  The packing is iteration-major: wins[j, c] and us[j, c]
    belong to iteration it0 + j of chain c, `cells` and `z` hold the cells and normals in (j, c) order, offs[j] is iteration j's
    prefix over the chains (offs[j, n] = its cell count) and bases[j] the running total, so that chain c's cells of iteration j are
    cells[bases[j] + offs[j, c] : bases[j] + offs[j, c + 1]].  Returns (packed arrays, block records [n, kb, 4])."""
    wins = np.empty((kb, n, 4), np.int32); offs = np.zeros((kb, n + 1), np.int32); us = np.empty((kb, n))
    blocks = np.empty((n, kb, 4), np.int64)
    inds = [[None] * n for _ in range(kb)]; zs = [[None] * n for _ in range(kb)]
    for c in range(n):                     # per chain in iteration order: each chain owns its generator
        for j in range(kb):
            blocks[c, j], wins[j, c], inds[j][c], zs[j][c], us[j, c] = chain._draw_iteration(rngs[c], cond_is_data)
    for j in range(kb):
        offs[j, 1:] = np.cumsum([a.shape[0] for a in inds[j]])
    bases = np.concatenate([[0], np.cumsum(offs[:, n], dtype=np.int64)])
    tot = int(bases[kb])
    cells = np.ascontiguousarray(np.concatenate([a for row in inds for a in row]) if tot else np.zeros((1, 2), np.int32))
    z = np.concatenate([a for row in zs for a in row]) if tot else np.zeros(1)
    return dict(it0=it0, kb=kb, wins=wins, offs=offs, us=us, bases=bases, cells=cells, z=z), blocks


def batch_plan(n_iter, batch, snapshot_iterations=None):
    """The sizes of the batches that n_iter iterations are run in: at most `batch` iterations each, and every snapshot iteration
    (posterior=) is the last iteration of its batch, so that the chains' state after it is on the device when the batch ends.
    Without snapshots: full batches and one shorter last one."""
    n_iter, batch = int(n_iter), int(batch)
    if n_iter < 1 or batch < 1:
        raise ValueError("n_iter and batch must be >= 1")
    ends = [] if snapshot_iterations is None else sorted({int(k) + 1 for k in snapshot_iterations if 0 <= int(k) < n_iter})
    sizes, done, e = [], 0, 0
    while done < n_iter:
        while e < len(ends) and ends[e] <= done:
            e += 1
        end = min(done + batch, n_iter, ends[e] if e < len(ends) else n_iter)
        sizes.append(end - done)
        done = end
    return sizes


def _is_device_qt(nst):
    """scikit-learn's QuantileTransformer with normal output and one feature: the transformer gsm_qt_transform restates"""
    return (type(nst).__name__ == 'QuantileTransformer' and getattr(nst, 'output_distribution', None) == 'normal'
            and getattr(nst, 'quantiles_', None) is not None and nst.quantiles_.ndim == 2 and nst.quantiles_.shape[1] == 1)


def check_groups(chain, groups, n):
    """The `groups` argument of run_many_sgs checked against the template chain and the number of chains; touches neither a device
    nor a generator.  Returns None (no groups) or (of [n] int32, trend [G, H, W] float64 or None, nst_trans list of G or None).
    groups = dict(of=<n ints>, trend=<[G, H, W]>, nst_trans=<list of G>): chain c continues the large-scale bed of group of[c] and
    takes that group's trend and transformer, the way the reference's driver derives both from the bed it starts from
    (smallScaleChain_multiprocessing.py:479-496).  `trend` is needed exactly when the template has detrend_map, `nst_trans` exactly
    when it has do_transform; a group no chain names is allowed.
    ValueError: a missing or uncalled-for key, wrong shapes, `of` out of range, a non-finite trend, transformers whose n_quantiles_
    differ.  NotImplementedError: a transformer that is not scikit-learn's QuantileTransformer with normal output (the host-side
    kind has no grouped path)."""
    if groups is None:
        return None
    if not isinstance(groups, dict) or 'of' not in groups:
        raise ValueError("groups must be a dict with the key 'of' (the group of every chain) and 'trend' / 'nst_trans' as the template calls for")
    extra = set(groups) - {'of', 'trend', 'nst_trans'}
    if extra:
        raise ValueError(f"groups: unknown keys {sorted(extra)}")
    H, W = np.asarray(chain.xx).shape
    of = np.asarray(groups['of'])
    if of.ndim != 1 or of.shape[0] != n or of.dtype.kind not in 'iu':
        raise ValueError(f"groups['of'] must hold one integer per chain ({n})")
    want_trend, want_nst = bool(chain.detrend_map), bool(chain.do_transform)
    for key, want, flag in (('trend', want_trend, 'detrend_map'), ('nst_trans', want_nst, 'do_transform')):
        if want and groups.get(key) is None:
            raise ValueError(f"groups[{key!r}] is needed: the template chain has {flag}")
        if not want and groups.get(key) is not None:
            raise ValueError(f"groups[{key!r}] is given but the template chain has no {flag}")
    if not want_trend and not want_nst:
        raise ValueError("groups: the template chain has neither detrend_map nor do_transform, so nothing differs between groups")
    trend = nst = None
    G = None
    if want_trend:
        trend = np.asarray(groups['trend'], dtype=np.float64)
        if trend.ndim != 3 or trend.shape[1:] != (H, W) or trend.shape[0] < 1:
            raise ValueError(f"groups['trend'] must have shape (G, {H}, {W})")
        if not np.isfinite(trend).all():
            raise ValueError("groups['trend'] must be finite: the conditioning data must sit at the same cells in every group")
        G = trend.shape[0]
    if want_nst:
        nst = list(groups['nst_trans'])
        if len(nst) < 1 or (G is not None and len(nst) != G):
            raise ValueError("groups['nst_trans'] must hold one transformer per group" + (f" ({G})" if G is not None else ""))
        G = len(nst)
        if not all(_is_device_qt(t) for t in nst):
            raise NotImplementedError("groups: every transformer must be scikit-learn's fitted QuantileTransformer(output_distribution="
                                      "'normal') of one feature; a transformer called on the host has no grouped path")
        if len({int(t.quantiles_.shape[0]) for t in nst}) != 1:
            raise ValueError("groups['nst_trans']: the transformers' n_quantiles_ differ (the device holds one table length)")
    if of.size and (int(of.min()) < 0 or int(of.max()) >= G):
        raise ValueError(f"groups['of'] must lie in [0, {G})")
    return np.ascontiguousarray(of, dtype=np.int32), trend, nst


def slice_groups(groups, lo, hi):
    """The groups of chains lo .. hi - 1 (one rank's share): `of` of those chains renumbered densely in ascending order of the old
    numbers, and only the trends and transformers those chains name, in that order.  Pure host code; None stays None."""
    if groups is None:
        return None
    of = np.asarray(groups['of'])[lo:hi]
    used, new_of = np.unique(of, return_inverse=True)
    out = dict(of=new_of.astype(np.int32).reshape(-1))
    if groups.get('trend') is not None:
        out['trend'] = np.ascontiguousarray(np.asarray(groups['trend'])[used])
    if groups.get('nst_trans') is not None:
        out['nst_trans'] = [groups['nst_trans'][int(g)] for g in used]
    return out


def handoff(chain, lsc_beds, of, sigma=10, n_quantiles=1000, random_state=None, device=None, fit='host'):
    """From large-scale beds to small-scale chains, the lines of the reference's driver that sit between the two samplers
    (smallScaleChain_multiprocessing.py:479-496), once per large-scale bed:
        bed = where((surf - bed <= 0) & (grounded_ice_mask == 1), surf - 1, bed)       the bed clamped under the surface
        trend = gaussian_filter(bed, sigma)                                            trend_of: all beds in one device call
        nst = QuantileTransformer(n_quantiles, 'normal', subsample=None, random_state).fit((bed - trend).reshape(-1, 1))     on the host
    lsc_beds [G, H, W]: the final beds of a large-scale ensemble (run_many); of [n]: the large-scale bed each small-scale chain
    continues.  `chain` is the small-scale template (its surf and grounded_ice_mask are used; set detrend_map / do_transform on it
    as the run should have them: a key the template does not call for is left out of the dict).
    Returns (initial_beds, groups): initial_beds[c] is the clamped bed of group of[c], and run_many_sgs(chain, initial_beds, rngs,
    n_iter, groups=groups) continues every bed with its own trend and transformer.
    fit='host' (default): the transformers are fitted by scikit-learn, bed by bed.  fit='device': trend and transformers of all beds
    on the device (trend_of and fit_normal_scores with device=True, the detrended stack formed there by one fp64 subtraction per cell,
    NumPy's bits); the tables have the bits of the host fit of the same trend.  ValueError with device=False."""
    if fit not in ('host', 'device'):
        raise ValueError("handoff: fit must be 'host' or 'device'")
    if fit == 'device' and device is not None and not device:
        raise ValueError("handoff: fit='device' needs the device path (device=True or None)")
    beds = np.array(lsc_beds, dtype=np.float64)
    if beds.ndim != 3 or beds.shape[1:] != np.asarray(chain.xx).shape:
        raise ValueError("lsc_beds must have shape (G, H, W) of the chain's grid")
    of = np.asarray(of)
    if of.ndim != 1 or of.dtype.kind not in 'iu' or (of.size and (of.min() < 0 or of.max() >= beds.shape[0])):
        raise ValueError(f"`of` must hold integers in [0, {beds.shape[0]})")
    surf = np.asarray(chain.surf, dtype=np.float64)
    clamp = ((surf[None] - beds) <= 0) & (np.asarray(chain.grounded_ice_mask)[None] == 1)
    beds = np.where(clamp, surf[None] - 1, beds)
    groups = dict(of=np.ascontiguousarray(of, dtype=np.int32))
    if fit == 'device':
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("no ROCm/HIP device visible to torch: handoff(fit='device') has no CPU fallback")
        d_beds = torch.as_tensor(beds).to(torch.device("cuda", torch.cuda.current_device()))
        d_trend = trend_of(d_beds, sigma=sigma, device=True)
        if chain.detrend_map:
            groups['trend'] = d_trend.cpu().numpy()
        if chain.do_transform:
            groups['nst_trans'] = fit_normal_scores(d_beds - d_trend, n_quantiles=n_quantiles, random_state=random_state, device=True)
        return [beds[int(g)].copy() for g in of], groups
    trend = trend_of(beds, sigma=sigma, device=device)
    if chain.detrend_map:
        groups['trend'] = trend
    if chain.do_transform:
        from sklearn.preprocessing import QuantileTransformer
        groups['nst_trans'] = [QuantileTransformer(n_quantiles=n_quantiles, output_distribution='normal', subsample=None,
                                                   random_state=random_state).fit((b - t).reshape(-1, 1)) for b, t in zip(beds, trend)]
    return [beds[int(g)].copy() for g in of], groups


# The draws of some iterations as gsm_sgs_iterate / gsm_sgs_blocks_batch read them.  Device draws: views of a buffer set, blk the
# block records, cell counts in cnt, off_stride n.  Uploaded host draws: blk and cnt None, off_stride n + 1, cell_base on the host.
_Draws = namedtuple('_Draws', 'win blk off cnt cells z us off_stride cell_base')


class _SgsRun:
    """What run_many_sgs computes once per call, and the operations its three iteration drivers share.
    Host plan (no device needed): axes, hw, vario, lag extents and table, max_cells, trend, z_cond, cond_is_data, the transformer
    kind (None, 'device_qt': scikit-learn's on the device, 'host_nst': any other object, called on the host), keep_all, track,
    windowed, batch, grid_finite, the draw source ('replay', 'pcg64' or 'philox').
    Device state (None where it does not apply): cur / nxt / prop, resampled, d_loss / d_bad, d_lprev / d_acc, d_energy / d_state
    (windowed iteration end), d_q / d_ref (transformer tables), d_region / d_isdata, d_gen or d_seeds and the draw buffer sets.
    Records: loss_cache, step_cache, blocks_cache, bed_cache, sample_values.
    posterior (checked options or None): sizes, the batch sizes of the run (batch_plan: a snapshot iteration ends its batch), snap_its,
    accum (posterior.PosteriorAccumulator on this run's handle) and snap, the scratch tensor of a snapshot in bed units."""

    def __init__(self, chain, initial_beds, rngs, n_iter, only_save_last_bed, info_per_iter, progress_bar, device, source,
                 philox_seeds, philox_iter0, posterior=None, groups=None):
        from .engine import GsmEngine
        self._plan(chain, initial_beds, rngs, int(n_iter), only_save_last_bed, source, groups)
        self.info_per_iter, self.progress_bar, self.philox_iter0 = max(int(info_per_iter), 1), progress_bar, int(philox_iter0)
        self.snap_its = frozenset()
        if posterior is not None:
            from .posterior import snapshot_iterations
            self.snap_its = frozenset(int(k) for k in snapshot_iterations(self.n_iter, posterior['burn_in'], posterior['thin']))
        self.sizes = batch_plan(self.n_iter, self.batch, self.snap_its)
        self.accum = self.snap = None
        self.eng = GsmEngine(self.H, self.W, self.n, device)
        try:
            self._device_state(philox_seeds)
            if posterior is not None:
                self._posterior_state(posterior)
        except BaseException:
            self.eng.close()
            raise
        self.t0 = time.time()

    def close(self):
        self.eng.close()

    def _plan(self, chain, initial_beds, rngs, n_iter, only_save_last_bed, source, groups=None):
        """groups: None or check_groups' triple.  With more than one group, `of` [n] is the group of every chain, trend_g [G, H, W],
        z_cond [G, H, W] and the transformers hold one entry per group, and `trend` is the chains' own planes [n, H, W] (trend_g[of]);
        one group is the ungrouped run with that group's trend and transformer in the template's place."""
        H, W = chain.xx.shape
        n = len(initial_beds)
        self.of = self.trend_g = self.nst_g = None
        chain_trend, chain_nst = chain.trend, chain.nst_trans
        if groups is not None:
            of, trend_g, nst_g = groups
            if (trend_g.shape[0] if trend_g is not None else len(nst_g)) == 1:
                chain_trend, chain_nst = (trend_g[0] if trend_g is not None else chain_trend), (nst_g[0] if nst_g is not None else chain_nst)
            else:
                self.of, self.trend_g, self.nst_g = of, trend_g, nst_g
        self.chain, self.rngs, self.source, self.n, self.n_iter, self.H, self.W = chain, rngs, source, n, n_iter, H, W
        self.xs, self.ys, self.dx, self.dy = _axes(np.asarray(chain.xx, dtype=np.float64), np.asarray(chain.yy, dtype=np.float64))
        self.rad, self.npts = float(chain.sgs_param[1]), int(chain.sgs_param[0])
        self.hw = int(math.ceil(self.rad / abs(self.dx)))
        self.vario = chain._vario()
        self.lag_mi, self.lag_mj = lag_extents(self.hw, H, W)
        self.lag = lag_cov_table(self.vario, self.hw, self.dx, self.dy, self.lag_mi, self.lag_mj)
        self.max_cells = min(1024, max(1, (int(chain.block_max_x) - 1) * (int(chain.block_max_y) - 1)))
        nst = self.nst = chain_nst if chain.do_transform else None
        if self.of is None:
            self.trend = np.asarray(chain_trend, dtype=np.float64) if chain.detrend_map else None
            detrended = lambda a, c=None: np.asarray(a, dtype=np.float64) - self.trend if self.trend is not None else np.array(a, dtype=np.float64)
            cond_c = detrended(chain.cond_bed)
            self.z_cond = nst.transform(cond_c.reshape(-1, 1)).reshape(H, W) if nst is not None else cond_c
            self.cond_is_data = ~np.isnan(self.z_cond)
        else:
            # per group what the ungrouped run makes once: the conditioning data minus the group's trend, through the group's transformer
            G = self.trend_g.shape[0] if self.trend_g is not None else len(self.nst_g)
            self.trend = self.trend_g[self.of] if self.trend_g is not None else None
            detrended = lambda a, c=None: (np.asarray(a, dtype=np.float64) - (self.trend_g[c] if c is not None else 0.0)
                                           if self.trend_g is not None else np.array(a, dtype=np.float64))
            cond_g = [detrended(chain.cond_bed, g) for g in range(G)]
            self.z_cond = np.stack([self.nst_g[g].transform(cond_g[g].reshape(-1, 1)).reshape(H, W) if self.nst_g is not None else cond_g[g]
                                    for g in range(G)])
            data = ~np.isnan(self.z_cond)
            if not (data == data[0]).all():
                raise ValueError("groups: the conditioning data do not sit at the same cells in every group")
            self.cond_is_data = data[0]
            nst = self.nst = self.nst_g[0] if self.nst_g is not None else None      # stands for the kind; the tables are per group
        # scikit-learn's QuantileTransformer with normal output and one feature (what the reference's drivers attach,
        # smallScaleChain_multiprocessing.py:493-496) runs on the device (gsm_qt_transform); any other transformer object is
        # called on the host once per iteration, where the reference calls it
        if nst is None:
            self.transformer = None
        elif _is_device_qt(nst):
            self.transformer = 'device_qt'
        else:
            self.transformer = 'host_nst'
        self.track = chain.sample_loc is not None
        self.keep_all = not only_save_last_bed
        # no transformer: only the block and its one-cell halo change per iteration -> carried squared residuals, windowed loss,
        # and loss / guard / acceptance test / commit in ONE launch (gsm_sgs_finish); the reference recomputes the whole map
        # (gsm_sgs_finish keeps block + halo in LDS: 36 x 36 cells; a longer, thinner block takes the whole-map path)
        self.windowed = (nst is None and os.environ.get('GSM_SGS_WINDOWED', '1') != '0' and
                         (int(chain.block_max_x) + 1) * (int(chain.block_max_y) + 1) <= 1296)
        # Without a host-side transformer and without per-iteration bed records nothing of an iteration has to come back to the
        # host before the next one: the draws do not depend on the chain state (chain_sgs.run consumes chain.rng in the same order
        # whatever is accepted), so a batch of iterations is drawn ahead and simulated / scored / decided / committed on the device
        # back to back by ONE gsm_sgs_iterate call.  A batch ends with a host round trip (device flag, record download) and restarts
        # the pipeline of records made ahead -- with few chains 128 instead of 32 iterations per batch is +7 % (4 chains: 66.6 ->
        # 71.0 k chain-iterations/s); with the chip full it changes nothing and the draw buffers grow with batch x chains
        one_by_one = self.transformer == 'host_nst' or self.keep_all or self.track
        self.batch = 1 if one_by_one else int(os.environ.get('GSM_SGS_BATCH', '128' if n <= 64 else '32'))
        # two sets of draw buffers: the device draws of batch b + 1 (they depend on the generators only, never on the chains' state)
        # are made on their own stream while batch b iterates.
        # Only for few chains (4 chains, pcg64 mode: 38.7 -> 56.2 k chain-iterations/s): with the chip full (256 chains) the draw
        # kernel fits into the gap where the host downloads a batch's records, and drawing ahead measured 10 % slower (same box)
        self.draw_ahead = os.environ.get('GSM_SGS_DRAW_AHEAD', '1' if n <= 64 else '0') != '0'
        self.bed0 = np.stack([detrended(b, None if self.of is None else self.of[c]) for c, b in enumerate(initial_beds)])
        # no NaN in the beds (and none can appear: every cell of a block is simulated): gsm_sgs_iterate may then make the records of
        # iteration j + 1 while iteration j is still running (include/gsm.h: grid_finite).  GSM_SGS_OVERLAP=0 turns that off.
        self.grid_finite = os.environ.get('GSM_SGS_OVERLAP', '1') != '0' and bool(np.isfinite(self.bed0).all())
        # the transforms inside the launch that ends an iteration (include/gsm.h: tail_qt): GSM_SGS_TAIL_QT=0 never, any other value wherever they fit
        tail_env = os.environ.get('GSM_SGS_TAIL_QT')
        self.tail_qt = TAIL_QT_AUTO if tail_env is None else TAIL_QT_OFF if tail_env == '0' else TAIL_QT_ON
        # records; every driver starts at iteration 0 and overwrites the record of the initial state there (module docstring)
        self.loss_cache = np.zeros((n, n_iter)); self.step_cache = np.zeros((n, n_iter)); self.blocks_cache = np.full((n, n_iter, 4), np.nan)
        self.bed_cache = self.sample_values = self.ij = None
        if self.keep_all:
            self.bed_cache = np.zeros((n, n_iter, H, W))
            self.bed_cache[:, 0] = self.bed0
        if self.track:
            from .MCMC_gpu import chain_crf_gpu
            self.ij = chain_crf_gpu._sample_indices(chain)          # the large-scale chain's lookup: same attributes (xx, yy, sample_loc)
            self.sample_values = np.zeros((n, self.ij.shape[0], n_iter))
            for c in range(n):
                self.sample_values[c, :, 0] = np.asarray(initial_beds[c])[self.ij[:, 0], self.ij[:, 1]]

    def _device_state(self, philox_seeds):
        import torch
        chain, eng, n, H, W = self.chain, self.eng, self.n, self.H, self.W
        dev, f64 = eng.dev, eng._f64
        self.lib, self.dev = eng.lib, dev
        eng.set_static(chain.surf, chain.velx, chain.vely, chain.dhdt, chain.smb, None, chain.grounded_ice_mask,
                       chain.mc_region_mask, chain.resolution, chain.sigma_mc)
        self.d_xs, self.d_ys, self.d_lag, self.d_zcond = f64(self.xs), f64(self.ys), f64(self.lag), f64(self.z_cond)
        self.d_trend_n = None                                    # the chains' own trend planes [n, H, W] (snapshot)
        if self.of is None:
            self.d_trend = f64(self.trend) if self.trend is not None else None
        else:
            # chain groups: trend, z_cond and the transformer tables hold one plane / table per group and the handle knows each chain's group
            self.d_trend = f64(self.trend_g) if self.trend_g is not None else None
            eng._check(self.lib.gsm_sgs_set_groups(eng.h, self.of.ctypes.data_as(C.POINTER(C.c_int32)), int(self.z_cond.shape[0])))
        self.cur = f64(self.bed0)
        self.nxt = self.cur.clone()
        self.bed_host = self.bed0 if self.transformer == 'host_nst' else None     # host-side transformer: the chains' state lives here
        self.bed_next = None                                     # ... and its proposals in data space
        self.d_q = self.d_ref = self.prop = None
        self.nq = 0
        if self.transformer == 'device_qt':
            tabs = [self.nst] if self.of is None else self.nst_g
            self.d_q, self.d_ref = f64(np.stack([t.quantiles_[:, 0] for t in tabs])), f64(np.stack([t.references_ for t in tabs]))
            self.nq = int(self.d_q.shape[1])
            self.prop = self.cur.clone()                         # proposed beds in data space (inverse transform of nxt)
        self.resampled = torch.zeros((n, H, W), dtype=torch.int32, device=dev)
        self.d_loss = torch.empty(n, dtype=torch.float64, device=dev)
        self.d_bad = torch.empty(n, dtype=torch.int32, device=dev)
        st = torch.cuda.current_stream(dev)
        self.loss_prev, _ = self.loss(self.cur, st)
        self.loss_cache[:, 0] = self.loss_prev
        self.d_lprev = f64(self.loss_prev)
        self.d_acc = torch.empty(n, dtype=torch.uint8, device=dev)
        self.d_energy = self.d_state = None
        if self.windowed:
            self.d_energy = torch.empty((n, H, W), dtype=torch.float64, device=dev)
            self.d_state = torch.empty((n, 4), dtype=torch.float64, device=dev)
            eng.call(self.lib.gsm_sgs_state_init, self.cur, self.d_trend, self.d_energy, self.d_state, stream=st)
        self.d_gen = self.d_seeds = self.d_region = self.d_isdata = None
        self.draw_sets = []
        if self.source == 'replay':
            return
        if self.source == 'pcg64':
            self.d_gen = eng.pcg64_to_device(list(self.rngs))
        else:
            self.d_seeds = torch.as_tensor(np.asarray([int(x) & 0xFFFFFFFFFFFFFFFF for x in philox_seeds], dtype=np.uint64).view(np.int64)).to(dev)
        if chain.update_in_region:
            self.d_region = eng.mask_u8(chain.region_mask)
        self.d_isdata = torch.as_tensor(np.ascontiguousarray(self.cond_is_data, dtype=np.uint8)).to(dev)
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
        kn = min(self.batch, self.n_iter) * n
        for _ in range(2 if self.draw_ahead else 1):
            self.draw_sets.append(dict(win=i32(kn * 4), blk=i32(kn * 4), off=i32(kn), cnt=i32(kn), cells=i32(kn * self.max_cells, 2),
                                       z=torch.empty(kn * self.max_cells, dtype=torch.float64, device=dev),
                                       us=torch.empty(kn, dtype=torch.float64, device=dev)))

    def _posterior_state(self, opt):
        """The accumulator of the snapshots on this run's handle (set_static was called: `residual` has its fields).  Sample traces
        are taken at chain.sample_loc, of the beds in bed units."""
        import torch
        from .posterior import PosteriorAccumulator, default_common_ref
        chain, eng = self.chain, self.eng
        g = opt['common_ref'] if opt['common_ref'] is not None else default_common_ref(chain.initial_bed)
        self.accum = PosteriorAccumulator(eng, self.n_iter, opt['burn_in'], opt['thin'], split=opt['split'], rhat=opt['rhat'], common_ref=g,
                                          sample_cells=None if self.ij is None else self.ij[:, 0] * self.W + self.ij[:, 1],
                                          sample_loc=chain.sample_loc, hist=opt['hist'], ess=opt['ess'], cov=opt['cov'],
                                          residual=opt['residual'], local=opt['local'], regions=opt['regions'])
        if self.trend is not None or self.bed_host is not None:
            self.snap = torch.empty((self.n, self.H, self.W), dtype=torch.float64, device=self.dev)
        if self.of is not None and self.d_trend is not None:
            self.d_trend_n = self.d_trend[torch.as_tensor(self.of.astype(np.int64)).to(self.dev)]

    def snapshot(self, it, st):
        """If iteration `it` is a snapshot: the chains' state after its decision, in bed units (what store_bed keeps in
        bed_cache[:, it]), folded into the accumulator on stream st.  `cur` is detrended: cur + trend is ONE fp64 add on the device,
        the bits of NumPy's add; a host-side transformer's state is uploaded.  The caller orders st behind the iteration and ahead
        of whatever writes `cur` next."""
        if it not in self.snap_its:
            return
        import torch
        accum = self.accum
        with torch.cuda.stream(st):
            if self.bed_host is not None:
                self.snap.copy_(torch.as_tensor(self.bed_host + self.trend if self.trend is not None else self.bed_host))
            elif self.snap is not None:
                torch.add(self.cur, self.d_trend if self.d_trend_n is None else self.d_trend_n, out=self.snap)
            self.eng.beds = self.snap if self.snap is not None else self.cur
            ring = accum.ring
            accum.add()
            if ring is not None and accum.ring is None:          # released with the last snapshot: st still reads it
                ring.record_stream(st)

    # ---- the library calls, each on the stream it is given -----------------------------------------------------------------
    def qt(self, src, dst, inverse, st):
        self.eng.call(self.lib.gsm_qt_transform, self.d_q, self.d_ref, self.nq, src, dst, int(src.numel()), int(inverse), stream=st)

    def loss(self, t, st):
        """loss and thickness-guard flag per chain of the beds t (full grid), on the host"""
        self.eng.call(self.lib.gsm_sgs_loss, t, self.d_trend, self.d_loss, self.d_bad, stream=st)
        return self.d_loss.cpu().numpy().copy(), self.d_bad.cpu().numpy().copy()

    def check(self, st):
        self.eng.call(self.lib.gsm_sgs_check, stream=st)

    def draw(self, it0, kb, bs, st):
        """the device draws of iterations it0 .. it0 + kb - 1 into the buffer set bs"""
        d, ch = self.views(bs, kb), self.chain
        args = (kb, self.d_region, self.d_isdata, int(ch.block_min_x), int(ch.block_max_x), int(ch.block_min_y), int(ch.block_max_y),
                self.max_cells, d.win, d.blk, d.off, d.cnt, d.cells, d.z, d.us)
        if self.source == 'pcg64':
            self.eng.call(self.lib.gsm_sgs_draw_pcg64, self.d_gen, *args, stream=st)
        else:
            self.eng.call(self.lib.gsm_sgs_draw_philox, self.d_seeds, self.philox_iter0 + it0, *args, stream=st)
        return d

    def views(self, bs, kb):
        n = self.n
        return _Draws(win=bs['win'][:kb * n * 4].view(kb, n, 4), blk=bs['blk'][:kb * n * 4].view(kb, n, 4), off=bs['off'][:kb * n].view(kb, n),
                      cnt=bs['cnt'][:kb * n].view(kb, n), cells=bs['cells'], z=bs['z'], us=bs['us'][:kb * n].view(kb, n),
                      off_stride=n, cell_base=None)

    def host_draws(self, it0, kb):
        """the host draws of iterations it0 .. it0 + kb - 1 (block records stored), packed"""
        d, self.blocks_cache[:, it0:it0 + kb] = host_draws(self.chain, self.rngs, self.cond_is_data, it0, kb, self.n)
        return d

    def upload(self, d):
        """packed host draws on the device; the tuple keeps the tensors alive"""
        import torch
        up = lambda a: torch.as_tensor(a).to(self.dev)
        return _Draws(win=up(d['wins']), blk=None, off=up(d['offs']), cnt=None, cells=up(d['cells']), z=up(d['z']), us=up(d['us']),
                      off_stride=self.n + 1, cell_base=d['bases'])

    def make_batch(self, d, d_lrec, d_arec):
        """gsm_sgs_batch (include/gsm.h) of the iterations whose draws are d: the loop body of chain_sgs.run (MCMC.py:1741-1822) is
        issued by ONE gsm_sgs_iterate call."""
        from ._lib import SgsBatch
        b = SgsBatch()
        pv = lambda t: t.data_ptr() if t is not None else None
        b.cur, b.next, b.proposed = pv(self.cur), pv(self.nxt), pv(self.prop)
        b.zcond, b.trend = pv(self.d_zcond), pv(self.d_trend)
        b.qt_quantiles, b.qt_references, b.qt_n = pv(self.d_q), pv(self.d_ref), self.nq
        b.energy, b.state, b.windowed = pv(self.d_energy), pv(self.d_state), int(self.windowed)
        b.x_axis, b.y_axis, b.lag_cov = pv(self.d_xs), pv(self.d_ys), pv(self.d_lag)
        b.windows, b.cell_off, b.cell_cnt, b.cells, b.z, b.u = pv(d.win), pv(d.off), pv(d.cnt), pv(d.cells), pv(d.z), pv(d.us)
        b.cell_off_stride = d.off_stride
        if d.cell_base is not None:
            b.cell_base = d.cell_base.ctypes.data
        b.resampled, b.loss, b.bad, b.loss_prev, b.accept = pv(self.resampled), pv(self.d_loss), pv(self.d_bad), pv(self.d_lprev), pv(self.d_acc)
        b.loss_rec, b.acc_rec = pv(d_lrec), pv(d_arec)
        b.radius, b.sill = self.rad, float(self.vario["sill"])
        b.lag_mi, b.lag_mj, b.hw, b.num_points, b.max_cells = self.lag_mi, self.lag_mj, self.hw, self.npts, self.max_cells
        b.grid_finite, b.tail_qt = int(self.grid_finite), self.tail_qt
        return b

    def iterate(self, d, kb, d_lrec, d_arec, st):
        """kb iterations on the draws d, decided on the device; losses and accept flags into d_lrec / d_arec [n, kb]"""
        self.eng.call(self.lib.gsm_sgs_iterate, C.byref(self.make_batch(d, d_lrec, d_arec)), kb, stream=st)

    def simulate(self, d, st):
        """the blocks of ONE iteration simulated into nxt"""
        self.eng.call(self.lib.gsm_sgs_blocks_batch, self.nxt, self.d_zcond, d.win, self.d_xs, self.d_ys, self.d_lag, self.lag_mi, self.lag_mj,
                      self.hw, self.rad, self.npts, float(self.vario["sill"]), d.off, d.cnt, d.cells, d.z, self.max_cells, stream=st)

    # ---- records --------------------------------------------------------------------------------------------------------------
    def store(self, it0, kb, loss, acc, blocks=None):
        """the records [n, kb] of iterations it0 .. it0 + kb - 1 (blocks [kb, n, 4] as the device draws record them)"""
        self.loss_cache[:, it0:it0 + kb] = loss
        self.step_cache[:, it0:it0 + kb] = acc
        if blocks is not None:
            self.blocks_cache[:, it0:it0 + kb] = blocks.transpose(1, 0, 2)

    def beds_on_host(self):
        return self.bed_host if self.bed_host is not None else self.cur.cpu().numpy()

    def store_bed(self, it):
        """per-iteration bed and sample-point records (chain_sgs.run, MCMC.py:1814-1822)"""
        if not (self.keep_all or self.track):
            return
        bed_c = self.beds_on_host()
        if self.keep_all:
            self.bed_cache[:, it] = bed_c + self.trend if self.trend is not None else bed_c
        if self.track:
            for c in range(self.n):
                self.sample_values[c, :, it] = bed_c[c][self.ij[:, 0], self.ij[:, 1]]

    def progress(self, done):
        if self.progress_bar is None:
            return
        el = time.time() - self.t0
        print(f"Chain {getattr(self.chain, 'chain_id', 0)} ({str(getattr(self.chain, 'seed', 'Unknown'))[:6]}): "
              f"{100 * (done - 1) / max(self.n_iter - 1, 1):3.0f}% | it/s: {done / max(el, 1e-9):7.2f} | n: {self.n_iter} | "
              f"loss: {self.loss_cache[0, done - 1]:.3e} | acc: {self.step_cache[0, :done].sum() / done:.4f}", file=sys.stdout, flush=True)

    def results(self):
        """the reference's result tuple per chain; in pcg64 mode the generators continue where the device left them, as after NumPy calls"""
        bed_c = self.beds_on_host()
        res = self.resampled.cpu().numpy().astype(np.float64)
        if self.source == 'pcg64':
            for g, st in zip(self.rngs, self.eng.pcg64_from_device(self.d_gen)):
                g.bit_generator.state = st
        out = []
        for c in range(self.n):
            last = bed_c[c] + (self.trend if self.of is None else self.trend[c]) if self.trend is not None else bed_c[c]
            tup = (self.bed_cache[c] if self.keep_all else last, self.loss_cache[c].copy(), np.zeros(self.n_iter), self.loss_cache[c],
                   self.step_cache[c], res[c], self.blocks_cache[c])
            out.append(tup + (self.sample_values[c],) if self.track else tup)
        return out

    # ---- driver 1: device draws, batches decided on the device ---------------------------------------------------------------
    def drive_device_draws(self):
        """Batch b iterates on the side stream while (two buffer sets) batch b + 1 is drawn on the draw stream; with one set the next
        draws follow the batch's record download.  kb is 1 with per-iteration bed records."""
        import torch
        n, n_iter, sizes, dev, sets = self.n, self.n_iter, self.sizes, self.dev, self.draw_sets
        kmax = max(sizes)
        b_lrec = torch.empty(n * kmax, dtype=torch.float64, device=dev); b_arec = torch.empty(n * kmax, dtype=torch.uint8, device=dev)
        main = torch.cuda.current_stream(dev)
        side = torch.cuda.Stream(dev)
        side.wait_stream(main)
        draw_st = torch.cuda.Stream(dev) if len(sets) == 2 else side
        draw_st.wait_stream(main)
        self.draw(0, sizes[0], sets[0], draw_st)
        it_done = n_batch = 0
        while it_done < n_iter:
            kb = sizes[n_batch]
            d = self.views(sets[n_batch % len(sets)], kb)
            d_lrec, d_arec = b_lrec[:n * kb].view(n, kb), b_arec[:n * kb].view(n, kb)
            side.wait_stream(draw_st)                                  # this batch's draws
            nxt_kb = sizes[n_batch + 1] if n_batch + 1 < len(sizes) else 0
            if nxt_kb > 0 and len(sets) == 2:                          # the other set: the batch that used it is over (its records were downloaded)
                self.draw(it_done + kb, nxt_kb, sets[(n_batch + 1) % 2], draw_st)
            self.iterate(d, kb, d_lrec, d_arec, side)
            self.check(side)
            self.snapshot(it_done + kb - 1, side)                      # ahead of the next batch on the same stream
            with torch.cuda.stream(side):
                lrec_h, arec_h, blk_h = d_lrec.cpu().numpy(), d_arec.cpu().numpy(), d.blk.cpu().numpy()
            if nxt_kb > 0 and len(sets) == 1:
                self.draw(it_done + kb, nxt_kb, sets[0], draw_st)
            n_batch += 1
            self.store(it_done, kb, lrec_h, arec_h, blk_h)
            self.store_bed(it_done)                                    # kb == 1 where there is anything to store
            it_done += kb
            if it_done >= n_iter:
                main.wait_stream(side)
                main.wait_stream(draw_st)
            self.progress(it_done)

    # ---- driver 2: host draws, batches decided on the device, pipelined -------------------------------------------------------
    def drive_host_draw_batches(self):
        """The host draws of batch b + 1 are made while the device works on batch b (its launches are asynchronous): gsm_sgs_check
        and the record download of batch b come after the draws of b + 1."""
        import torch
        st = torch.cuda.current_stream(self.dev)
        running = self._launch(self.host_draws(0, self.sizes[0]), st)
        it_done = running[1]
        for kb in self.sizes[1:]:
            hd = self.host_draws(it_done, kb)                          # overlaps the device work of `running`
            self._finish(running, st)
            running = self._launch(hd, st)
            it_done += kb
        self._finish(running, st)

    def _launch(self, hd, st):
        """one batch of packed host draws uploaded and started; the returned tuple keeps its tensors alive until _finish"""
        import torch
        kb, d = hd['kb'], self.upload(hd)
        d_lrec = torch.empty((self.n, kb), dtype=torch.float64, device=self.dev)
        d_arec = torch.empty((self.n, kb), dtype=torch.uint8, device=self.dev)
        self.iterate(d, kb, d_lrec, d_arec, st)
        return hd['it0'], kb, d, d_lrec, d_arec

    def _finish(self, running, st):
        it0, kb, _, d_lrec, d_arec = running
        self.check(st)
        self.snapshot(it0 + kb - 1, st)                                # ahead of the next batch's launch
        self.store(it0, kb, d_lrec.cpu().numpy(), d_arec.cpu().numpy())
        self.progress(it0 + kb)

    # ---- driver 3: one iteration at a time, decided on the host ---------------------------------------------------------------
    def drive_one_by_one(self):
        """The loop of chain_sgs.run (MCMC.py:1741-1822) launch by launch: full-grid loss, acceptance test on the host.  The
        transformer kind picks the three operations around the simulation: to scores, score the proposal, commit."""
        import torch
        st = torch.cuda.current_stream(self.dev)
        to_scores, score_proposal, commit = {None: (self._plain_to_scores, self._plain_score, self._plain_commit),
                                             'device_qt': (self._qt_to_scores, self._qt_score, self._qt_commit),
                                             'host_nst': (self._host_to_scores, self._host_score, self._host_commit)}[self.transformer]
        for it in range(self.n_iter):
            if self.source == 'replay':
                hd = self.host_draws(it, 1)
                d, wins, us = self.upload(hd), hd['wins'][0], hd['us'][0]
            else:
                d = self.draw(it, 1, self.draw_sets[0], st)
                wins, us = d.win.cpu().numpy()[0], d.us.cpu().numpy()[0]
                self.blocks_cache[:, it] = d.blk.cpu().numpy()[0]
            to_scores(st)
            self.simulate(d, st)
            self.check(st)
            loss_next, bad = score_proposal(st)
            loss_next = np.where(bad > 0, np.inf, loss_next)
            with np.errstate(over='ignore', invalid='ignore'):
                # np.fmin: a NaN exponential gives 1, as the reference's built-in min(1, nan) and the device's decision
                p_acc = np.where(self.loss_prev > loss_next, 1.0, np.fmin(1.0, np.exp(self.loss_prev - loss_next)))
            acc = us <= p_acc
            commit(d, wins, acc, torch.as_tensor(acc.astype(np.uint8)).to(self.dev), st)
            self.loss_prev = np.where(acc, loss_next, self.loss_prev)
            self.store(it, 1, self.loss_prev[:, None], acc[:, None])
            self.store_bed(it)
            self.snapshot(it, st)
            if it % self.info_per_iter == 0 or it == self.n_iter - 1:
                self.progress(it + 1)

    def _plain_to_scores(self, st):
        pass                                                            # no transformer: nxt holds the beds themselves

    def _plain_score(self, st):
        return self.loss(self.nxt, st)

    def _plain_commit(self, d, wins, acc, d_acc, st):
        self.eng.call(self.lib.gsm_sgs_commit, self.cur, self.nxt, self.resampled, d.win, d_acc, stream=st)

    def _qt_to_scores(self, st):
        self.qt(self.cur, self.nxt, 0, st)

    def _qt_score(self, st):
        self.qt(self.nxt, self.prop, 1, st)
        return self.loss(self.prop, st)

    def _qt_commit(self, d, wins, acc, d_acc, st):
        self.eng.call(self.lib.gsm_sgs_commit_map, self.cur, self.prop, self.resampled, d.win, d_acc, stream=st)

    def _host_maps(self, fn, beds):
        return np.stack([fn(beds[c].reshape(-1, 1)).reshape(self.H, self.W) for c in range(self.n)])

    def _host_to_scores(self, st):
        self.nxt.copy_(self.eng._f64(self._host_maps(self.nst.transform, self.bed_host)))       # the caller's transformer on the whole map (MCMC.py:1766)

    def _host_score(self, st):
        self.bed_next = self._host_maps(self.nst.inverse_transform, self.nxt.cpu().numpy())        # MCMC.py:1777
        return self.loss(self.eng._f64(self.bed_next), st)

    def _host_commit(self, d, wins, acc, d_acc, st):
        for c in np.flatnonzero(acc):
            self.bed_host[c] = self.bed_next[c]
            r0, r1, c0, c1 = wins[c]
            self.resampled[c, r0:r1, c0:c1] += 1


def run_many_sgs(chain, initial_beds, rngs, n_iter, only_save_last_bed=True, info_per_iter=100, progress_bar=None, device=None,
                 philox_seeds=None, philox_iter0=0, pcg64=False, posterior=None, return_accumulator=False, groups=None):
    """n small-scale chains of one template (same static fields, variogram, block sizes) in ONE handle.  rngs: one NumPy
    Generator per chain (consumed exactly as chain_sgs.run consumes chain.rng).  philox_seeds (one 64-bit key per chain): Philox
    mode -- the draws of iterations philox_iter0 .. are made on the device and rngs are not touched.  pcg64=True: the draws of
    replay mode (rngs' own PCG64 streams, bit for bit) are made on the device and the generators are left where NumPy would leave
    them.
    Returns (list of result tuples, rngs).

    posterior: None, or the dict of MCMC_gpu.run_many (`burn_in`, `thin` and optionally `split`, `rhat`, `common_ref`, `hist`, `ess`,
    `cov`, `residual`, `local`; mcmc_gpu_amd/posterior.py), in every draw mode and with every transformer kind.  Snapshot k, for the
    iterations k = burn_in, burn_in + thin, ... < n_iter, is all chains' state after iteration k's decision in bed units, trend
    included: the bed that only_save_last_bed=False stores at bed_cache[:, k].  A snapshot iteration ends its batch (batch_plan) and
    is folded into the accumulators on the device where the batch ran; no bed comes to the host for it.  `common_ref` defaults to
    the template's initial bed, `residual` uses the template's static fields.  With chain.sample_loc set the summary's
    sample_values [n, points, T] are the thinned traces of those beds, trend included, while the per-iteration sample_values of
    the result tuples stay the detrended values they are without `posterior` (and, as without it, sample points mean one
    iteration per batch).  The call then returns (results, rngs,
    PosteriorSummary), or with return_accumulator=True the PosteriorAccumulator in place of the summary: its local_sums(),
    sample_values(), projections() and finalize() are readable after the call, to be merged over ranks first.  The chains are
    those of the run without `posterior`: beds, accept masks, blocks, counts and generator states bit for bit; the losses bit for
    bit with device draws and to the agreement of the batched with the one-by-one path (1e-12 relative) with host draws.

    groups: None, or dict(of=<n ints>, trend=<[G, H, W]>, nst_trans=<list of G>) -- chains that continue DIFFERENT large-scale beds
    in this one handle (check_groups has the rules; sgs.handoff makes the dict from a run_many ensemble).  Chain c is detrended with
    trend[of[c]], transformed with nst_trans[of[c]] and conditioned on the data as that pair transforms them, everywhere the
    ungrouped run uses the template's trend and transformer: initial beds and conditioning scores, the loss and the guard, both
    transforms, the posterior snapshots, the stored beds and the returned beds.  Every chain is, bit for bit, the chain of a
    run_many_sgs call on its group alone with a template set up with that group's trend and transformer (losses to 1e-12 relative
    with host draws, as above).  All draw modes, drivers and `posterior`; one group is the run without groups on that group's trend
    and transformer.  Refused before a handle exists or a generator is touched (check_groups)."""
    n = len(initial_beds)
    groups = check_groups(chain, groups, n)
    if len(rngs) != n:
        raise ValueError('need one random generator per chain')
    if pcg64 and philox_seeds is not None:
        raise ValueError("choose one of philox_seeds / pcg64")
    if philox_seeds is not None and len(philox_seeds) != n:
        raise ValueError('need one Philox seed per chain')
    if posterior is not None:
        from .posterior import check_options
        posterior = check_options(posterior, n_iter, n_chains=n)
    source = 'pcg64' if pcg64 else 'philox' if philox_seeds is not None else 'replay'
    run = _SgsRun(chain, initial_beds, rngs, n_iter, only_save_last_bed, info_per_iter, progress_bar, device, source, philox_seeds, philox_iter0,
                  posterior=posterior, groups=groups)
    try:
        if run.source != 'replay' and run.transformer != 'host_nst':
            run.drive_device_draws()                 # batch is 1 with keep_all / track
        elif run.source == 'replay' and run.batch > 1:
            run.drive_host_draw_batches()            # batch is 1 with a host-side transformer, keep_all / track or GSM_SGS_BATCH=1
        else:
            run.drive_one_by_one()                   # a host-side transformer in any draw mode; replay with batch 1
        if run.accum is None:
            return run.results(), rngs
        if return_accumulator:
            run.accum.partials()                     # made while the handle is open; the accumulator keeps them
            return run.results(), rngs, run.accum
        return run.results(), rngs, run.accum.finalize()
    finally:
        run.close()


def init_msc_chain_by_instance(param_dict):
    """Rebuild a small-scale chain from a copy of another one's __dict__ (+ 'rng_seed', 'initial_bed') (MCMC.py:402-431)."""
    p = param_dict
    ch = chain_sgs_gpu(p['xx'], p['yy'], p['initial_bed'], p['surf'], p['velx'], p['vely'], p['dhdt'], p['smb'], p['cond_bed'],
                       p['data_mask'], p['grounded_ice_mask'], p['resolution'])
    ch.update_in_region = p['update_in_region']
    ch.region_mask = p['region_mask']
    ch.sigma_mc = p['sigma_mc']
    ch.mc_region_mask = p['mc_region_mask']
    ch.block_min_x, ch.block_min_y = p['block_min_x'], p['block_min_y']
    ch.block_max_x, ch.block_max_y = p['block_max_x'], p['block_max_y']
    ch.do_transform = p['do_transform']
    ch.nst_trans = deepcopy(p['nst_trans'])
    ch.trend = p['trend']
    ch.detrend_map = p['detrend_map']
    ch.vario_type = p['vario_type']
    ch.vario_param = deepcopy(p['vario_param'])
    ch.sgs_param = deepcopy(p['sgs_param'])
    ch.rng = np.random.default_rng(seed=p['rng_seed'])
    ch.rng_seed = p['rng_seed']
    ch.sample_loc = deepcopy(p['sample_loc'])
    return ch
