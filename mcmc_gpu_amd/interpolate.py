"""Device mirror of gstatsim_custom.interpolate (gstatsMCMC/gstatsim_custom/interpolate.py): sequential Gaussian simulation of a
whole grid (sgs, :92-191), the step that makes the chains' initial beds (T2_StatisticalAnalysis.ipynb calls it once per seed),
and its deterministic twin, the kriging estimate and spread on the whole grid (krige, :13-89).

    sgs           interpolate.sgs's arguments and return value, plus `device`
    sgs_many      many realisations in one call, row r == sgs(..., seed=seeds[r]) bit for bit
    krige         interpolate.krige's arguments and return value, plus `device`
    krige_scores  the same call in normal-score space: estimate, variance and neighbour count per cell
    cross_validate  every measured cell kriged from the others under a hold-out (leave-one-out, a buffer, folds from
                  block_folds / random_folds), several candidate variograms per call (gsm_krige_cv, csrc/krige_cv_kernel.hip);
                  not in the reference

The generator is consumed as the reference consumes it, in its order -- one rng.shuffle of the cells of sim_mask, then one
standard normal per simulated cell (rng.normal(est, sd, 1) = est + sd * z) or, with bounds, one uniform per simulated cell whose
bounds differ (truncnorm.rvs = truncnorm.ppf(uniform, a, b) * scale + est) -- and the normal-score transform with
scikit-learn (utilities.gaussian_transformation, the same call) is made on the host.  The shuffle and the draws are NumPy's own
on the host (mode='replay', the default) or the same PCG64 stream advanced on the device, all realisations side by side
(mode='pcg64': gsm_sgs_grid_draw_pcg64, csrc/sgs_grid_draw_kernel.hip), bit for bit either way.  Neighbour search, kriging
and the sequential value pass run on the device (gsm_sgs_grid, csrc/sgs_grid_kernel.hip); nothing is computed on the CPU in
their place.  Kriging has no
generator and no sequence -- every cell conditions on the measured values alone -- so all its cells are searched, solved and
finished side by side in one kernel (gsm_krige_grid, csrc/krige_grid_kernel.hip).

Numerics: the kriging systems are solved by Gauss-Jordan elimination where the reference calls numpy.linalg.lstsq, and the
truncated-normal ppf is a restatement of scipy's (csrc/truncnorm.h), so values agree with the reference to ~1e-9 of the
normal-score scale, not bit for bit.  Equidistant neighbour candidates are taken in ascending (row, col); the reference's
argsort is unstable there.

Variogram: every parameter (major_range, minor_range, azimuth, sill, nugget) is a number or a map of the grid's shape, in any
mix, as in the reference (non-stationary SGS / kriging: the system of a cell is built from the parameters at that cell,
interpolate.py:56-62, :141-147).  All numbers: one covariance table per call, made on the host, any of the four models.  As
soon as one parameter is a map the call goes through gsm_sgs_grid_local / gsm_krige_grid_local: the host makes a six-number
row per cell (_local_table: the rotation matrix in the reference's arithmetic, sill, nugget) and the kernels evaluate every
covariance from the coordinates -- exponential, gaussian and spherical; Matern needs Bessel K, which the device does not have.
The reference's gaussian model has no nugget on the diagonal (covariance.py:8-10: its "nugget" scales the model), so with
ranges of many cells its systems are near singular, in the reference as here.

Grids: axis-aligned with uniform spacing; either axis may ascend or descend (north-up rasters) and the cells need not be
square (tests/test_gpu_interp_sgs_geometry.py: both signs of both axes, |dy| / |dx| from 0.5 to 2).
"""
from __future__ import annotations

import ctypes as C
import math
import numbers

import numpy as np

from .sgs import _axes, _generator, lag_cov_table

__all__ = ["sgs", "sgs_many", "krige", "krige_scores", "cross_validate", "CrossValidation", "block_folds", "random_folds"]

RECORD_BYTES = 800          # one path cell's record on the device: 48 (value, weight) pairs + a 32-byte header
WIDEN_STEP = 100e3          # interpolate.py:155


def _sanity_checks(xx, yy, grid, vario, radius, num_points, ktype, sim_mask):
    """The argument errors of interpolate._sanity_checks (interpolate.py:265-330), same types and messages."""
    for name, a in (("xx", xx), ("yy", yy), ("grid", grid)):
        if not isinstance(a, np.ndarray) or a.ndim != 2:
            raise ValueError(f"{name} must be a 2D NumPy array")
    if xx.shape != yy.shape or xx.shape != grid.shape:
        raise ValueError("xx, yy, and grid must have same shape")
    missing = [k for k in ("major_range", "minor_range", "azimuth", "sill", "nugget", "vtype") if k not in vario.keys()]
    if missing:
        raise ValueError(f"Variogram missing {', '.join(missing)}")
    if vario["vtype"].lower() not in ("matern", "exponential", "gaussian", "spherical"):
        raise ValueError("vtype must be exponential, gaussian, spherical, or matern")
    if vario["vtype"].lower() == "matern" and "s" not in vario.keys():
        raise ValueError("Matern covariance requires the s parameter in the variogram")
    if sim_mask is not None:
        if not isinstance(sim_mask, np.ndarray):
            raise ValueError("sim_mask must be None or a 2D array")
        if sim_mask.shape != grid.shape:
            raise ValueError("sim_mask shape must be same as grid if provided")
    for k, v in vario.items():
        if k == "vtype":
            continue
        if isinstance(v, numbers.Number):
            if np.isnan(v):
                raise ValueError(f"variogram parameter {k} is NaN")
        elif isinstance(v, np.ndarray):
            bad = np.isnan(v) if sim_mask is None else (sim_mask == True) & np.isnan(v)  # noqa: E712
            if np.count_nonzero(bad) > 0:
                raise ValueError(f"Variogram parameter {k} contains NaN" + ("" if sim_mask is None else " in sim_mask"))
    if not isinstance(radius, numbers.Number):
        raise ValueError("radius must be a number")
    if not isinstance(num_points, numbers.Number):
        raise ValueError("num_points must be a number")
    if ktype not in ("ok", "sk"):
        raise ValueError("ktype must be 'ok' or 'sk'")


class _Plan:
    """Everything of one call that does not depend on the seed: the fitted transformer, the grid in normal-score space, the
    transformed bounds and the cells of sim_mask in the reference's (C) order."""

    def __init__(self, xx, yy, grid, variogram, radius, num_points, ktype, sim_mask, stencil, rcond, bounds):
        from sklearn.preprocessing import QuantileTransformer
        _sanity_checks(xx, yy, grid, variogram, radius, num_points, ktype, sim_mask)
        if stencil is not None or rcond is not None:
            raise NotImplementedError("the device SGS searches the circular stencil and solves with lstsq's default cut-off "
                                      "(stencil=None, rcond=None)")
        self.local = None
        if any(isinstance(v, np.ndarray) for k, v in variogram.items() if k != "vtype"):
            self.local = _local_table(variogram, grid.shape)
        if not 8 <= int(num_points) <= 48:
            raise NotImplementedError("the device SGS takes 8 <= num_points <= 48")
        grid = np.asarray(grid, dtype=np.float64)
        self.H, self.W = grid.shape
        self.cond = ~np.isnan(grid)
        if not self.cond.any():
            raise ValueError("grid holds no conditioning value (the reference's neighbour search would widen for ever)")
        # utilities.gaussian_transformation (utilities.py:7-25)
        self.nst = QuantileTransformer(n_quantiles=500, output_distribution="normal").fit(grid[self.cond].reshape(-1, 1))
        self.grid_ns = np.full(grid.shape, np.nan)
        np.place(self.grid_ns, self.cond, self.nst.transform(grid[self.cond].reshape(-1, 1)).squeeze())
        self.global_mean = float(np.mean(self.grid_ns[self.cond]))
        self.bounds = None if bounds is None else self._bounds(bounds, xx.shape)
        if sim_mask is None:
            sim_mask = np.full(xx.shape, True)
        ii, jj = np.meshgrid(np.arange(self.H), np.arange(self.W), indexing="ij")
        self.inds = np.array([ii[sim_mask].flatten(), jj[sim_mask].flatten()]).T
        self.xs, self.ys, self.dx, self.dy = _axes(np.asarray(xx, dtype=np.float64), np.asarray(yy, dtype=np.float64))
        self.vario = None if self.local is not None else {k: (v if k == "vtype" else float(v)) for k, v in variogram.items()}
        self.vtype = variogram["vtype"].lower()
        self.radius, self.num_points, self.ktype = float(radius), int(num_points), ktype

    def _bounds(self, bounds, shape):
        """interpolate._preprocess's bounds (interpolate.py:240-261): a number is transformed and broadcast, an array of the
        grid's shape is transformed cell by cell; any other input is the reference's ValueError."""
        try:
            if len(bounds) != 2:
                raise ValueError
            out = []
            for b in bounds:
                if isinstance(b, numbers.Number):
                    out.append(np.full(shape, self.nst.transform(np.array([b]).reshape(-1, 1)).squeeze()))
                elif isinstance(b, np.ndarray):
                    if b.shape != shape:
                        raise ValueError
                    out.append(self.nst.transform(b.reshape(-1, 1)).reshape(shape))
                else:
                    raise ValueError
        except Exception:
            raise ValueError("bounds must be None or a 2D numpy array") from None
        return np.ascontiguousarray(out[0], dtype=np.float64), np.ascontiguousarray(out[1], dtype=np.float64)

    def draws(self, rng):
        """Consume `rng` as interpolate.sgs does: (path of flat cell indices, one number per path cell)."""
        inds = self.inds.copy()
        rng.shuffle(inds)                                                            # interpolate.py:127
        flat = inds[:, 0] * self.W + inds[:, 1]
        path = flat[~self.cond.ravel()[flat]]
        if self.bounds is None:
            d = rng.standard_normal(path.size)                                       # rng.normal(est, sd, 1), :174
        else:
            lo, hi = self.bounds
            live = lo.ravel()[path] != hi.ravel()[path]                              # lo == hi: no draw, :181-182
            d = np.zeros(path.size)
            d[live] = rng.random(int(live.sum()))                                    # truncnorm.rvs: uniform(size=1), :185
        return np.ascontiguousarray(path, dtype=np.int32), d


LOCAL_KEYS = ("major_range", "minor_range", "azimuth", "sill", "nugget")
LOCAL_VTYPES = {"exponential": 0, "gaussian": 1, "spherical": 2}            # GSM_VTYPE_* (include/gsm.h)


def _local_table(variogram, shape):
    """The per-cell table of gsm_sgs_grid_local / gsm_krige_grid_local, [H * W, 6] = R00, R01, R10, R11, sill, nugget per cell,
    for a variogram of which at least one parameter is a map.  interpolate._preprocess (interpolate.py:226-231) broadcasts the
    numbers to the grid's shape and the cell loop picks every parameter at the visited cell (:141-147); R is
    make_rotation_matrix(azimuth, major_range, minor_range) (_krige.py:83-103) in the reference's NumPy arithmetic -- theta =
    (azimuth / 180.0) * pi, [[cos, -sin], [sin, cos]] . diag(1 / major, 1 / minor) -- so that the device takes no sine.  The
    dot product's second terms are exact zeros: R00 = cos * (1 / major), R01 = -sin * (1 / minor), R10 = sin * (1 / major),
    R11 = cos * (1 / minor), the bits of oracle/mcmc_oracle.rotation_matrix cell by cell (tests/test_nonstationary_host.py)."""
    if variogram["vtype"].lower() == "matern":
        raise NotImplementedError("the device has no Bessel K: with vtype 'matern' it takes scalar variogram parameters only (one "
                                  "covariance table per call, made on the host); parameter maps take vtype exponential, gaussian "
                                  "or spherical")
    f = {}
    for k in LOCAL_KEYS:
        v = variogram[k]
        if isinstance(v, np.ndarray):
            if v.shape != tuple(shape):
                raise ValueError(f"variogram parameter {k} has shape {v.shape}, the grid {tuple(shape)}")
            f[k] = np.asarray(v, dtype=np.float64)
        else:
            f[k] = np.full(shape, v, dtype=np.float64)                                # interpolate.py:229-231
    with np.errstate(all="ignore"):                                                  # cells outside sim_mask may hold NaN
        th = (f["azimuth"] / 180.0) * np.pi
        c, sn = np.cos(th), np.sin(th)
        inv_major, inv_minor = 1 / f["major_range"], 1 / f["minor_range"]
        out = np.stack([c * inv_major, -sn * inv_minor, sn * inv_major, c * inv_minor, f["sill"], f["nugget"]], axis=-1)
    return np.ascontiguousarray(out.reshape(-1, 6))


def _window_rows(ys, dx, dy):
    """Row coordinates on which the Euclidean distance to a value bounds the reference's search from above.  A search finds a
    value when it lies within the radius AND within hw = ceil(radius / |dx|) cells of the cell in rows and in columns
    (neighbors.py:4-64 scans that window only).  Columns: |dj| |dx| <= d < radius <= hw |dx| always.  Rows: only while
    |dy| >= |dx|; with closer rows a value can be inside the radius and outside the window.  On rows spread to |dx| apart,
    d' = sqrt(dx_^2 + (di |dx|)^2) >= max(d, |di| |dx|), so d' < radius puts the value inside both."""
    if abs(dy) >= abs(dx):
        return ys
    return np.arange(ys.size, dtype=np.float64) * abs(dx)


def _lag_extents_from(d, radius, dx, H, W):
    """Lag table extents (rows, columns) from d, the distance (on _window_rows) of every cell to simulate to the nearest
    conditioning value: a cell's search widens by 100 km at most k times, k the least number with d < radius + 100 km k, and the
    window of that search is ceil(r / |dx|) cells either way, so two chosen neighbours are at most twice that apart."""
    d_max = float(np.max(d)) if np.size(d) else 0.0
    k = 0 if d_max < radius else int(math.floor((d_max - radius) / WIDEN_STEP)) + 1
    r_max = radius + WIDEN_STEP * k
    hw_max = int(math.ceil(r_max / abs(dx))) + 1
    return min(2 * hw_max, H - 1), min(2 * hw_max, W - 1)


def _lag_extents(plan, eng, torch):
    """Lag table extents that the radius widening never runs off (_lag_extents_from), the distances from
    gsm_min_dist_from_mask."""
    H, W = plan.H, plan.W
    dev = eng.dev
    ys = _window_rows(plan.ys, plan.dx, plan.dy)
    xx = torch.as_tensor(np.ascontiguousarray(np.broadcast_to(plan.xs[None, :], (H, W)))).to(dev)
    yy = torch.as_tensor(np.ascontiguousarray(np.broadcast_to(ys[:, None], (H, W)))).to(dev)
    mask = torch.as_tensor(plan.cond.astype(np.uint8).ravel()).to(dev)
    dist = torch.empty(H * W, dtype=torch.float64, device=dev)
    eng.call(eng.lib.gsm_min_dist_from_mask, xx, yy, mask, dist)
    return _lag_extents_from(dist.cpu().numpy()[~plan.cond.ravel()], plan.radius, plan.dx, H, W)


def _segment_cells(R, max_path, torch, dev, extra_bytes):
    free, _ = torch.cuda.mem_get_info(dev)
    budget = (free - extra_bytes) // 2
    s = int(budget // (R * RECORD_BYTES)) // 64 * 64
    if s < 64:
        raise MemoryError(f"not enough device memory for 64 path slots of records x {R} realisations")
    return max(64, min(s, (max_path + 63) // 64 * 64))


def _kriging_operands(plan, eng, torch, n_grids):
    """What gsm_sgs_grid* and gsm_krige_grid* take alike, uploaded to the device of `eng`: the axes, the variogram -- one lag
    covariance table that the radius widening never runs off (_lag_extents), or the plan's per-cell table -- and the global mean
    of each of the handle's n_grids grids, handed to gsm_sgs_set_kriging with the plan's kriging type.  Returns (axes, suffix,
    operands, keep): lib.gsm_sgs_grid + suffix (or gsm_krige_grid + suffix) is called with (..., *axes, *operands, ...); `keep`
    holds the device arrays until the call is over."""
    from .engine import _ptr
    f64 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(eng.dev)
    hw = int(math.ceil(plan.radius / abs(plan.dx)))
    if plan.local is None:
        mi, mj = _lag_extents(plan, eng, torch)
        if (2 * mi + 1) * (2 * mj + 1) * 8 > torch.cuda.mem_get_info(eng.dev)[0] // 4:
            raise MemoryError(f"the lag covariance table for the widest search radius ({2 * mi + 1} x {2 * mj + 1} lags) does not "
                              "fit the device; raise `radius` or add conditioning data")
        d_vario = f64(lag_cov_table(plan.vario, hw, plan.dx, plan.dy, mi, mj))
        suffix, operands = "", (_ptr(d_vario), mi, mj, hw, plan.radius, plan.num_points, float(plan.vario["sill"]))
    else:
        d_vario = f64(plan.local)                                                     # a variogram per cell: no table
        suffix, operands = "_local", (_ptr(d_vario), LOCAL_VTYPES[plan.vtype], hw, plan.radius, plan.num_points)
    d_xs, d_ys, d_gm = f64(plan.xs), f64(plan.ys), f64(np.full(n_grids, plan.global_mean))
    with torch.cuda.device(eng.dev):
        eng._check(eng.lib.gsm_sgs_set_kriging(eng.h, 1 if plan.ktype == "sk" else 0, _ptr(d_gm)))
    return (_ptr(d_xs), _ptr(d_ys)), suffix, operands, (d_xs, d_ys, d_vario, d_gm)


MODES = ("replay", "pcg64")


def _check_mode(mode, gens):
    """The ValueErrors of the `mode` keyword, raised before any device work."""
    if mode not in MODES:
        raise ValueError(f"mode must be 'replay' or 'pcg64', not {mode!r}")
    if mode != "pcg64":
        return
    for g in gens:
        if g.bit_generator.state.get("bit_generator") != "PCG64":
            raise ValueError("mode 'pcg64' needs numpy.random.Generator(PCG64) generators (numpy.random.default_rng); "
                             f"got {type(g.bit_generator).__name__}")
    if len({id(g.bit_generator) for g in gens}) != len(gens):
        raise ValueError("mode 'pcg64' advances the generators of `seeds` side by side on the device: the same Generator listed "
                         "twice is one sequential stream (mode 'replay' consumes it row after row)")


def _device_draws(plan, gens, eng, torch, d_lo, d_hi):
    """mode 'pcg64': _Plan.draws of every generator on the device (gsm_sgs_grid_draw_pcg64), the generators left where NumPy would
    leave them.  d_lo, d_hi: the transformed bounds on the device, or None.  Returns the device arrays gsm_sgs_grid takes -- path
    [R * path_len], path_off [R + 1], draws [R * path_len] -- and path_len: every path filters the same cells by the same mask."""
    dev, R = eng.dev, len(gens)
    flat = np.ascontiguousarray(plan.inds[:, 0] * plan.W + plan.inds[:, 1], dtype=np.int32)
    path_len = int(np.count_nonzero(~plan.cond.ravel()[flat]))
    d_states = eng.pcg64_to_device(gens)
    d_cells = torch.as_tensor(flat).to(dev)
    d_has = torch.as_tensor(plan.cond.astype(np.uint8).ravel()).to(dev)
    d_work = torch.empty(max(1, R * flat.size), dtype=torch.int32, device=dev)
    d_path = torch.empty(max(1, R * path_len), dtype=torch.int32, device=dev)
    d_draw = torch.empty(max(1, R * path_len), dtype=torch.float64, device=dev)
    eng.call(eng.lib.gsm_sgs_grid_draw_pcg64, d_states, d_cells, int(flat.size), d_has, d_lo, d_hi, 1 if plan.bounds is not None else 0,
             d_work, d_path, d_draw, path_len)
    for g, st in zip(gens, eng.pcg64_from_device(d_states)):
        g.bit_generator.state = st
    d_off = torch.arange(R + 1, dtype=torch.int64, device=dev) * path_len
    return d_path, d_off, d_draw, path_len


def _run(plan, gens, segment_cells=None, device=None, trace=False, mode="replay"):
    """Draw for every generator -- mode 'replay': on the host, in turn; 'pcg64': on the device, side by side (_device_draws) --
    and simulate all realisations in one gsm_sgs_grid call.  Returns the normal-score grids [R, H, W] and, with trace,
    (paths, traces [total, 3])."""
    import torch
    from .engine import GsmEngine, _ptr
    _check_mode(mode, gens)
    R, H, W = len(gens), plan.H, plan.W
    if mode == "replay":
        plans = [plan.draws(g) for g in gens]
        lens = np.array([p.size for p, _ in plans], dtype=np.int64)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        max_path = int(lens.max()) if R else 0
        total = int(off[-1])
    eng = GsmEngine(H, W, R, device)
    try:
        dev, lib, h = eng.dev, eng.lib, eng.h
        f64 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
        d_lo = d_hi = None
        if plan.bounds is not None:
            d_lo, d_hi = f64(plan.bounds[0]), f64(plan.bounds[1])
        if mode == "pcg64":
            d_path, d_off, d_draw, max_path = _device_draws(plan, gens, eng, torch, d_lo, d_hi)
            total = R * max_path
        axes, suffix, operands, keep = _kriging_operands(plan, eng, torch, R)
        grids = f64(plan.grid_ns)[None].repeat(R, 1, 1).contiguous()
        if mode == "replay":
            d_path = torch.as_tensor(np.concatenate([p for p, _ in plans])).to(dev)
            d_off = torch.as_tensor(off).to(dev)
            d_draw = f64(np.concatenate([d for _, d in plans]))
        d_tr = torch.zeros((total, 3), dtype=torch.float64, device=dev) if trace else None
        if segment_cells is None:
            segment_cells = _segment_cells(R, max_path, torch, dev, 0)
        with torch.cuda.device(dev):
            eng._check(getattr(lib, "gsm_sgs_grid" + suffix)(
                h, _ptr(grids), _ptr(d_path), _ptr(d_off), max_path, _ptr(d_draw), _ptr(d_lo), _ptr(d_hi),
                1 if plan.bounds is not None else 0, *axes, *operands, int(segment_cells), _ptr(d_tr), eng._stream()))
        ns = grids.cpu().numpy()
        if trace:
            paths = [p for p, _ in plans] if mode == "replay" else list(d_path.cpu().numpy()[:total].reshape(R, max_path))
        extra = (paths, d_tr.cpu().numpy()) if trace else None
    finally:
        eng.close()
    return ns, extra


def _inverse(plan, ns):
    return plan.nst.inverse_transform(ns.reshape(-1, 1)).squeeze().reshape(ns.shape)


def sgs(xx, yy, grid, variogram, radius=100e3, num_points=20, ktype='ok', sim_mask=None, quiet=False, stencil=None, rcond=None,
        bounds=None, seed=None, device=None, mode='replay'):
    """Sequential Gaussian simulation with ordinary ('ok') or simple ('sk') kriging on the device -- interpolate.sgs
    (gstatsim_custom/interpolate.py:92-191): same arguments and return value (the simulated grid in data units), the generator
    consumed exactly as the reference consumes it.  `device`: CUDA/HIP device index (default: torch's current device).
    `mode`: where the generator is consumed, 'replay' (host) or 'pcg64' (device), as in sgs_many; the result is the same.
    Variogram parameters: numbers or maps of the grid's shape, in any mix (module docstring); a map of another shape raises
    ValueError.
    Not supported (NotImplementedError): a custom stencil, rcond other than None, vtype 'matern' with a parameter map,
    num_points outside [8, 48], a grid that is not axis-aligned with uniform spacing.  A grid without any conditioning value raises
    ValueError (the reference never terminates there); so does a truncated draw scipy would not make (kriging variance 0,
    or bounds that leave no interval), raised from the device as GsmError."""
    return sgs_many(xx, yy, grid, variogram, [seed], radius=radius, num_points=num_points, ktype=ktype, sim_mask=sim_mask,
                    quiet=quiet, stencil=stencil, rcond=rcond, bounds=bounds, device=device, mode=mode)[0]


def sgs_many(xx, yy, grid, variogram, seeds, *, radius=100e3, num_points=20, ktype='ok', sim_mask=None, quiet=False, stencil=None,
             rcond=None, bounds=None, segment_cells=None, device=None, mode='replay'):
    """len(seeds) realisations of interpolate.sgs in one device call: out[r] is bit for bit sgs(..., seed=seeds[r]) -- an int,
    a numpy Generator (advanced exactly as the reference advances it, in the order of `seeds`) or None.  Returns [R, H, W];
    list(out) is what largeScaleChain_mp takes as initial_beds.
    One normal-score transformer is fitted for all rows.  That equals separate calls while the conditioning data hold at most
    10 000 values: above that scikit-learn's QuantileTransformer fits on a random subsample (subsample=10_000, random_state=None),
    so the reference's own fit differs from call to call there.
    segment_cells: path slots whose records are resident at once (default: from the free device memory); it does not change
    the result.
    mode: 'replay' (default) makes every row's shuffle and draws with NumPy on the host, one generator after the other; 'pcg64'
    makes them on the device for all rows side by side (gsm_sgs_grid_draw_pcg64: the generators' own PCG64 streams, bit for
    bit) -- the same result and the same final generator states, without the host's shuffle, which dominates a call of many
    rows.  'pcg64' takes numpy.random.Generator(PCG64) generators (ints and None become such) and raises ValueError for another
    bit generator or for the same Generator listed twice (one sequential stream in 'replay', rows side by side on the device)."""
    plan = _Plan(xx, yy, grid, variogram, radius, num_points, ktype, sim_mask, stencil, rcond, bounds)
    if segment_cells is not None and int(segment_cells) < 1:
        raise ValueError("segment_cells must be >= 1")
    gens = [_generator(s) for s in seeds]
    _check_mode(mode, gens)
    if not gens:
        return np.zeros((0,) + plan.grid_ns.shape)
    ns, _ = _run(plan, gens, segment_cells, device, mode=mode)
    return _inverse(plan, ns)


# ---- interpolate.krige ----------------------------------------------------------------------------------------------------------
def _krige_plan(xx, yy, grid, variogram, radius, num_points, ktype, sim_mask, stencil):
    return _Plan(xx, yy, grid, variogram, radius, num_points, ktype, sim_mask, stencil, None, None)


def _krige_cells(plan):
    """The cells interpolate.krige solves a system for (interpolate.py:46-55): those of sim_mask that hold no value, in C order."""
    flat = plan.inds[:, 0] * plan.W + plan.inds[:, 1]
    return np.ascontiguousarray(flat[~plan.cond.ravel()[flat]], dtype=np.int32)


def _krige_run(plan, cells=None, device=None):
    """One gsm_krige_grid call on `cells` (default: _krige_cells).  Returns per listed cell the estimate, the SIGNED variance
    (sill - sum w rho) and the neighbour count."""
    import torch
    from .engine import GsmEngine, _ptr
    if cells is None:
        cells = _krige_cells(plan)
    cells = np.ascontiguousarray(cells, dtype=np.int32)
    if cells.size == 0:
        return np.zeros(0), np.zeros(0), np.zeros(0, dtype=np.int32)
    H, W = plan.H, plan.W
    eng = GsmEngine(H, W, 1, device)
    try:
        dev, lib, h = eng.dev, eng.lib, eng.h
        axes, suffix, operands, keep = _kriging_operands(plan, eng, torch, 1)
        d_grid = torch.as_tensor(np.ascontiguousarray(plan.grid_ns, dtype=np.float64)).to(dev)
        d_cells = torch.as_tensor(cells).to(dev)
        d_est = torch.empty(cells.size, dtype=torch.float64, device=dev)
        d_var = torch.empty(cells.size, dtype=torch.float64, device=dev)
        d_n = torch.empty(cells.size, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            eng._check(getattr(lib, "gsm_krige_grid" + suffix)(h, _ptr(d_grid), _ptr(d_cells), int(cells.size), *axes, *operands,
                                                               _ptr(d_est), _ptr(d_var), _ptr(d_n), eng._stream()))
        out = d_est.cpu().numpy(), d_var.cpu().numpy(), d_n.cpu().numpy()
    finally:
        eng.close()
    return out


def _score_maps(plan, cells, est, var, n):
    """The per-cell results as interpolate.krige's grids in normal-score space (interpolate.py:40-41, :80-83): the estimate
    over the transformed data (NaN stays where a cell is neither data nor solved), the variance 0 except at the solved cells
    and clipped at 0 there, and the neighbour counts (0 where no system was solved)."""
    est_ns = plan.grid_ns.copy()
    var_ns = np.zeros(plan.grid_ns.shape)
    n_map = np.zeros(plan.grid_ns.shape, dtype=np.int32)
    est_ns.ravel()[cells] = est
    var_ns.ravel()[cells] = np.where(var < 0, 0, var)
    n_map.ravel()[cells] = n
    return est_ns, var_ns, n_map


def _data_maps(plan, est_ns, var_ns):
    """interpolate.py:85-87: both grids through the transformer's inverse_transform, the standard deviation too."""
    return _inverse(plan, est_ns), _inverse(plan, np.sqrt(var_ns))


def _scores(plan, device=None):
    cells = _krige_cells(plan)
    return _score_maps(plan, cells, *_krige_run(plan, cells, device))


def krige_scores(xx, yy, grid, variogram, radius=100e3, num_points=20, ktype='ok', sim_mask=None, quiet=False, stencil=None,
                 device=None):
    """interpolate.krige in normal-score space: (est_ns, var_ns, n_neighbours), three [H, W] maps.  est_ns: the transformed
    data with the kriging estimate at every cell of sim_mask that holds no value (NaN elsewhere).  var_ns: the kriging variance
    there, clipped at 0 as interpolate.py:83 does, 0 at every other cell; sqrt(var_ns) is the kriging standard deviation in
    scores.  n_neighbours (int32): the size of each cell's system, 0 where none was solved.  Arguments, errors and limits as
    krige."""
    return _scores(_krige_plan(xx, yy, grid, variogram, radius, num_points, ktype, sim_mask, stencil), device)


def krige(xx, yy, grid, variogram, radius=100e3, num_points=20, ktype='ok', sim_mask=None, quiet=False, stencil=None, device=None):
    """Ordinary ('ok') or simple ('sk') kriging on the device -- interpolate.krige (gstatsim_custom/interpolate.py:13-89): same
    arguments and return value, (sim_trans, std_trans), two [H, W] maps in data units.  `device`: CUDA/HIP device index
    (default: torch's current device).  The reference's own krige raises TypeError at its current HEAD (it unpacks seven values
    from a _preprocess that returns eight); this is that function with the call repaired.
    sim_trans is the kriging mean: the data's round trip through the transformer at the conditioning cells, the back-transformed
    estimate at the cells of sim_mask, NaN elsewhere.
    std_trans reproduces the reference to the letter, quirk included: it is inverse_transform(sd), the data QUANTILE whose
    normal score equals the kriging standard deviation -- the data median where sd = 0 (every conditioning cell), higher values
    where the data constrain less.  It is not a standard deviation in data units.  krige_scores returns the quantity that means
    something (the variance in normal-score space) and the neighbour counts.
    Variogram parameters: numbers or maps of the grid's shape, in any mix (module docstring); a map of another shape raises
    ValueError.
    Not supported (NotImplementedError): a custom stencil, vtype 'matern' with a parameter map, num_points outside [8, 48], a
    grid that is not axis-aligned with uniform spacing.  A grid without any conditioning value raises ValueError (the reference never
    terminates there)."""
    plan = _krige_plan(xx, yy, grid, variogram, radius, num_points, ktype, sim_mask, stencil)
    est_ns, var_ns, _ = _scores(plan, device)
    return _data_maps(plan, est_ns, var_ns)


# ---- cross-validation -------------------------------------------------------------------------------------------------------------
CV_MAX_MODELS = 8            # models per gsm_krige_cv call (kKrigeCvMaxModels); more are sent in groups


def block_folds(shape, block=(8, 8), k=5, seed=None, mask=None):
    """Spatial folds: the grid is cut into blocks of block = (bh, bw) cells (the last row and column of blocks may be smaller),
    the blocks are shuffled with numpy.random.default_rng(seed) and dealt to the k folds in turn, so the folds hold the same
    number of blocks to within one.  The hold-out that means something for data on lines: a whole neighbourhood leaves
    together.  Returns int32 [H, W] labels in 0 .. k - 1; -1 (in no fold) outside `mask` if one is given."""
    H, W = (int(v) for v in shape)
    bh, bw = (int(v) for v in block)
    k = int(k)
    if H < 1 or W < 1 or bh < 1 or bw < 1:
        raise ValueError("shape and block must be positive")
    nbi, nbj = -(-H // bh), -(-W // bw)
    if not 2 <= k <= nbi * nbj:
        raise ValueError(f"k must be in [2, number of blocks = {nbi * nbj}]")
    of_block = np.empty(nbi * nbj, dtype=np.int32)
    of_block[np.random.default_rng(seed).permutation(nbi * nbj)] = np.arange(nbi * nbj, dtype=np.int32) % k
    out = np.ascontiguousarray(of_block.reshape(nbi, nbj)[np.arange(H)[:, None] // bh, np.arange(W)[None, :] // bw], dtype=np.int32)
    if mask is not None:
        mask = np.asarray(mask, dtype=bool)
        if mask.shape != (H, W):
            raise ValueError("mask must have the grid's shape")
        out[~mask] = -1
    return out


def random_folds(mask, k=5, seed=None):
    """Random folds of the cells of `mask` (bool [H, W]: the data cells, ~numpy.isnan(grid)): shuffled with
    numpy.random.default_rng(seed) and dealt to the k folds in turn (equal sizes to within one).  Returns int32 [H, W]
    labels in 0 .. k - 1, -1 (in no fold) outside the mask."""
    mask = np.asarray(mask)
    if mask.ndim != 2 or mask.dtype != np.bool_:
        raise ValueError("mask must be a 2D bool array")
    k = int(k)
    cells = np.flatnonzero(mask)
    if not 2 <= k <= max(cells.size, 1) or cells.size < 2:
        raise ValueError(f"k must be in [2, number of cells of the mask = {cells.size}]")
    out = np.full(mask.size, -1, dtype=np.int32)
    out[cells[np.random.default_rng(seed).permutation(cells.size)]] = np.arange(cells.size, dtype=np.int32) % k
    return out.reshape(mask.shape)


class CrossValidation:
    """What cross_validate returns: per validated data cell the held-back value and, per model, the estimate made without it.
        cells [n]            flat indices (row * W + column) of the validated cells, ascending unless given otherwise
        names [M]            the models' names
        z_ns [n]             the held-back values, normal scores
        est_ns [M, n]        the kriging estimates, normal scores; NaN where a model's system was singular
        var_ns [M, n]        the kriging variances clipped at 0 (as krige_scores clips them); var_signed: as computed
        n_neighbours [n]     size of the solved systems (one neighbour set for all models)
        z, est               the same values and estimates in data units (the transformer's inverse_transform)"""

    def __init__(self, plan, cells, names, est_ns, var_signed, n_neighbours):
        self.shape = (plan.H, plan.W)
        self._nst = plan.nst
        self.cells = np.asarray(cells)
        self.names = list(names)
        self.z_ns = plan.grid_ns.ravel()[self.cells] if self.cells.size else np.zeros(0)
        self.est_ns = np.asarray(est_ns, dtype=np.float64).reshape(len(self.names), self.cells.size)
        self.var_signed = np.asarray(var_signed, dtype=np.float64).reshape(self.est_ns.shape)
        self.var_ns = np.where(self.var_signed < 0, 0, self.var_signed)                  # NaN stays NaN
        self.n_neighbours = np.asarray(n_neighbours, dtype=np.int32)

    def _to_data(self, ns):
        if ns.size == 0:
            return ns.copy()
        return self._nst.inverse_transform(ns.reshape(-1, 1)).reshape(ns.shape)

    @property
    def z(self):
        return self._to_data(self.z_ns)

    @property
    def est(self):
        return self._to_data(self.est_ns)

    def _index(self, m):
        return self.names.index(m) if isinstance(m, str) else int(m)

    def error(self, data_units=False):
        """estimate - held-back value, [M, n]: in normal scores, or in data units."""
        return self.est - self.z[None, :] if data_units else self.est_ns - self.z_ns[None, :]

    def standardized(self):
        """error / kriging standard deviation in normal scores, [M, n]; NaN where the (clipped) variance is 0."""
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(self.var_ns > 0, self.error() / np.sqrt(self.var_ns), np.nan)

    def maps(self, m=0):
        """Model m (index or name) scattered to the grid: dict of [H, W] maps est_ns, var_ns, error, standardized (NaN at every
        cell that was not validated) and n_neighbours (int32, 0 there)."""
        m = self._index(m)
        out = {}
        for key, v in (("est_ns", self.est_ns[m]), ("var_ns", self.var_ns[m]), ("error", self.error()[m]),
                       ("standardized", self.standardized()[m])):
            a = np.full(self.shape, np.nan)
            a.ravel()[self.cells] = v
            out[key] = a
        n = np.zeros(self.shape, dtype=np.int32)
        n.ravel()[self.cells] = self.n_neighbours
        out["n_neighbours"] = n
        return out

    def summary(self):
        """Per model name a dict: n (cells with an estimate), mean_error, mae, rmse (normal scores), rmse_data (data units),
        mean_standardized, msdr (mean squared standardized error: about 1 where the kriging variance is calibrated), r (Pearson
        correlation of estimate and held-back score) and coverage95 (share of |standardized error| <= 1.96).  Cells without an
        estimate (NaN) are left out, and cells with variance 0 out of the three standardized figures; a figure over no cell is
        NaN."""
        e, ed, s = self.error(), self.error(data_units=True), self.standardized()
        out = {}
        for m, name in enumerate(self.names):
            ok = np.isfinite(e[m])
            sm = s[m][np.isfinite(s[m])]
            nan = float("nan")
            row = {"n": int(ok.sum())}
            row["mean_error"] = float(np.mean(e[m][ok])) if ok.any() else nan
            row["mae"] = float(np.mean(np.abs(e[m][ok]))) if ok.any() else nan
            row["rmse"] = float(np.sqrt(np.mean(e[m][ok] ** 2))) if ok.any() else nan
            row["rmse_data"] = float(np.sqrt(np.mean(ed[m][ok] ** 2))) if ok.any() else nan
            row["mean_standardized"] = float(np.mean(sm)) if sm.size else nan
            row["msdr"] = float(np.mean(sm ** 2)) if sm.size else nan
            row["coverage95"] = float(np.mean(np.abs(sm) <= 1.96)) if sm.size else nan
            a, b = self.est_ns[m][ok], self.z_ns[ok]
            row["r"] = float(np.corrcoef(a, b)[0, 1]) if ok.sum() >= 2 and np.std(a) > 0 and np.std(b) > 0 else nan
            out[name] = row
        return out

    def best(self, by="rmse"):
        """Name of the model with the smallest mae / rmse / rmse_data, the largest r, or the msdr closest to 1."""
        s = self.summary()
        if by in ("rmse", "mae", "rmse_data"):
            key = lambda n: s[n][by]
        elif by == "r":
            key = lambda n: -s[n]["r"]
        elif by == "msdr":
            key = lambda n: abs(s[n]["msdr"] - 1.0)
        else:
            raise ValueError("by must be 'rmse', 'mae', 'rmse_data', 'r' or 'msdr'")
        ranked = [n for n in self.names if not math.isnan(key(n))]
        if not ranked:
            raise ValueError("no model has an estimate to rank")
        return min(ranked, key=key)


def _cv_models(variogram):
    """(names, variogram dicts) of cross_validate's `variogram`: one variogram, a dict name -> variogram (variograms(...)[0])
    or a list of variograms (named '0', '1', ...)."""
    if isinstance(variogram, dict) and "vtype" in variogram:
        return [str(variogram["vtype"]).lower()], [variogram]
    if isinstance(variogram, dict):
        names, models = [str(k) for k in variogram.keys()], list(variogram.values())
    elif isinstance(variogram, (list, tuple)):
        names, models = [str(i) for i in range(len(variogram))], list(variogram)
    else:
        raise ValueError("variogram must be a variogram dict, a dict of them or a list of them")
    if not models or not all(isinstance(v, dict) for v in models):
        raise ValueError("variogram must hold at least one variogram dict")
    return names, models


def _cv_cells(plan, cells):
    """The flat indices cross_validate validates: every data cell, those of a bool mask, or the listed ones as they are."""
    cond = plan.cond.ravel()
    if cells is None:
        flat = np.flatnonzero(cond)
    else:
        cells = np.asarray(cells)
        if cells.dtype == np.bool_:
            if cells.shape != (plan.H, plan.W):
                raise ValueError("a cells mask must have the grid's shape")
            flat = np.flatnonzero(cells)
        elif np.issubdtype(cells.dtype, np.integer) and cells.ndim == 1:
            flat = cells.astype(np.int64)
            if flat.size and (flat.min() < 0 or flat.max() >= cond.size):
                raise ValueError("cells holds an index outside the grid")
        else:
            raise ValueError("cells must be None, a bool mask of the grid's shape or a 1D array of flat indices")
        if not cond[flat].all():
            raise ValueError("cells lists a cell without a value: only data cells can be validated")
    return np.ascontiguousarray(flat, dtype=np.int32)


def _cv_run(plan, models, cells, fold, exclude_radius, device=None):
    """gsm_krige_cv / gsm_krige_cv_local on `cells` for the variograms `models` (all scalar or all with maps), CV_MAX_MODELS per
    call.  Returns est [M, n], the signed variance [M, n] and the neighbour counts [n]."""
    import torch
    from .engine import GsmEngine, _ptr
    H, W, M, n = plan.H, plan.W, len(models), int(cells.size)
    est, var, cnt = np.full((M, n), np.nan), np.full((M, n), np.nan), np.zeros(n, dtype=np.int32)
    if n == 0:
        return est, var, cnt
    local = plan.local is not None
    hw = int(math.ceil(plan.radius / abs(plan.dx)))
    eng = GsmEngine(H, W, 1, device)
    try:
        dev, lib, h = eng.dev, eng.lib, eng.h
        f64 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
        per_model = H * W * 6 * 8 if local else (2 * H - 1) * (2 * W - 1) * 8
        group = min(M, CV_MAX_MODELS)
        if per_model * group > torch.cuda.mem_get_info(dev)[0] // 4:
            raise MemoryError(f"the {'per-cell variogram' if local else 'whole-grid lag covariance'} tables of {group} models "
                              f"({per_model * group} bytes) do not fit the device; pass fewer models per call")
        d_xs, d_ys, d_gm = f64(plan.xs), f64(plan.ys), f64(np.full(1, plan.global_mean))
        d_grid = f64(plan.grid_ns)
        d_cells = torch.as_tensor(cells).to(dev)
        d_fold = None if fold is None else torch.as_tensor(fold).to(dev)
        d_n = torch.empty(n, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            eng._check(lib.gsm_sgs_set_kriging(h, 1 if plan.ktype == "sk" else 0, _ptr(d_gm)))
        for m0 in range(0, M, CV_MAX_MODELS):
            part = models[m0:m0 + CV_MAX_MODELS]
            d_est = torch.empty((len(part), n), dtype=torch.float64, device=dev)
            d_var = torch.empty((len(part), n), dtype=torch.float64, device=dev)
            head = (h, _ptr(d_grid), _ptr(d_cells), n, _ptr(d_fold), float(exclude_radius), _ptr(d_xs), _ptr(d_ys), len(part))
            tail = (_ptr(d_est), _ptr(d_var), _ptr(d_n), eng._stream())
            with torch.cuda.device(dev):
                if local:
                    d_tab = f64(np.stack([_local_table(v, (H, W)) for v in part]))
                    vt = (C.c_int32 * len(part))(*[LOCAL_VTYPES[v["vtype"].lower()] for v in part])
                    rc = lib.gsm_krige_cv_local(*head, _ptr(d_tab), vt, hw, plan.radius, plan.num_points, *tail)
                else:
                    scal = [{k: (v if k == "vtype" else float(v)) for k, v in vv.items()} for vv in part]
                    d_tab = f64(np.stack([lag_cov_table(v, hw, plan.dx, plan.dy, H - 1, W - 1) for v in scal]))
                    sill = (C.c_double * len(part))(*[v["sill"] for v in scal])
                    rc = lib.gsm_krige_cv(*head, _ptr(d_tab), H - 1, W - 1, hw, plan.radius, plan.num_points, sill, *tail)
            # a singular system leaves NaN at its (model, cell) and the rest of the call complete: keep what was computed
            est[m0:m0 + len(part)], var[m0:m0 + len(part)] = d_est.cpu().numpy(), d_var.cpu().numpy()
            eng._check(rc)
        cnt = d_n.cpu().numpy()
    finally:
        eng.close()
    return est, var, cnt


def cross_validate(xx, yy, grid, variogram, radius=100e3, num_points=20, ktype='ok', folds=None, exclude_radius=0.0, cells=None,
                   device=None):
    """Kriging cross-validation on the device (gsm_krige_cv, csrc/krige_cv_kernel.hip): every measured cell is kriged from the
    other measurements and compared with the value that was held back -- gstat's krige.cv, GSLIB's jackknife -- with krige's
    search, radius widening and solve.  The step between variograms(...) and krige / sgs: which model, which radius and
    num_points, and whether parameter maps beat one stationary model.

    variogram: one variogram dict, a dict name -> variogram (variograms(...)[0] goes in directly) or a list of them.  All models
    share one neighbour search per cell; more than eight are sent in groups of eight.  Either every model has scalar parameters
    or every model has at least one parameter map (ValueError otherwise).
    The hold-out of a target cell t, beside t itself:
        folds            int [H, W] labels (block_folds, random_folds): every cell of t's fold; a negative label is "in no fold"
        exclude_radius   > 0: every cell within this distance (in the units of xx, yy) of t -- the buffered hold-out for data
                         on lines, where the next cell of t's own line all but predicts it.  Choose it off the grid's distances
                         (2.5 cell widths on square cells)
    With neither, plain leave-one-out.  A target that is left no value at all raises GsmError.
    cells: the data cells to validate, a bool mask or flat indices (row * W + column); default: every data cell.

    The normal-score transformer is fitted ONCE on all data, the target's included (_Plan's), and neither it nor the global
    mean of simple kriging is refitted per hold-out.  That is the convention here because the transform is marginal -- it
    carries no spatial information from the target to its estimate -- and because it is the transform the krige / sgs call
    that follows will use: the errors are those of that call's scores.
    Cost: the held-out neighbours are not known on the host, so each model gets a covariance table over every lag of the grid,
    (2H - 1)(2W - 1) * 8 bytes; MemoryError beyond a quarter of the free device memory.
    Arguments, ValueErrors and NotImplementedErrors otherwise as krige (no stencil; Matern with parameter maps is refused).
    Returns a CrossValidation."""
    names, models = _cv_models(variogram)
    plan = _Plan(xx, yy, grid, models[0], radius, num_points, ktype, None, None, None, None)
    for v in models[1:]:
        _sanity_checks(xx, yy, grid, v, radius, num_points, ktype, None)
    mapped = [any(isinstance(x, np.ndarray) for k, x in v.items() if k != "vtype") for v in models]
    if any(mapped) and not all(mapped):
        raise ValueError("the models must all have scalar parameters or all have a parameter map (two calls otherwise)")
    if all(mapped):
        for v in models[1:]:
            _local_table(v, grid.shape)                                               # its errors before any device work
    if not isinstance(exclude_radius, numbers.Number) or not exclude_radius >= 0:
        raise ValueError("exclude_radius must be a number >= 0")
    fold = None
    if folds is not None:
        folds = np.asarray(folds)
        if folds.shape != grid.shape or not np.issubdtype(folds.dtype, np.integer):
            raise ValueError("folds must be an integer array of the grid's shape")
        fold = np.ascontiguousarray(np.clip(folds, -1, np.iinfo(np.int32).max), dtype=np.int32).ravel()
    flat = _cv_cells(plan, cells)
    est, var, n = _cv_run(plan, models, flat, fold, float(exclude_radius), device)
    return CrossValidation(plan, flat, names, est, var, n)
