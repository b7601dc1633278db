"""Cases and the plain reference of the small-scale chain's iteration end (mcmc_gpu_amd/csrc/sgs_iter_kernel.hip): the full-grid
loss and thickness guard, the windowed state, the Metropolis decision and the commits.  NumPy only; the GPU tests
(tests/test_gpu_sgs_iter.py) and the host check that the bar is fair (tests/test_sgs_iter_host.py) share it.

The reference restates the reference project's lines in numpy.longdouble:
  residual   Topography.get_mass_conservation_residual on np.gradient: interior (f[i+1] - f[i-1]) / (2 h), one-sided (f[1] - f[0]) / h
             and (f[-1] - f[-2]) / h at the borders; x runs along the columns, y along the rows
  loss       nansum(residual^2 where mc_mask == 1) / (2 sigma^2)                                    (MCMC.py:1021-1044)
  guard      count of update_mask == 1 cells with surf - (bed [+ trend]) <= 0; a NaN thickness is not bad     (MCMC.py:1789-1795)
  decision   1 if lp > ln else min(1, np.exp(lp - ln)) with Python's built-in min, then u <= rate              (MCMC.py:1797-1801)
The reference adds the trend in fp64 before anything else (bed_next + trend), so `bed` below is always that fp64 sum.

Bounds (u = 2^-53, first order with the slack named; FMA contraction only removes roundings).  cell_residual makes, on the way
of q_xr to the result: thickness surf - bed (1), velx * thickness (2), q_xr - q_xl (3), / den_x (4; den is res or 2 res, exact),
dx + dy (5), + dhdt (6), - smb (7): seven roundings, each relative to a partial result that is at most
  A = (|q_xr| + |q_xl|) / den_x + (|q_yd| + |q_yu|) / den_y + |dhdt| + |smb|
in magnitude; the y terms likewise, dhdt two, smb one.  So |v_dev - v_ld| <= 7 u A to first order, and
  RES_BOUND(cell) = 8 u A
holds with the second-order terms ((1 + u)^7 - 1 < 7 u (1 + 4 u)) and the long-double reference's own error (2^-64 per operation)
inside the eighth unit.  cell_energy squares: e_dev = v_dev^2 (1 + eps), so with dv = RES_BOUND
  ENERGY_BOUND(cell) = 2 |v| dv + dv^2 + u v^2
(the omitted u (2 |v| dv + dv^2) is below the slack 2 |v| u A + 15 u^2 A^2 that the eighth unit leaves).  A sum of n terms in any
order makes n - 1 additions with nonzero operands, each off by at most u times the sum of the (positive) terms; the division by
2 sigma^2 is one more, one is spare:
  LOSS_BOUND = (sum over the cells that enter of ENERGY_BOUND + (n + 1) u sum e) / (2 sigma^2),  n = cells that enter the sum.
A compensated sum (state[0] + state[1]) promises 2 u sum e against the exact sum of the SAME terms (COMP_BOUND)."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
SIGMA = 5.0
TWO_SIGMA2 = 2.0 * (SIGMA * SIGMA)                     # gsm_set_static: 2 * (sigma_mc * sigma_mc); the reference: 2 * sigma_mc ** 2
RES = 500.0
KSGS_HALO_MAX = 36 * 36                                # sgs_iter_kernel.hip: kSgsHaloMax
KSGS_MAX_WIN = 1024                                    # gsm_internal.h: kSgsMaxWin, cells of a block the simulation takes
KTAIL_TILE, KTAIL_QT = 2048, 1024                      # sgs_iter_kernel.hip: kTailTile, kTailQt
QT_INV_ATOL = 1e-9                                     # metres: gsm_qt_transform's inverse against scikit-learn (tests/test_gpu_sgs.py)

# 32 x 33 splits into two parts of 528 cells = 16 whole rows; 33 x 32 puts the same boundary at cell 528 in the middle of row 16
# 2 x 2 (every cell on two borders) is checked on the host only: gsm_create takes no side below 3, so 3 x 3 stands in on the device
GRIDS = [(2, 2), (3, 3), (5, 7), (33, 31), (32, 33), (33, 32), (41, 50), (8, 512), (20, 600), (256, 257)]
SMALL_GRIDS = [g for g in GRIDS if g[0] * g[1] <= 1056]          # where 70 chains run
GPU_GRIDS = [g for g in GRIDS if min(g) >= 3]
CHAINS = [1, 3, 70]


def loss_parts(H, W):
    """sgs_loss_parts: parts of a chain's map, and the cells of a part."""
    parts = max(1, min(64, (H * W + 1023) // 1024))
    return parts, (H * W + parts - 1) // parts


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def _grad_ld(q, axis, res, absolute=False):
    """np.gradient(q, res, axis) in long double; absolute: (|q[i+1]| + |q[i-1]|) / den instead, the magnitude of the same stencil."""
    q = np.moveaxis(q, axis, 0)
    op = (lambda a, b: np.abs(a) + np.abs(b)) if absolute else (lambda a, b: a - b)
    out = np.empty_like(q)
    out[1:-1] = op(q[2:], q[:-2]) / (LD(2.0) * LD(res))
    out[0] = op(q[1], q[0]) / LD(res)
    out[-1] = op(q[-1], q[-2]) / LD(res)
    return np.moveaxis(out, 0, axis)


def residual_ld(bed, surf, velx, vely, dhdt, smb, res):
    """(v, A): the mass-conservation residual d/dx(velx (surf - bed)) + d/dy(vely (surf - bed)) + dhdt - smb of a [..., H, W] bed in
    long double, and the magnitude A of the module docstring per cell (NaN where v is NaN)."""
    bed, surf, velx, vely, dhdt, smb = (np.asarray(a, dtype=np.float64).astype(LD) for a in (bed, surf, velx, vely, dhdt, smb))
    thick = surf - bed
    qx, qy = velx * thick, vely * thick
    v = _grad_ld(qx, -1, res) + _grad_ld(qy, -2, res) + dhdt - smb
    A = _grad_ld(qx, -1, res, True) + _grad_ld(qy, -2, res, True) + np.abs(dhdt) + np.abs(smb)
    return v, A


def energy_ld(v, mc_mask):
    """The squared residual as it enters the loss: 0 where mc_mask != 1 or the residual is NaN (nansum)."""
    enters = (np.asarray(mc_mask) == 1) & ~np.isnan(v)
    return np.where(enters, v * v, LD(0.0)), enters


def energy_bound(v, A, enters):
    dv = LD(8.0) * LD(U) * A
    return np.where(enters, LD(2.0) * np.abs(v) * dv + dv * dv + LD(U) * v * v, LD(0.0))


def loss_ld(v, A, mc_mask):
    """(loss, LOSS_BOUND, sum of the energies) per plane of a [..., H, W] residual, long double."""
    e, enters = energy_ld(v, mc_mask)
    eb = energy_bound(v, A, enters)
    n = enters.sum(axis=(-2, -1))
    s = e.sum(axis=(-2, -1))
    bound = (eb.sum(axis=(-2, -1)) + (n + 1) * LD(U) * s) / LD(TWO_SIGMA2)
    return s / LD(TWO_SIGMA2), bound, s


def bad_count(bed, surf, update_mask):
    """Cells of update_mask == 1 with surf - bed <= 0, in fp64 as the reference computes it (bed: the fp64 sum with the trend)."""
    with np.errstate(invalid="ignore"):
        return ((np.asarray(surf) - np.asarray(bed) <= 0) & (np.asarray(update_mask) == 1)).sum(axis=(-2, -1))


def with_trend(bed, trend):
    """bed_next + trend in fp64 (MCMC.py:1781), or the bed itself."""
    return bed if trend is None else bed + trend


def score(case, beds, trend):
    """Reference loss, its bound and the bad count of [n, H, W] beds: what gsm_sgs_loss answers.  Floats: (loss, bound, bad, sum e)."""
    b = with_trend(beds, trend)
    v, A = residual_ld(b, case["surf"], case["velx"], case["vely"], case["dhdt"], case["smb"], RES)
    loss, bound, s = loss_ld(v, A, case["mc"])
    return loss, bound, bad_count(b, case["surf"], case["upd"]), s


def decide_ref(lp, ln, u):
    """The reference's literal decision (MCMC.py:1797-1801), scalar by scalar: Python's min(1, nan) is 1."""
    lp, ln, u = float(lp), float(ln), float(u)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        rate = 1 if lp > ln else min(1, np.exp(lp - ln))
    return bool(u <= rate)


def rate_ref(lp, ln):
    lp, ln = float(lp), float(ln)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return 1.0 if lp > ln else float(min(1, np.exp(lp - ln)))


def u_at_margin(lp, ln, bound_diff, below):
    """u placed at p_ref (1 -/+ m), m = max(1e-9, 8 x the derived bound on lp - ln): exp(d + e) = exp(d) (1 + e + ..) moves the device's p by
    at most a factor 1 + 2 |e| for |e| < 1/2, so a u that far on one side of p_ref is decided alike by every path inside the bound.
    A uniform draw lies in [0, 1): where p_ref is 1 there is no `above`, and u is 1 - m."""
    m = max(1e-9, 8.0 * float(bound_diff))
    assert m < 0.25, "the bound on lp - ln leaves the row undecidable"
    p = rate_ref(lp, ln)
    return p * ((1.0 - m) if below or p == 1.0 else (1.0 + m))


# ---- static fields and beds ------------------------------------------------------------------------------------------------------
def make_case(H, W, n_chains, seed=0):
    """Random fields of ice-sheet magnitude on an H x W grid: surface 1500-2500 m, ice 600-1400 m thick, velocities of a few hundred
    m/yr, dhdt and smb below 1 m/yr.  mc_mask has holes, update_mask differs from it, a few bed cells are NaN (their own residual
    and their neighbours' leave the sum), and a thin-ice patch (0.5 m) lets a proposal of about a metre ground cells or not.
    Chain c's bed depends on (grid, c) alone, so chain c is the same bed whatever n_chains is."""
    rng = np.random.default_rng([H, W, seed])
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    surf = 2000.0 + 300.0 * np.sin(0.21 * xx + 0.3) * np.cos(0.17 * yy) + 5.0 * rng.standard_normal((H, W))
    thick = 1000.0 + 300.0 * np.cos(0.13 * xx - 0.29 * yy) + 20.0 * rng.standard_normal((H, W))
    velx = 250.0 * np.sin(0.11 * yy + 0.4) + 30.0 * rng.standard_normal((H, W))
    vely = -180.0 * np.cos(0.09 * xx) + 30.0 * rng.standard_normal((H, W))
    dhdt = 0.4 * rng.standard_normal((H, W))
    smb = 0.3 * rng.standard_normal((H, W))
    mc = (rng.random((H, W)) < 0.8).astype(np.uint8)
    upd = (rng.random((H, W)) < 0.85).astype(np.uint8)
    if H * W >= 4:
        mc.flat[0], upd.flat[0], mc.flat[-1], upd.flat[-1] = 1, 0, 0, 1              # the two masks differ on every grid
    # thin-ice patch: up to 3 x 4 cells around the middle, all guarded
    pr, pc = slice(H // 2, min(H, H // 2 + 3)), slice(W // 2, min(W, W // 2 + 4))
    thick[pr, pc] = 0.5
    upd[pr, pc] = 1
    base = surf - thick
    trend = base - 40.0 * np.sin(0.05 * xx + 0.07 * yy) - 100.0                        # a smooth surface below the bed's level
    beds = np.empty((n_chains, H, W))
    for c in range(n_chains):
        r = np.random.default_rng([H, W, seed, 1000 + c])
        beds[c] = base + 3.0 * r.standard_normal((H, W))
        # odd chains: the patch is pushed through the surface on some cells (exactly onto it on the first), even chains stay afloat
        patch = surf[pr, pc] - 0.5 + (0.25 * r.random(surf[pr, pc].shape) if c % 2 == 0 else 1.5 * r.random(surf[pr, pc].shape) - 0.25)
        if c % 2 == 1:
            patch.flat[0] = surf[pr, pc].flat[0]                                       # thickness exactly 0: bad (<=)
        beds[c][pr, pc] = patch
    n_nan = 0 if H * W < 30 else max(2, H * W // 400)
    nan_cells = rng.choice(H * W, size=n_nan, replace=False)
    for c in range(n_chains):
        beds[c].flat[nan_cells] = np.nan
    if H * W >= 30:
        upd.flat[nan_cells[0]] = 1                                                     # a NaN thickness inside the guard: not bad
    return dict(H=H, W=W, n=n_chains, surf=surf, velx=velx, vely=vely, dhdt=dhdt, smb=smb, mc=mc, upd=upd, beds=beds, trend=trend,
                patch=(pr, pc), nan_cells=nan_cells)


def detrended(case):
    """The beds as a detrended chain holds them: bed - trend in fp64; the chain's loss is of (that + trend)."""
    return case["beds"] - case["trend"]


# ---- windows ---------------------------------------------------------------------------------------------------------------------
def halo(win, H, W):
    r0, r1, c0, c1 = win
    return max(0, r0 - 1), min(H, r1 + 1), max(0, c0 - 1), min(W, c1 + 1)


def halo_cells(win, H, W):
    h = halo(win, H, W)
    return (h[1] - h[0]) * (h[3] - h[2])


def finish_windows():
    """{name: (grid, window, over the limit)} of the gsm_sgs_finish cases; every window lies inside its grid."""
    H, W = 41, 50
    w = {"1x1": ((H, W), (17, 18, 23, 24)), "3x3": ((H, W), (8, 11, 30, 33)),
         "corner_tl": ((H, W), (0, 4, 0, 5)), "corner_tr": ((H, W), (0, 3, W - 6, W)),
         "corner_bl": ((H, W), (H - 5, H, 0, 2)), "corner_br": ((H, W), (H - 2, H, W - 3, W)),
         "edge_t": ((H, W), (0, 3, 10, 17)), "edge_b": ((H, W), (H - 4, H, 20, 26)),
         "edge_l": ((H, W), (12, 19, 0, 4)), "edge_r": ((H, W), (25, 31, W - 5, W)),
         "empty": ((H, W), (14, 14, 9, 15)),
         "whole_20x20": ((20, 20), (0, 20, 0, 20)),
         "34x34": ((H, W), (3, 37, 5, 39)),
         "16x70": ((20, 600), (2, 18, 100, 170)),
         "thin_patch": ((H, W), (H // 2 - 1, H // 2 + 4, W // 2 - 2, W // 2 + 5))}
    out = {k: (g, win, False) for k, (g, win) in w.items()}
    out["35x34_over"] = ((H, W), (2, 37, 5, 39), True)
    return out


def tail_windows(H, W):
    """Three disjoint windows (row bands) of at most 1024 cells for the three iterations of one gsm_sgs_iterate call: between them the
    grids meet corners, edges, 1 x 1, empty, 32 x 32 and 4 x 256 windows."""
    special = {(8, 512): [(0, 4, 100, 356), (4, 6, 0, 3), (6, 8, 509, 512)],            # 4 x 256 = kSgsMaxWin; two corners' rows
               (256, 257): [(10, 42, 200, 232), (100, 101, 0, 9), (250, 256, 250, 257)],  # 32 x 32; left edge; bottom-right corner
               (20, 600): [(0, 5, 0, 7), (7, 7, 20, 30), (9, 20, 580, 600)],              # corner, empty, corner
               (41, 50): [(0, 3, 20, 29), (19, 24, 22, 30), (40, 41, 49, 50)],            # top edge, the thin patch, 1 x 1 corner
               (2, 2): [(0, 1, 0, 1), (1, 2, 0, 2), (2, 2, 0, 2)]}
    if (H, W) in special:
        return special[(H, W)]
    a, b = H // 3, 2 * H // 3
    return [(0, a, 0, min(W, 4)), (a, b, W // 2 - min(W // 2, 3), min(W, W // 2 + 4)), (b, H, max(0, W - 5), W)]


# ---- decision rows ---------------------------------------------------------------------------------------------------------------
def decision_rows():
    """(lp, ln, bad, u) rows of gsm_sgs_decide; the losses are inputs here, so u sits exactly where the row says."""
    inf, nan = float("inf"), float("nan")
    below1 = float(np.nextafter(1.0, 0.0))
    p = float(np.exp(-0.75))
    return [(10.0, 9.0, 0, 1.0), (10.0, 9.0, 0, 0.3),                                        # lp > ln
            (7.5, 7.5, 0, 1.0), (7.5, 7.5, 0, below1),                                       # lp == ln: p = 1
            (3.0, 3.75, 0, p * (1 - 1e-9)), (3.0, 3.75, 0, p * (1 + 1e-9)),                  # uphill, u either side of p
            (1.0, 2000.0, 0, 0.0), (1.0, 2000.0, 0, 5e-324),                                 # exp underflows to 0
            (5.0, 4.0, 2, 0.0), (5.0, 4.0, 1, 1e-300), (5.0, 6.0, 3, 0.5),                   # bad > 0: loss_next = +inf
            (inf, 12.0, 0, 0.9), (inf, inf, 0, 0.9), (inf, 5.0, 4, 0.9),                     # (+inf, finite), (+inf, +inf) twice
            (nan, 3.0, 0, 0.5), (3.0, nan, 0, 0.5), (nan, nan, 0, 1.0)]                      # NaN rows: min(1, nan) = 1
