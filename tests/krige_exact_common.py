"""Cases, truth and bars that pin krige_solve (csrc/sgs_search.h) -- the one kriging solve under gsm_sgs_blocks, gsm_sgs_grid,
gsm_krige_grid, gsm_krige_cv and their _local twins -- to an extended-precision solve (tests/test_krige_exact_host.py: the bars
are fair, the cases reach their regimes; tests/test_gpu_krige_exact.py: the device).

Truth.  The fp64 system the device solves -- [Sigma 1; 1' 0] w = [rho; 1] in ordinary kriging, Sigma w = rho in simple kriging --
solved in numpy.longdouble (64-bit significand; the module skips on a narrower one) by Gaussian elimination with partial
pivoting and three steps of iterative refinement with long-double residuals.  Table forms: the entries are those of the lag
table the device is handed (sgs.lag_cov_table; an entry depends on its lag alone, not on the table's extents), so the truth is
the exact solution of the device's own inputs.  Local form: the entries are evaluated in long double from the six numbers of the
cell's row of interpolate._local_table and the coordinates.  est* = sum w* v + (1 - sum w*) mean (the neighbours' mean in ordinary,
the global mean in simple kriging), var* = sill - sum w* rho.

Neighbours never come from the device: oracle/sgs_oracle.neighbors with STABLE_TIES on tie-free grids (sgs_common.TIE_FREE_DY)
and the radius widening of krige_common.krige_scores_cpu (search); held-out grids from krige_cv_common.held_out; the SGS tests
pass the oracle's NBR_LOG.

Bars, per cell, with u = 2^-53, kappa = numpy.linalg.cond of the fp64 system (n + 1 rows in ordinary, n in simple kriging):
    B_est = ((n + 3) u + E) kappa (||w*||_1 max|v| + [simple kriging] (1 + ||w*||_1) |global mean|)
    B_var = ((n + 3) u + E) kappa sill (1 + ||w*||_1)
First-order perturbation theory: a backward-stable solve of A w = b returns the exact solution of (A + dA) w = b + db with
||dA|| <= c n u ||A||, hence ||dw|| <= c n u kappa ||w||, and est, var are inner products of w with v and rho (|rho| <= sill;
the 1 + takes the roundings of the final reductions).  Simple kriging adds (1 - sum w) m with the global mean m to the estimate,
a term of size (1 + ||w||_1) |m| whose own roundings do not shrink with the weights: where rho is all but zero (a cell far from
its only neighbour) or the one neighbour's score is 0 the estimate is m to within u |m| and ||w*||_1 max|v| is (next to) nothing,
so a bar without that term is missed by any fp64 evaluation, numpy.linalg.lstsq's and the restatement's alike.  In ordinary
kriging sum w = 1, the mean is the neighbours' and ||w*||_1 >= 1: the first term covers it.  An unpivoted elimination on a positive-definite block has growth factor 1, so
c is a small constant: tests/test_krige_exact_host.py measures the fp64 restatement of the device's order (host_solve) at no
more than 0.36 of these bars over all cases here (n = 1 .. 48, kappa up to 1.8e12), and numpy.linalg.lstsq up to 3 x above
them at small n: lstsq cannot be the reference at this level.
E = 0 for the table forms.  Local form: E = 2 eps_c, the entries of A and of b each perturbed by eps_c relative:
    eps_c = [bound of special_common.local_cov_reference for local_cov_of on a given h2] + 6 h_max u
with h_max the largest normalised lag of the system.  The first term is 4 eps (1 + |t|), t = -3 h (exponential) or -3 h^2
(Gaussian) at h_max.  The spherical model's c0 - 1.5 h + 0.5 h^3 cancels towards the range, so its bound is absolute,
4 eps (c0 + 1.5 h + 0.5 h^3) + 6 h u (h <= 1: beyond the range the value is the constant sill - 1; |dC / dh| <= 1.5), and E is
that error relative to ||A||_max = c0 plus the same relative to ||b||_inf (max|rho|, or 1 with the Lagrange row) -- relative to c0
alone it promises digits of a small rho that no fp64 evaluation of the polynomial has.  The second: u = dx R00 + dy R10, v likewise and h2 = u u + v v are six roundings of u each, i.e. 3 u
relative in h = sqrt(h2), and dC / C = 3 dh = 3 h (dh / h) for the exponential model; the special-function bound's own slack
(8 u per operation where each rounds by u) takes what the Gaussian model's steeper exponent adds.

A refusal ("singular kriging system") is allowed only where kappa > 1e12; for kappa in (1e12, 1e16) the tests assert "refused,
or finite" and print the device's and lstsq's error against the truth."""
import functools
import warnings
from collections import namedtuple

import numpy as np
import pytest

import krige_common as kc
import krige_cv_common as kcv
import nonstationary_common as nc
import sgs_common as sc
import sgs_oracle as so

LD = np.longdouble
if np.finfo(LD).nmant < 63:
    pytest.skip("numpy.longdouble has no 64-bit significand here: no extended-precision truth", allow_module_level=True)

U = 2.0 ** -53
EPS = 2.0 ** -52
KAPPA_REFUSE = 1e12          # a refusal below this condition number is a failure (the existing sweep's figure)
KAPPA_FINITE = 1e16


def _iso(vtype, r, sill=1.0, nugget=0.0, **kw):
    return dict(major_range=float(r), minor_range=float(r), azimuth=0.0, sill=sill, nugget=nugget, vtype=vtype, **kw)


GAUSSIAN_RANGES = (700.0, 1500.0, 2200.0, 3000.0, 3600.0)
MODELS = {
    "exp9k": _iso("Exponential", 9000.0),
    "matern": _iso("Matern", sc.DRIVER_V1_P[0], sill=sc.DRIVER_V1_P[1], nugget=float(sc.DRIVER_V1_P[3]), s=sc.DRIVER_V1_P[2]),
    "sph9k": _iso("Spherical", 9000.0),
    "exp_aniso": dict(major_range=8000.0, minor_range=5000.0, azimuth=30.0, sill=1.0, nugget=0.05, vtype="Exponential"),
    **{f"gau{int(r)}": _iso("Gaussian", r) for r in GAUSSIAN_RANGES},
}
KTYPES = ("ok", "sk")
LAYOUTS = ("a", "b", "c", "d")
LOCAL_VTYPES = ("Exponential", "Gaussian", "Spherical")
MAX_CELLS = 60


# ---- data layouts -----------------------------------------------------------------------------------------------------------------
def _spread(cells, count):
    """`count` of `cells` (ascending flat indices), evenly spread, the first and the last included."""
    cells = np.asarray(cells)
    if cells.size <= count:
        return cells
    return cells[np.unique(np.round(np.linspace(0, cells.size - 1, count)).astype(int))]


def search(xx, yy, grid, i, j, radius, num_points):
    """The reference's octant search of cell (i, j) on `grid` (NaN: no value) with its radius widening, as
    krige_common.krige_scores_cpu makes it, equidistant candidates in the device's order.  Returns (rows, columns, widenings)."""
    H, W = grid.shape
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    cond = ~np.isnan(grid)
    saved, so.STABLE_TIES = so.STABLE_TIES, True
    try:
        rad, k = radius, 0
        while True:
            stencil, _, _ = so.make_circle_stencil(xx[0, :], rad)
            near = so.neighbors(i, j, ii, jj, xx, yy, grid, cond, rad, num_points, stencil=stencil)
            if near.shape[0] > 0:
                return near[:, 3].astype(int), near[:, 4].astype(int), k
            rad += 100e3
            k += 1
    finally:
        so.STABLE_TIES = saved


@functools.lru_cache(maxsize=None)
def layout(lid):
    """dict(xx, yy, grid, radius, num_points, cells, nb): the data layouts, all on 48 x 48 tie-free grids of 500 m columns, with at
    most MAX_CELLS listed cells (flat indices, ascending) and nb[k] = (rows, columns, widenings) of cell k's neighbours.
        a  sgs_common.driver_problem's lines (every 8th row, every 16th column), 48 points within 30 km: n = 48
        b  values on a lattice 8 rows by 16 columns apart in the grid's upper part and one lone value in the far corner, 8 points
           (one per octant) within 9 km: every n from 1 to 8, and cells that find nothing within the radius and widen
        c  a's lines at 20 points, 2 per octant: n = 16
        d  a's lines on descending y, 16 points"""
    H = 48
    prob = sc.driver_problem(H, dy=sc.TIE_FREE_DY)
    xx = np.ascontiguousarray(prob["xx"], dtype=np.float64)
    yy = np.ascontiguousarray(prob["yy"], dtype=np.float64)
    grid = prob["cond_bed"].copy()
    radius, num_points = 30e3, {"a": 48, "b": 8, "c": 20, "d": 16}[lid]
    if lid == "b":
        radius = 9e3
        has = np.zeros((H, H), bool)
        has[0:25:8, 0:33:16] = True
        has[H - 1, H - 1] = True
        grid = np.where(has, prob["bed"], np.nan)
    if lid == "d":
        yy = np.ascontiguousarray(yy[::-1])
    free = np.flatnonzero(np.isnan(grid).ravel())
    if lid == "b":
        found = [search(xx, yy, grid, c // H, c % H, radius, num_points) for c in free]
        n_of = np.array([f[0].size for f in found])
        wide = np.array([f[2] for f in found])
        pick = [free[wide > 0][:4]] + [_spread(free[(n_of == n) & (wide == 0)], 7) for n in range(1, 9)]
        cells = np.unique(np.concatenate(pick))
    else:
        cells = _spread(free, MAX_CELLS)
    assert 0 < cells.size <= MAX_CELLS
    nb = [search(xx, yy, grid, c // H, c % H, radius, num_points) for c in cells]
    return dict(xx=xx, yy=yy, grid=grid, radius=radius, num_points=num_points, cells=np.ascontiguousarray(cells, dtype=np.int32), nb=nb)


def plan_of(lid, vario, ktype):
    """interpolate._Plan of a layout: the device's inputs (normal scores, axes, global mean, per-cell table) made on the host."""
    L = layout(lid)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                  # fewer conditioning values than the transformer's 500 quantiles
        return kc.plan_of(L["xx"], L["yy"], L["grid"], vario, dict(radius=L["radius"], num_points=L["num_points"], ktype=ktype))


def local_vario(lid, vtype, maps):
    """A variogram of parameter maps for layout `lid`: nonstationary_common's smooth maps ('smooth'; the Gaussian model at a
    quarter of the ranges, as there) or the same variogram at every cell ('constant', through the per-cell path all the same)."""
    H, W = layout(lid)["grid"].shape
    if maps == "smooth":
        return nc.vario_of(H, W, vtype, 0.25 if vtype == "Gaussian" else 1.0)
    base = dict(MODELS["exp_aniso"], vtype=vtype)
    if vtype == "Gaussian":
        base.update(major_range=2000.0, minor_range=1250.0)
    return {k: (v if k == "vtype" else np.full((H, W), float(v))) for k, v in base.items()}


# ---- covariance forms -------------------------------------------------------------------------------------------------------------
class TableCov:
    """The lag-table form: entries of sgs.lag_cov_table at extents (H - 1, W - 1), indexed as krige_solve indexes them."""

    def __init__(self, vario, hw, dx, dy, H, W):
        from mcmc_gpu_amd import sgs
        self.mi, self.mj = H - 1, W - 1
        self.table = sgs.lag_cov_table(vario, hw, dx, dy, self.mi, self.mj)
        self.sill = float(vario["sill"])
        self.c00 = float(self.table[self.mi, self.mj])

    def system(self, i0, j0, ni, nj, lagr):
        S = self.table[ni[:, None] - ni[None, :] + self.mi, nj[:, None] - nj[None, :] + self.mj]
        rho = self.table[ni - i0 + self.mi, nj - j0 + self.mj]
        return S, rho, S.astype(LD), rho.astype(LD), 0.0, self.sill, self.c00


class LocalCov:
    """The per-cell form: covariances from row `cell` of interpolate._local_table and the axes, in fp64 in krige_fill_local's
    expression order (what the host restatement solves) and in long double (what the truth solves)."""

    def __init__(self, local, vtype, xs, ys):
        self.local, self.vtype, self.xs, self.ys = local, vtype.lower(), xs, ys

    def _cov(self, h2, c0, sill, T):
        h = np.sqrt(h2)
        if self.vtype == "exponential":
            return c0 * np.exp(T(-3.0) * h)
        if self.vtype == "gaussian":
            return c0 * np.exp(T(-3.0) * (h * h))
        c = c0 - T(1.5) * h + T(0.5) * (h * h * h)
        return np.where(h > 1.0, sill - T(1.0), c)

    def _entries(self, i0, j0, ni, nj, T):
        W = self.xs.size
        R00, R01, R10, R11, sill, nug = (T(v) for v in self.local[i0 * W + j0])
        x, y = self.xs[nj].astype(T), self.ys[ni].astype(T)

        def pair(ddx, ddy):
            u, v = ddx * R00 + ddy * R10, ddx * R01 + ddy * R11
            h2 = u * u + v * v
            return self._cov(h2, sill - nug, sill, T), h2
        S, h2s = pair(x[:, None] - x[None, :], y[:, None] - y[None, :])
        rho, h2r = pair(x - T(self.xs[j0]), y - T(self.ys[i0]))
        return S, rho, float(np.sqrt(max(h2s.max(), h2r.max()))), float(sill), float(sill - nug)

    def system(self, i0, j0, ni, nj, lagr):
        S, rho, h_max, sill, c0 = self._entries(i0, j0, ni, nj, np.float64)
        S_ld, rho_ld, _, _, _ = self._entries(i0, j0, ni, nj, LD)
        if self.vtype == "spherical":
            hs = min(h_max, 1.0)
            err = 4 * EPS * (abs(c0) + 1.5 * hs + 0.5 * hs ** 3) + 6.0 * hs * U          # of an entry, absolute
            b_norm = max(float(np.max(np.abs(rho))), 1.0 if lagr else 0.0)
            E = err / abs(c0) + (err / b_norm if b_norm > 0 else 0.0)
        else:
            E = 2.0 * (4 * EPS * (1.0 + 3.0 * (h_max if self.vtype == "exponential" else h_max * h_max)) + 6.0 * h_max * U)
        return S, rho, S_ld, rho_ld, E, sill, c0


# ---- solvers ----------------------------------------------------------------------------------------------------------------------
def _assemble(S, rho, lagr, T):
    n = rho.size
    if not lagr:
        return np.array(S, dtype=T), np.array(rho, dtype=T)
    A = np.zeros((n + 1, n + 1), dtype=T)
    A[:n, :n] = S
    A[:n, n] = 1
    A[n, :n] = 1
    b = np.ones(n + 1, dtype=T)
    b[:n] = rho
    return A, b


def _lu(A):
    A = A.copy()
    n = A.shape[0]
    p = np.arange(n)
    for k in range(n - 1):
        m = k + int(np.argmax(np.abs(A[k:, k])))
        if m != k:
            A[[k, m]] = A[[m, k]]
            p[[k, m]] = p[[m, k]]
        if A[k, k] != 0:
            A[k + 1:, k] /= A[k, k]
            A[k + 1:, k + 1:] -= A[k + 1:, k, None] * A[None, k, k + 1:]
    return A, p


def _lu_solve(LU, p, b):
    x = b[p].copy()
    n = x.size
    for k in range(1, n):
        x[k] -= np.sum(LU[k, :k] * x[:k])
    for k in range(n - 1, -1, -1):
        x[k] = (x[k] - np.sum(LU[k, k + 1:] * x[k + 1:])) / LU[k, k]
    return x


def solve_ld(A, b):
    """A x = b in long double: partial pivoting and three refinement steps.  Returns (x, max|A x - b| / (||A||_inf ||x||_inf))."""
    LU, p = _lu(A)
    with np.errstate(all="ignore"):
        x = _lu_solve(LU, p, b)
        for _ in range(3):
            x = x + _lu_solve(LU, p, b - A @ x)
        res = np.max(np.abs(A @ x - b)) / (np.max(np.sum(np.abs(A), axis=1)) * np.max(np.abs(x)))
    return x, float(res)


def host_solve(S, rho, lagr, c00):
    """krige_solve restated in NumPy fp64: Gauss-Jordan on the diagonal in the device's order (covariance pivots 0 .. n - 1, then
    the Lagrange row), no pivoting, the device's pivot test, w = r[49] / pivot.  Returns the n weights, or None where the device
    would refuse."""
    n = rho.size
    A, b = _assemble(S, rho, lagr, np.float64)
    M = np.concatenate([A, b[:, None]], axis=1)
    rows = M.shape[0]
    tol, tol_l = EPS * (n + 1) * abs(c00), EPS * (n + 1) / abs(c00)
    piv = np.ones(rows)
    for K in range(rows):
        pv = M[K, K]
        if not abs(pv) > (tol_l if K == n else tol):
            return None
        f = M[:, K] / pv
        f[K] = 0.0
        piv[K] = pv
        M[:, K + 1:] -= f[:, None] * M[None, K, K + 1:]
    return (M[:, -1] / piv)[:n]


def finish(w, rho, v, mean, sill):
    """Estimate and variance from the weights as the kernels form them: sum w v + (1 - sum w) mean, sill - sum w rho."""
    return np.sum(w * v) + (1 - np.sum(w)) * mean, sill - np.sum(w * rho)


Rec = namedtuple("Rec", "n w est var kappa b_est b_var resid host lstsq")
Rec.__doc__ = """One cell's truth: n, w* (fp64 copy), est*, var* (long double), kappa, the two bars, the
truth's relative residual, and (est, var) of host_solve (None: refused) and of numpy.linalg.lstsq on the fp64 system."""


def solve_cell(cov, i0, j0, ni, nj, v, ktype, gmean):
    """Truth, bars and the two fp64 solves of the system of cell (i0, j0) with neighbours (ni, nj) holding the values v."""
    lagr = ktype == "ok"
    ni, nj, v = np.asarray(ni), np.asarray(nj), np.asarray(v, dtype=np.float64)
    n = v.size
    S, rho, S_ld, rho_ld, E, sill, c00 = cov.system(i0, j0, ni, nj, lagr)
    A, b = _assemble(S, rho, lagr, np.float64)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        kappa = float(np.linalg.cond(A))
        x, resid = solve_ld(*_assemble(S_ld, rho_ld, lagr, LD))
        w = x[:n]
        mean = LD(np.mean(v) if lagr else gmean)
        est, var = finish(w, rho_ld, v.astype(LD), mean, LD(sill))
        l1 = float(np.sum(np.abs(w)))
        c = ((n + 3) * U + E) * (kappa if np.isfinite(kappa) else np.inf)
        b_est = c * (l1 * float(np.max(np.abs(v))) + (0.0 if lagr else (1.0 + l1) * abs(float(gmean))))
        b_var = c * sill * (1.0 + l1)
        wh = host_solve(S, rho, lagr, c00)
        host = None if wh is None else finish(wh, rho, v, float(mean), sill)
        wl = np.linalg.lstsq(A, b, rcond=None)[0][:n]
        lsq = finish(wl, rho, v, float(mean), sill)
    return Rec(n, w.astype(np.float64), est, var, kappa, b_est, b_var, resid, host, lsq)


# ---- the truth of the whole-grid kriging cases -------------------------------------------------------------------------------------
def _cells_truth(lid, plan, cov, ktype):
    L = layout(lid)
    out = []
    for c, (ni, nj, _) in zip(L["cells"], L["nb"]):
        out.append(solve_cell(cov, int(c) // plan.W, int(c) % plan.W, ni, nj, plan.grid_ns[ni, nj], ktype, plan.global_mean))
    return out


def table_cov(plan, vario):
    import math
    return TableCov(vario, int(math.ceil(plan.radius / abs(plan.dx))), plan.dx, plan.dy, plan.H, plan.W)


@functools.lru_cache(maxsize=None)
def truth(lid, mid, ktype):
    """The Recs of layout lid's listed cells under MODELS[mid] (one lag table)."""
    plan = plan_of(lid, MODELS[mid], ktype)
    return _cells_truth(lid, plan, table_cov(plan, plan.vario), ktype)


@functools.lru_cache(maxsize=None)
def truth_local(lid, vtype, maps, ktype):
    """The Recs of layout lid's listed cells under local_vario(lid, vtype, maps) (a variogram per cell)."""
    plan = plan_of(lid, local_vario(lid, vtype, maps), ktype)
    return _cells_truth(lid, plan, LocalCov(plan.local, vtype, plan.xs, plan.ys), ktype)


# ---- cross-validation ---------------------------------------------------------------------------------------------------------------
CV_LAYOUT = "a"
CV_MODELS = tuple(f"gau{int(r)}" for r in GAUSSIAN_RANGES) + ("exp9k", "sph9k", "exp_aniso")
CV_LOCAL = (("Exponential", "smooth"), ("Gaussian", "smooth"), ("Spherical", "constant"))


@functools.lru_cache(maxsize=None)
def cv_targets():
    """(targets, nb): some 40 data cells of the cross-validation layout (krige_cv_common.pick_targets: corners, border, line ends,
    the rest evenly), and the neighbours of each with the target held out."""
    L = layout(CV_LAYOUT)
    W = L["grid"].shape[1]
    xs, ys = L["xx"][0, :], L["yy"][:, 0]
    targets = np.ascontiguousarray(kcv.pick_targets(~np.isnan(L["grid"]), 40), dtype=np.int32)
    nb = []
    for t in targets:
        held = kcv.held_out(L["grid"], xs, ys, int(t))
        nb.append(search(L["xx"], L["yy"], held, int(t) // W, int(t) % W, L["radius"], L["num_points"]))
    return targets, nb


def _cv_truth(plan, covs, ktype):
    targets, nb = cv_targets()
    return [[solve_cell(cov, int(t) // plan.W, int(t) % plan.W, ni, nj, plan.grid_ns[ni, nj], ktype, plan.global_mean)
             for t, (ni, nj, _) in zip(targets, nb)] for cov in covs]


@functools.lru_cache(maxsize=None)
def cv_truth(ktype):
    """[model][target] Recs of leave-one-out under CV_MODELS.  The transformer and the global mean are the plan's, fitted on all
    data (interpolate.cross_validate's convention)."""
    plan = plan_of(CV_LAYOUT, MODELS[CV_MODELS[0]], ktype)
    return _cv_truth(plan, [table_cov(plan, MODELS[m]) for m in CV_MODELS], ktype)


def cv_local_varios():
    return [local_vario(CV_LAYOUT, vt, maps) for vt, maps in CV_LOCAL]


@functools.lru_cache(maxsize=None)
def cv_truth_local(ktype):
    from mcmc_gpu_amd import interpolate
    varios = cv_local_varios()
    plan = plan_of(CV_LAYOUT, varios[0], ktype)
    covs = [LocalCov(interpolate._local_table(v, (plan.H, plan.W)), v["vtype"], plan.xs, plan.ys) for v in varios]
    return _cv_truth(plan, covs, ktype)


# ---- comparison ---------------------------------------------------------------------------------------------------------------------
def ratios(recs, est, var, n, what):
    """Largest |est - est*| / B_est and |var - var*| / B_var over the cells with kappa <= KAPPA_REFUSE, after the assertions that
    hold whatever the numbers: the neighbour count of every solved cell, no refusal (NaN) at kappa <= 1e12, refused or finite
    up to 1e16.  Beyond 1e12 the errors of `what` and of lstsq are printed, not asserted."""
    r_est = r_var = 0.0
    for k, rec in enumerate(recs):
        refused = bool(np.isnan(est[k]))
        if not refused and n is not None:
            assert n[k] == rec.n, f"{what}: cell {k}: {n[k]} neighbours, the reference's search finds {rec.n}"
        if rec.kappa > KAPPA_REFUSE:
            if rec.kappa < KAPPA_FINITE:
                assert refused or (np.isfinite(est[k]) and np.isfinite(var[k])), f"{what}: cell {k}: neither refused nor finite"
            got = "refused" if refused else f"|est err| {float(abs(LD(est[k]) - rec.est)):.2e} |var err| {float(abs(LD(var[k]) - rec.var)):.2e}"
            print(f"  {what}: cell {k} n {rec.n} cond {rec.kappa:.2e}: {got}; lstsq |est err| {float(abs(LD(rec.lstsq[0]) - rec.est)):.2e} "
                  f"|var err| {float(abs(LD(rec.lstsq[1]) - rec.var)):.2e}; bars {rec.b_est:.2e} {rec.b_var:.2e}")
            continue
        assert not refused, f"{what}: cell {k}: refused a system of condition number {rec.kappa:.2e}"
        r_est = max(r_est, float(abs(LD(est[k]) - rec.est) / rec.b_est))
        r_var = max(r_var, float(abs(LD(var[k]) - rec.var) / rec.b_var))
    return r_est, r_var


def host_arrays(recs):
    """(est, var) of host_solve over recs, NaN where it refuses."""
    est = np.array([np.nan if r.host is None else r.host[0] for r in recs])
    var = np.array([np.nan if r.host is None else r.host[1] for r in recs])
    return est, var
