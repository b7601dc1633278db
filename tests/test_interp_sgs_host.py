"""CPU: the host side of mcmc_gpu_amd.interpolate -- csrc/truncnorm.h (the device's truncated-normal ppf, compiled for the host with
g++) against scipy.stats.truncnorm.ppf, and the draw plan (visiting order, draws, generator advance) and argument errors of
interpolate.sgs against golden F14 (the unmodified reference, scripts/make_fixtures_interp_sgs.py)."""
import ctypes as C
import json
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import interp_sgs_common as ic

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
st = pytest.importorskip("scipy.stats")
sp = pytest.importorskip("scipy.special")
pytest.importorskip("sklearn.preprocessing")
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not found")
    so = tmp_path_factory.mktemp("tn") / "libtn.so"
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", str(ROOT / "mcmc_gpu_amd" / "csrc"), "-o", str(so),
                    str(ROOT / "tests" / "native" / "truncnorm_host.cpp")], check=True)
    L = C.CDLL(str(so))
    dp = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
    L.tn_ppf.argtypes = [dp, dp, dp, dp, C.c_int]
    L.tn_log_ndtr.argtypes = [dp, dp, C.c_int]
    L.tn_ndtri_exp.argtypes = [dp, dp, C.c_int]
    return L


def _ppf(lib, q, a, b):
    shp = np.broadcast_shapes(np.shape(q), np.shape(a), np.shape(b))
    q, a, b = (np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), shp)) for v in (q, a, b))
    out = np.empty_like(q)
    lib.tn_ppf(q, a, b, out, q.size)
    return q, a, b, out


def test_log_ndtr_and_ndtri_exp_equal_scipy(lib):
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.uniform(-40, 10, 100000), -(10.0 ** rng.uniform(0, 3, 20000)), [0.0, -1.0, 1.0, -38.0, np.inf, -np.inf]])
    out = np.empty_like(x); lib.tn_log_ndtr(x, out, x.size)
    ref = sp.log_ndtr(x)
    fin = np.isfinite(ref)
    assert np.array_equal(out[~fin], ref[~fin])
    # 16 ulp: erfcx for x < -1 is Cephes erfc's rational function where scipy evaluates the Faddeeva package's
    assert np.max(np.abs(out[fin] - ref[fin]) / np.spacing(np.abs(ref[fin]))) <= 16
    y = np.concatenate([-(10.0 ** rng.uniform(-300, 300, 100000)), rng.uniform(-3, 0, 50000), [-2.0, -0.14541345786885906, 0.0, -np.inf]])
    out = np.empty_like(y); lib.tn_ndtri_exp(y, out, y.size)
    np.testing.assert_array_equal(out, sp.ndtri_exp(y))


@pytest.mark.parametrize("region", ["general", "deep_right", "deep_left", "infinite", "narrow"])
def test_truncnorm_ppf_equals_scipy(lib, region):
    """|device - scipy| <= 4 eps (max(1, |x|) + (1 + |log Phi at the far bound|) c(x)), c(x) = Phi(x) / phi(x) in scipy's left
    branch (a < 0) and Phi(-x) / phi(x) in its right branch: both evaluate x = ndtri_exp(y) of a log-CDF y that is summed from
    O(1) logs, so y carries a few eps absolutely and x inherits them times dx/dy = c(x).  c(x) <= 1.3 wherever x <= 0 in the left
    branch or x >= 0 in the right one: a few ulp there.  Where Phi(x) rounds to 1 in the left branch (eps c(x) > 1e-6, x > ~7.5)
    the quantile is set by that rounding and scipy itself returns 8.2, inf or nan for neighbouring q: those are left out."""
    rng = np.random.default_rng(7)
    n = 60000
    q = np.concatenate([rng.random(n), 10.0 ** rng.uniform(-300, 0, n), 1.0 - 10.0 ** rng.uniform(-16, 0, n),
                        [0.0, 1.0, 1e-300, 1.0 - 1e-16, 0.5]])
    m = q.size
    if region == "general":
        a = rng.uniform(-6, 3, m); b = a + 10.0 ** rng.uniform(-3, 1.5, m)
    elif region == "deep_right":                                      # a up to 30, b infinite or far
        a = rng.uniform(0, 30, m); b = np.where(rng.random(m) < 0.5, np.inf, a + rng.uniform(0.1, 10, m))
    elif region == "deep_left":                                       # b down to -30
        b = rng.uniform(-30, 0, m); a = np.where(rng.random(m) < 0.5, -np.inf, b - rng.uniform(0.1, 10, m))
    elif region == "infinite":
        a, b = np.full(m, -np.inf), np.full(m, np.inf)
    else:                                                             # b - a = 1e-8
        a = rng.uniform(-8, 8, m); b = a + 1e-8
    q, a, b, got = _ppf(lib, q, a, b)
    with np.errstate(all="ignore"):
        ref = st.truncnorm.ppf(q, a, b)
        left = a < 0
        c = np.where(left, np.exp(sp.log_ndtr(ref) - st.norm.logpdf(ref)), np.exp(sp.log_ndtr(-ref) - st.norm.logpdf(ref)))
        y = 1.0 + np.abs(np.where(left, sp.log_ndtr(a), sp.log_ndtr(-b)))
        tol = 4 * EPS * (np.maximum(1.0, np.abs(ref)) + y * c)
    fin = np.isfinite(ref)
    keep = fin & ~(left & (EPS * c > 1e-6))
    assert keep.sum() > 0.8 * m
    bad = np.flatnonzero(keep & ~(np.abs(got - ref) <= tol))
    assert bad.size == 0, [(q[i], a[i], b[i], got[i], ref[i]) for i in bad[:5]]
    # infinities where scipy returns them (q = 0 / 1 at an infinite bound); not scipy's inf / nan for q near 1 below a finite b
    nf = ~fin & ~(left & np.isfinite(b) & (q > 0.5))
    np.testing.assert_array_equal(got[nf], ref[nf])


def _case(tag):
    xx, yy, grid, cases = (ic.t2_like() if tag == "d" else ic.small())
    vario, kw, seeds = cases[tag]
    return xx, yy, grid, vario, kw, seeds, np.load(GOLD / f"f14{tag}_interp_sgs.npz", allow_pickle=False)


@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_draw_plan_follows_the_reference(tag):
    """Visiting order, number of draws and the generator's final state of every seed of F14 -- the host half of interpolate.sgs."""
    from mcmc_gpu_amd import interpolate
    xx, yy, grid, vario, kw, seeds, g = _case(tag)
    plan = interpolate._Plan(xx, yy, grid, vario, kw["radius"], kw["num_points"], kw["ktype"], kw.get("sim_mask"), None, None,
                             kw.get("bounds"))
    for s in seeds:
        rng = np.random.default_rng(s)
        path, draws = plan.draws(rng)
        assert json.loads(str(g[f"{s}_state"])) == rng.bit_generator.state
        if f"{s}_cells" in g.files:
            np.testing.assert_array_equal(path, g[f"{s}_cells"])
        assert draws.size == path.size
        if plan.bounds is not None:
            lo, hi = plan.bounds
            deg = lo.ravel()[path] == hi.ravel()[path]
            assert (deg.any() if tag == "b" else True) and np.all(draws[deg] == 0.0)
            assert np.all((draws[~deg] >= 0.0) & (draws[~deg] < 1.0))


def test_transformed_bounds_clip_outside_the_data():
    from mcmc_gpu_amd import interpolate
    xx, yy, grid, vario, kw, seeds, _ = _case("b")
    plan = interpolate._Plan(xx, yy, grid, vario, kw["radius"], kw["num_points"], kw["ktype"], None, None, None, kw["bounds"])
    lo, hi = plan.bounds
    assert np.all(lo == lo.min())                               # a number below the data: one score everywhere
    assert np.all(lo[30:36, 2:9] == hi[30:36, 2:9]) and np.count_nonzero(lo == hi) == 42
    assert plan.global_mean == pytest.approx(np.mean(plan.grid_ns[~np.isnan(grid)]))


def test_argument_errors_follow_the_reference():
    from mcmc_gpu_amd import interpolate
    xx, yy, grid, vario, kw, _, _ = _case("a")
    run = lambda **o: interpolate.sgs(**{**dict(xx=xx, yy=yy, grid=grid, variogram=vario, radius=3000.0, num_points=16, seed=1), **o})
    cases = [
        (dict(xx=xx[0]), ValueError, "xx must be a 2D NumPy array"),
        (dict(yy=list(yy)), ValueError, "yy must be a 2D NumPy array"),
        (dict(grid=grid[:, :-1]), ValueError, "xx, yy, and grid must have same shape"),
        (dict(variogram={k: v for k, v in vario.items() if k not in ("sill", "azimuth")}), ValueError, "Variogram missing azimuth, sill"),
        (dict(variogram={**vario, "vtype": "Cubic"}), ValueError, "vtype must be exponential"),
        (dict(variogram={k: v for k, v in vario.items() if k != "s"}), ValueError, "Matern covariance requires the s parameter"),
        (dict(variogram={**vario, "nugget": np.nan}), ValueError, "variogram parameter nugget is NaN"),
        (dict(sim_mask=np.ones((3, 3), bool)), ValueError, "sim_mask shape must be same as grid"),
        (dict(sim_mask=[[True]]), ValueError, "sim_mask must be None or a 2D array"),
        (dict(radius="far"), ValueError, "radius must be a number"),
        (dict(num_points=None), ValueError, "num_points must be a number"),
        (dict(ktype="uk"), ValueError, "ktype must be 'ok' or 'sk'"),
        (dict(bounds=(0.0,)), ValueError, "bounds must be None or a 2D numpy array"),
        (dict(bounds=(0.0, np.zeros((3, 3)))), ValueError, "bounds must be None or a 2D numpy array"),
        (dict(bounds=(0.0, "high")), ValueError, "bounds must be None or a 2D numpy array"),
        (dict(seed=np.int64(3)), ValueError, "Seed should be an integer"),
        (dict(grid=np.full(grid.shape, np.nan)), ValueError, "no conditioning value"),
        (dict(stencil=np.ones((5, 5))), NotImplementedError, "stencil"),
        (dict(rcond=1e-10), NotImplementedError, "rcond"),
        (dict(variogram={**vario, "sill": np.ones(grid.shape)}), NotImplementedError, "scalar variogram"),
        (dict(num_points=4), NotImplementedError, "num_points"),
        (dict(num_points=64), NotImplementedError, "num_points"),
    ]
    for over, exc, msg in cases:
        with pytest.raises(exc, match=msg.replace("(", r"\(").replace(")", r"\)")):
            run(**over)
    with pytest.raises(ValueError, match="segment_cells"):
        interpolate.sgs_many(xx, yy, grid, vario, [1], radius=3000.0, num_points=16, segment_cells=0)


def test_sgs_many_of_no_seed_is_empty():
    from mcmc_gpu_amd import interpolate
    xx, yy, grid, vario, kw, _, _ = _case("a")
    assert interpolate.sgs_many(xx, yy, grid, vario, [], radius=3000.0, num_points=16).shape == (0,) + grid.shape


def test_regime_case_reaches_the_deep_tails_and_narrow_intervals():
    """interp_sgs_common.regimes(): in the CPU helper's trace at least 20 simulated cells each draw from a standardised interval
    with a >= 6, with b <= -6 and with b - a <= 1e-3 -- what tests/test_gpu_interp_sgs_geometry.py then runs on the device."""
    c = ic.regimes()
    tr = c["trace"]
    lo, hi = c["plan"].bounds
    i, j = tr[:, 0].astype(int), tr[:, 1].astype(int)
    sd = np.sqrt(tr[:, 4])
    a, b = (lo[i, j] - tr[:, 3]) / sd, (hi[i, j] - tr[:, 3]) / sd
    assert tr.shape[0] == 420 and np.all(tr[:, 2] > 0) and np.all(a < b)
    assert np.count_nonzero(a >= 6.0) >= 20 and np.count_nonzero(b <= -6.0) >= 20 and np.count_nonzero(b - a <= 1e-3) >= 20
    # the tails in both forms: open-ended and a narrow interval far out
    assert np.count_nonzero((a >= 6.0) & np.isinf(b)) >= 20 and np.count_nonzero((b <= -6.0) & np.isinf(a)) >= 20
    assert np.count_nonzero((np.minimum(np.abs(a), np.abs(b)) >= 6.0) & (b - a <= 1e-3)) >= 20
    assert np.all(np.isfinite(c["out"]))


def _lag_case(cid):
    if cid.startswith("small"):
        xx, yy, grid, cases = ic.small()
        vario, kw, seeds = cases[cid[-1]]
        return xx, yy, grid, vario, kw, seeds[0]
    xx, yy, grid, vario, kw, _ = ic.geometry()[cid]
    return xx, yy, grid, vario, kw, 5


@pytest.mark.parametrize("cid", ["small_a", "small_c", "G3", "G5", "G7"])
def test_lag_table_reaches_every_lag_of_the_reference_search(cid):
    """interpolate._lag_extents_from on KD-tree distances (what gsm_min_dist_from_mask returns, test_min_dist_device_equals_kdtree)
    against the neighbours the oracle's search actually chooses: every lag between a cell and a chosen neighbour and between two
    chosen neighbours fits the table.  G7: rows 250 m apart under a 3 km radius and a +-6-cell window -- values inside the radius
    but outside the window, searches that come back empty and widen by 100 km.  The Euclidean distance alone (2062 m at most)
    says no search widens there."""
    import warnings
    from scipy.spatial import cKDTree
    import sgs_oracle as so
    from mcmc_gpu_amd import interpolate
    xx, yy, grid, vario, kw, seed = _lag_case(cid)
    plan = interpolate._Plan(xx, yy, grid, vario, kw["radius"], kw["num_points"], kw["ktype"], kw.get("sim_mask"), None, None,
                             kw.get("bounds"))
    H, W = plan.H, plan.W
    rows = interpolate._window_rows(plan.ys, plan.dx, plan.dy)
    pts = np.stack([np.broadcast_to(plan.xs[None, :], (H, W)).ravel(), np.broadcast_to(rows[:, None], (H, W)).ravel()], axis=1)
    d = cKDTree(pts[plan.cond.ravel()]).query(pts[~plan.cond.ravel()])[0]
    mi, mj = interpolate._lag_extents_from(d, plan.radius, plan.dx, H, W)
    # never smaller than the table of the Euclidean distance on the grid's own rows
    pts0 = np.stack([xx.ravel(), yy.ravel()], axis=1)
    d0 = cKDTree(pts0[plan.cond.ravel()]).query(pts0[~plan.cond.ravel()])[0]
    mi0, mj0 = interpolate._lag_extents_from(d0, plan.radius, plan.dx, H, W)
    assert mi >= mi0 and mj >= mj0
    if abs(plan.dy) >= abs(plan.dx):
        assert (mi, mj) == (mi0, mj0)
    so.STABLE_TIES, so.NBR_LOG = True, []
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            so.sgs(xx, yy, plan.grid_ns, dict(vario), kw["radius"], kw["num_points"], kw["ktype"], sim_mask=kw.get("sim_mask"),
                   rng=np.random.default_rng(seed), bounds=plan.bounds)
        log = so.NBR_LOG
    finally:
        so.STABLE_TIES, so.NBR_LOG = False, None
    need_i = need_j = 0
    for i, j, nb in log:
        if nb:
            a = np.array(nb + [(i, j)])
            need_i, need_j = max(need_i, int(np.ptp(a[:, 0]))), max(need_j, int(np.ptp(a[:, 1])))
    assert 0 < need_i <= mi and 0 < need_j <= mj, (need_i, need_j, mi, mj)
    if cid == "G7":
        assert need_i > mi0, "the case no longer needs more rows than the Euclidean rule gives"
