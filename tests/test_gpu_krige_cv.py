"""GPU: gsm_krige_cv / gsm_krige_cv_local (csrc/krige_cv_kernel.hip) and interpolate.cross_validate.

Through the C ABI in normal-score space, device against device, every comparison an equality: a hold-out is what gsm_krige_grid
computes on a copy of the grid with the held-out cells set to NaN (the composition) -- per fold, and per target for
leave-one-out and the buffered hold-out --, model m of a many-model call is the one-model call, and the widened search of a
target whose every datum within the radius is excluded is the composition's.  Against the CPU restatement of
tests/krige_cv_common.py at the bounds of tests/test_gpu_krige.py.  Then the refusals, the device-found errors, the public
function end to end, and krige_scores against bits recorded from the parent commit."""
import ctypes as C
import functools
import math
import warnings
from pathlib import Path

import numpy as np
import pytest

import interp_sgs_common as ic
import krige_common as kc
import krige_cv_common as cc

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
E_ARG, E_STATE, E_UNSUPPORTED, E_DEVICE_DATA = -1, -2, -4, -5
SENTINEL, SENTINEL_I = -12345.5, -77


def _mapped(v, shape):
    """v with its ranges and azimuth as smooth maps (the per-cell form)."""
    i, j = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
    s = 1.0 + 0.3 * np.sin(0.21 * i + 0.13 * j)
    return dict(v, major_range=v["major_range"] * s, minor_range=v["minor_range"] * (2.0 - s), azimuth=v["azimuth"] + 25.0 * np.cos(0.17 * j))


class _World:
    """One handle on a case's grid with the operands both entry points take, all in normal scores."""

    def __init__(self, cid):
        import torch
        from mcmc_gpu_amd.engine import GsmEngine
        c = cc.cases()[cid]
        self.torch, self.case = torch, c
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                                              # fewer data than the transformer's quantiles
            plan = kc.plan_of(c["xx"], c["yy"], c["grid"], c["vario"], c["kw"])
        self.plan, self.H, self.W = plan, plan.H, plan.W
        self.grid_ns, self.cond = plan.grid_ns, plan.cond
        self.data = np.flatnonzero(plan.cond).astype(np.int32)
        self.radius, self.num_points = plan.radius, plan.num_points
        self.hw = int(math.ceil(plan.radius / abs(plan.dx)))
        self.eng = GsmEngine(plan.H, plan.W, 1)
        self.dev = self.eng.dev
        self.xs, self.ys, self.gm = self.f64(plan.xs), self.f64(plan.ys), self.f64([plan.global_mean])
        self.d_grid = self.f64(plan.grid_ns)
        self._tabs = {}

    def f64(self, a):
        return self.torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(self.dev)

    def i32(self, a):
        return self.torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32)).to(self.dev)

    def models(self, form):
        """The case's own model in the table form; an exponential one with parameter maps in the per-cell form."""
        return [self.case["vario"]] if form == "table" else [cc.MODELS[0]]

    def operands(self, form, models):
        """(device tables [M, ...], host sills or vtypes) of `models`, whole-grid lag tables or per-cell tables."""
        from mcmc_gpu_amd import interpolate, sgs
        key = (form, tuple(id(m) for m in models))
        if key not in self._tabs:
            if form == "table":
                tab = np.stack([sgs.lag_cov_table(m, self.hw, self.plan.dx, self.plan.dy, self.H - 1, self.W - 1) for m in models])
                host = [float(m["sill"]) for m in models]
            else:
                tab = np.stack([interpolate._local_table(_mapped(m, (self.H, self.W)), (self.H, self.W)) for m in models])
                host = [interpolate.LOCAL_VTYPES[m["vtype"].lower()] for m in models]
            self._tabs[key] = (self.f64(tab), host, models)                              # `models` kept: the ids stay unique
        return self._tabs[key][:2]

    def set_ktype(self, ktype):
        with self.torch.cuda.device(self.dev):
            assert self.eng.lib.gsm_sgs_set_kriging(self.eng.h, 1 if ktype == "sk" else 0, C.c_void_p(self.gm.data_ptr())) == 0

    def _finish(self, rc, outs):
        text = self.eng.lib.gsm_last_error(self.eng.h).decode() if rc else ""
        return (rc, text) + tuple(o.cpu().numpy() for o in outs)

    def cv(self, targets, fold, ex, form, models, ktype="ok", radius=None, hw=None, num_points=None, **override):
        """gsm_krige_cv / _local -> (code, text, est [M, n], var [M, n], n_neighbours [n]); the outputs start as sentinels.
        override: argument name -> value in place of the valid one (the refusal rows)."""
        torch, lib = self.torch, self.eng.lib
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        tab, host = self.operands(form, models)
        M, n = len(models), len(targets)
        keep = dict(cells=self.i32(targets), fold=None if fold is None else self.i32(fold),
                    est=torch.full((M, max(n, 1)), SENTINEL, dtype=torch.float64, device=self.dev),
                    var=torch.full((M, max(n, 1)), SENTINEL, dtype=torch.float64, device=self.dev),
                    cnt=torch.full((max(n, 1),), SENTINEL_I, dtype=torch.int32, device=self.dev))
        a = dict(grid=p(self.d_grid), cells=p(keep["cells"]), n_cells=n, fold=p(keep["fold"]), exclude_radius=float(ex), x_axis=p(self.xs),
                 y_axis=p(self.ys), n_models=M, tab=p(tab))
        if form == "table":
            a.update(lag_mi=self.H - 1, lag_mj=self.W - 1)
        else:
            a.update(vtype=(C.c_int32 * M)(*host))
        a.update(hw=self.hw if hw is None else hw, radius=self.radius if radius is None else radius,
                 num_points=self.num_points if num_points is None else num_points)
        if form == "table":
            a.update(sill=(C.c_double * M)(*host))
        a.update(est=p(keep["est"]), var=p(keep["var"]), n_neighbours=p(keep["cnt"]))
        assert set(override) <= set(a), override
        a.update(override)
        self.set_ktype(ktype)
        with torch.cuda.device(self.dev):
            rc = getattr(lib, "gsm_krige_cv" if form == "table" else "gsm_krige_cv_local")(self.eng.h, *a.values(), self.eng._stream())
        return self._finish(rc, (keep["est"][:, :n], keep["var"][:, :n], keep["cnt"][:n]))

    def krige(self, grid_ns, cells, form, model, ktype="ok", radius=None, hw=None):
        """gsm_krige_grid / _local on `grid_ns` with the operands cv() uses -> (code, text, est [n], var [n], n_neighbours [n])."""
        torch, lib = self.torch, self.eng.lib
        p = lambda t: C.c_void_p(t.data_ptr())
        tab, host = self.operands(form, [model])
        n = len(cells)
        d_grid, d_cells = self.f64(grid_ns), self.i32(cells)
        est = torch.full((n,), SENTINEL, dtype=torch.float64, device=self.dev)
        var = torch.full((n,), SENTINEL, dtype=torch.float64, device=self.dev)
        cnt = torch.full((n,), SENTINEL_I, dtype=torch.int32, device=self.dev)
        hw, radius = self.hw if hw is None else hw, self.radius if radius is None else radius
        self.set_ktype(ktype)
        with torch.cuda.device(self.dev):
            if form == "table":
                rc = lib.gsm_krige_grid(self.eng.h, p(d_grid), p(d_cells), n, p(self.xs), p(self.ys), p(tab), self.H - 1, self.W - 1, hw, radius,
                                        self.num_points, host[0], p(est), p(var), p(cnt), self.eng._stream())
            else:
                rc = lib.gsm_krige_grid_local(self.eng.h, p(d_grid), p(d_cells), n, p(self.xs), p(self.ys), p(tab), host[0], hw, radius,
                                              self.num_points, p(est), p(var), p(cnt), self.eng._stream())
        return self._finish(rc, (est, var, cnt))


@functools.lru_cache(maxsize=None)
def world(cid):
    return _World(cid)


def _ok(res):
    assert res[0] == 0, res[:2]
    return res[2:]


def _folds(w, kind):
    from mcmc_gpu_amd import interpolate
    if kind == "block":
        return interpolate.block_folds((w.H, w.W), block=(8, 9), k=4, seed=2), 4
    return interpolate.random_folds(w.cond, k=5, seed=2), 5


# ---- folds: bit for bit the composition ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["table", "local"])
@pytest.mark.parametrize("cid", sorted(cc.cases()))
def test_fold_hold_out_equals_krige_grid_on_nan_copies(cid, form):
    w = world(cid)
    model = w.models(form)[0]
    for kind in ("block", "random"):
        fold, k = _folds(w, kind)
        labels = fold.ravel()[w.data]
        assert labels.min() == 0 and labels.max() == k - 1                               # every fold holds data
        for ktype in ("ok", "sk"):
            est, var, n = _ok(w.cv(w.data, fold.ravel(), 0.0, form, [model], ktype))
            assert n.min() >= 1 and np.isfinite(est).all() and np.isfinite(var).all()
            for f in range(k):
                at = labels == f
                g = np.where(fold == f, np.nan, w.grid_ns)
                e2, v2, n2 = _ok(w.krige(g, w.data[at], form, model, ktype))
                assert np.array_equal(n[at], n2) and np.array_equal(est[0, at], e2) and np.array_equal(var[0, at], v2), (kind, ktype, f)


# ---- leave-one-out and the buffer: bit for bit, one composition call per target ---------------------------------------------
@pytest.mark.parametrize("form", ["table", "local"])
@pytest.mark.parametrize("cid", ["L", "G3", "G2"])
def test_leave_one_out_and_buffer_equal_krige_grid_per_target(cid, form):
    w = world(cid)
    model = w.models(form)[0]
    ktype = w.case["kw"]["ktype"]                                                        # G2: simple kriging
    targets = cc.pick_targets(w.cond)
    xs, ys = w.plan.xs, w.plan.ys
    changed = 0
    for ex in (0.0, w.case["ex"]):
        est, var, n = _ok(w.cv(targets, None, ex, form, [model], ktype))
        for q, t in enumerate(targets):
            e2, v2, n2 = _ok(w.krige(cc.held_out(w.grid_ns, xs, ys, t, None, ex), [t], form, model, ktype))
            assert n[q] == n2[0] and est[0, q] == e2[0] and var[0, q] == v2[0], (ex, t)
        if ex == 0.0:
            plain = est.copy()
        else:
            changed = int((est != plain).sum())
    assert changed > targets.size // 2                                                   # the buffer is not a no-op on these targets


def test_fold_and_buffer_together_equal_krige_grid_per_target():
    w = world("L")
    fold, _ = _folds(w, "block")
    fold = fold.copy()
    fold.ravel()[w.data[::5]] = -1                                                       # data in no fold: held out only as targets
    targets = cc.pick_targets(w.cond)
    assert (fold.ravel()[targets] < 0).any() and (fold.ravel()[targets] >= 0).any()
    for form in ("table", "local"):
        model = w.models(form)[0]
        est, var, n = _ok(w.cv(targets, fold.ravel(), w.case["ex"], form, [model]))
        for q, t in enumerate(targets):
            g = cc.held_out(w.grid_ns, w.plan.xs, w.plan.ys, t, fold, w.case["ex"])
            e2, v2, n2 = _ok(w.krige(g, [t], form, model))
            assert n[q] == n2[0] and est[0, q] == e2[0] and var[0, q] == v2[0], (form, t)


# ---- against the CPU restatement -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["loo", "buffer", "folds"])
def test_equals_cpu_restatement_on_the_lines_grid(mode):
    w = world("L")
    c = w.case
    fold = _folds(w, "block")[0] if mode == "folds" else None
    ex = c["ex"] if mode == "buffer" else 0.0
    est, var, n = _ok(w.cv(w.data, None if fold is None else fold.ravel(), ex, "table", [c["vario"]]))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref_n, ref_est, ref_var = cc.cv_cpu(c["xx"], c["yy"], w.grid_ns, c["vario"], c["kw"], w.data, fold, ex)
    sill = c["vario"]["sill"]
    np.testing.assert_array_equal(n, ref_n)
    np.testing.assert_allclose(est[0], ref_est, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(var[0], ref_var, rtol=1e-7, atol=1e-9 * sill)


# ---- models ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form, models", [("table", cc.MODELS), ("local", cc.MODELS[:3])])
def test_model_m_of_a_many_model_call_is_the_one_model_call(form, models):
    w = world("L")
    fold, _ = _folds(w, "random")
    for ktype, f, ex in (("ok", None, w.case["ex"]), ("sk", fold.ravel(), 0.0)):
        est, var, n = _ok(w.cv(w.data, f, ex, form, models, ktype))
        assert est.shape == (len(models), w.data.size) and np.isfinite(est).all() and np.isfinite(var).all()
        for m, model in enumerate(models):
            e1, v1, n1 = _ok(w.cv(w.data, f, ex, form, [model], ktype))
            assert np.array_equal(n, n1)                                                 # one neighbour set for all models
            assert np.array_equal(est[m], e1[0]) and np.array_equal(var[m], v1[0]), (ktype, m)
        assert not np.array_equal(est[0], est[1]) and not np.array_equal(var[0], var[2])


# ---- widening and exhaustion ---------------------------------------------------------------------------------------------------
def test_target_with_every_datum_within_the_radius_excluded_widens():
    """Radius 2 cells, buffer 2.5 cells: the first search of every target comes back empty and the search is widened by 100 km,
    which covers the grid."""
    w = world("L")
    radius, hw, ex = 1000.0, 2, w.case["ex"]
    targets = cc.pick_targets(w.cond)[::2]
    for form in ("table", "local"):
        model = w.models(form)[0]
        est, var, n = _ok(w.cv(targets, None, ex, form, [model], radius=radius, hw=hw))
        assert n.min() >= 1 and np.isfinite(est).all()
        for q, t in enumerate(targets):
            g = cc.held_out(w.grid_ns, w.plan.xs, w.plan.ys, t, None, ex)
            e2, v2, n2 = _ok(w.krige(g, [t], form, model, radius=radius, hw=hw))
            assert n[q] == n2[0] and est[0, q] == e2[0] and var[0, q] == v2[0], (form, t)
        # without the buffer a target on a line stops at the four line cells within two cells of it; widened, it takes two
        # cells of every octant that holds data
        near = _ok(w.cv(targets, None, 0.0, form, [model], radius=radius, hw=hw))[2]
        assert (near < n).mean() > 0.5


def test_fold_that_holds_all_data_is_reported_and_the_rest_completes():
    w = world("L")
    model = w.case["vario"]
    every = np.where(w.cond, 0, -1).astype(np.int32)
    rc, text, est, var, n = w.cv(w.data, every.ravel(), 0.0, "table", [model, cc.MODELS[2]])
    assert rc == E_DEVICE_DATA and "gsm_krige_cv: a cell to validate has no value anywhere on the grid outside its hold-out" in text
    assert np.isnan(est).all() and np.isnan(var).all() and np.all(n == 0)
    # all data but one cell A: targets within the buffer of A are left nothing, the others find A alone (after widening)
    A = int(w.data[w.data.size // 2])
    fold = every.copy()
    fold.ravel()[A] = -1
    ex = w.case["ex"]
    d = np.hypot(w.plan.xs[A % w.W] - w.plan.xs[w.data % w.W], w.plan.ys[A // w.W] - w.plan.ys[w.data // w.W])
    lost = (d <= ex) & (w.data != A)
    assert 2 <= lost.sum() < w.data.size // 4
    rc, text, est, var, n = w.cv(w.data, fold.ravel(), ex, "table", [model])
    assert rc == E_DEVICE_DATA and "no value anywhere" in text
    assert np.isnan(est[0, lost]).all() and np.isnan(var[0, lost]).all() and np.all(n[lost] == 0)
    assert np.isfinite(est[0, ~lost]).all() and np.isfinite(var[0, ~lost]).all()
    found = ~lost & (w.data != A)
    assert np.all(n[found] == 1)
    np.testing.assert_allclose(est[0, found], w.grid_ns.ravel()[A], rtol=1e-12)           # ordinary kriging on one neighbour: its value
    q = int(np.flatnonzero(found)[0])
    g = cc.held_out(w.grid_ns, w.plan.xs, w.plan.ys, w.data[q], fold, ex)
    e2, v2, n2 = _ok(w.krige(g, [w.data[q]], "table", model))
    assert est[0, q] == e2[0] and var[0, q] == v2[0] and n[q] == n2[0]
    # the flag was cleared: a valid call on the same handle gives what it gave before
    again = _ok(w.cv(w.data, None, 0.0, "table", [model]))
    assert np.isfinite(again[0]).all()


def test_target_without_a_value_or_off_the_grid_is_reported():
    w = world("L")
    model = w.case["vario"]
    good = _ok(w.cv(w.data[:20], None, 0.0, "table", [model]))
    for bad, form in ((int(np.flatnonzero(~w.cond)[3]), "table"), (w.H * w.W, "table"), (-1, "local")):
        cells = w.data[:20].copy()
        cells[7] = bad
        rc, text, est, var, n = w.cv(cells, None, 0.0, form, w.models(form))
        assert rc == E_DEVICE_DATA and "a listed cell outside the grid or holding no value" in text
        assert np.isnan(est[0, 7]) and np.isnan(var[0, 7]) and n[7] == 0
        keep = np.arange(20) != 7
        assert np.isfinite(est[0, keep]).all() and np.all(n[keep] >= 1)
        if form == "table":
            assert np.array_equal(est[0, keep], good[0][0, keep]) and np.array_equal(var[0, keep], good[1][0, keep])


def test_lag_table_too_small_is_reported():
    w = world("L")
    small = w.f64(np.ones(9))
    rc, text, est, var, n = w.cv(w.data[:30], None, 0.0, "table", [w.case["vario"]], lag_mi=1, lag_mj=1, tab=C.c_void_p(small.data_ptr()))
    assert rc == E_DEVICE_DATA and "lag covariance table" in text
    assert np.isnan(est).all() and np.all(n >= 1)                                        # the search itself succeeded


# ---- refusals: nothing is launched ---------------------------------------------------------------------------------------------------
NULL = None
REFUSALS = [
    ("table", dict(grid=NULL), E_ARG, "NULL pointer"), ("table", dict(cells=NULL), E_ARG, "NULL pointer"),
    ("table", dict(x_axis=NULL), E_ARG, "NULL pointer"), ("table", dict(y_axis=NULL), E_ARG, "NULL pointer"),
    ("table", dict(tab=NULL), E_ARG, "NULL pointer"), ("table", dict(sill=NULL), E_ARG, "NULL pointer"),
    ("table", dict(est=NULL), E_ARG, "NULL pointer"), ("table", dict(var=NULL), E_ARG, "NULL pointer"),
    ("table", dict(n_neighbours=NULL), E_ARG, "NULL pointer"),
    ("local", dict(tab=NULL), E_ARG, "NULL pointer"), ("local", dict(vtype=NULL), E_ARG, "NULL pointer"),
    ("local", dict(grid=NULL), E_ARG, "NULL pointer"),
    ("table", dict(n_models=0), E_ARG, "n_models must be in [1, 8]"), ("table", dict(n_models=9), E_ARG, "n_models must be in [1, 8]"),
    ("local", dict(n_models=9), E_ARG, "n_models must be in [1, 8]"),
    ("table", dict(exclude_radius=-1.0), E_ARG, "exclude_radius must be >= 0"),
    ("table", dict(exclude_radius=float("nan")), E_ARG, "exclude_radius must be >= 0"),
    ("local", dict(exclude_radius=-0.5), E_ARG, "exclude_radius must be >= 0"),
    ("table", dict(n_cells=-1), E_ARG, "n_cells must be in [0, H * W]"), ("table", dict(n_cells=40 * 36 + 1), E_ARG, "n_cells must be in"),
    ("table", dict(num_points=7), E_UNSUPPORTED, "num_points must be in [8, 48]"),
    ("local", dict(num_points=49), E_UNSUPPORTED, "num_points must be in [8, 48]"),
    ("table", dict(hw=0), E_ARG, "search half-width"), ("table", dict(radius=0.0), E_ARG, "radius must be > 0"),
    ("table", dict(lag_mi=-1), E_ARG, "lag table extents"),
    ("local", dict(vtype=(C.c_int32 * 1)(3)), E_UNSUPPORTED, "vtype must be GSM_VTYPE_EXPONENTIAL, GSM_VTYPE_GAUSSIAN or GSM_VTYPE_SPHERICAL"),
]


@pytest.mark.parametrize("form, override, code, text", REFUSALS, ids=[f"{f}-{'-'.join(o)}-{i}" for i, (f, o, _, _) in enumerate(REFUSALS)])
def test_refusals_launch_nothing(form, override, code, text):
    w = world("L")
    name = "gsm_krige_cv" if form == "table" else "gsm_krige_cv_local"
    rc, msg, est, var, n = w.cv(w.data[:16], None, 0.0, form, w.models(form), **override)
    assert rc == code and msg.startswith(name + ": ") and text in msg, (rc, msg)
    assert np.all(est == SENTINEL) and np.all(var == SENTINEL) and np.all(n == SENTINEL_I)
    est, var, n = _ok(w.cv(w.data[:16], None, 0.0, form, w.models(form)))                # and the handle still works
    assert np.isfinite(est).all() and np.all(n >= 1)


def test_handle_refusals_and_the_empty_call():
    import torch
    from mcmc_gpu_amd.engine import GsmEngine
    w = world("L")
    p = lambda t: C.c_void_p(t.data_ptr())
    tab, sill = w.operands("table", [w.case["vario"]])
    out = torch.full((4,), SENTINEL, dtype=torch.float64, device=w.dev)
    cnt = torch.full((4,), SENTINEL_I, dtype=torch.int32, device=w.dev)
    cells = w.i32(w.data[:4])

    def call(eng, n_cells=4):
        with torch.cuda.device(w.dev):
            rc = eng.lib.gsm_krige_cv(eng.h, p(w.d_grid), p(cells), n_cells, None, 0.0, p(w.xs), p(w.ys), 1, p(tab), w.H - 1, w.W - 1, w.hw,
                                      w.radius, w.num_points, (C.c_double * 1)(*sill), p(out), p(out), p(cnt), eng._stream())
        return rc, eng.lib.gsm_last_error(eng.h).decode()

    two = GsmEngine(w.H, w.W, 2)
    try:
        rc, msg = call(two)
        assert rc == E_ARG and "gsm_krige_cv: one grid per handle" in msg
    finally:
        two.close()
    w.set_ktype("ok")
    assert call(w.eng, 0)[0] == 0                                                        # no cells: nothing to do, no error
    assert torch.all(out == SENTINEL).item() and torch.all(cnt == SENTINEL_I).item()
    with torch.cuda.device(w.dev):                                                       # simple kriging needs its mean (the setter's refusal)
        assert w.eng.lib.gsm_sgs_set_kriging(w.eng.h, 1, None) == E_ARG


# ---- interpolate.cross_validate ------------------------------------------------------------------------------------------------------
def test_cross_validate_end_to_end():
    """Data simulated with interpolate.sgs from a known exponential model, on lines.  Both orderings hold in the CPU restatement
    by margins above 0.19 of a score (tests/krige_cv_common.py: E2E_SEED; tests/test_krige_cv_host.py asserts them there)."""
    from mcmc_gpu_amd import interpolate
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        xx, yy, grid = cc.e2e_data(interpolate.sgs)
        cond = ~np.isnan(grid)
        cv = interpolate.cross_validate(xx, yy, grid, {"true": cc.E2E_TRUE, "short": cc.E2E_WRONG}, **cc.E2E_KW)
        buf = interpolate.cross_validate(xx, yy, grid, cc.E2E_TRUE, exclude_radius=cc.E2E_EX, **cc.E2E_KW)
        plan = kc.plan_of(xx, yy, grid, cc.E2E_TRUE, cc.E2E_KW)
    assert cv.names == ["true", "short"] and buf.names == ["exponential"]
    assert np.array_equal(cv.cells, np.flatnonzero(cond)) and np.array_equal(cv.z_ns, plan.grid_ns[cond])
    assert cv.est_ns.shape == cv.var_ns.shape == (2, cond.sum()) and np.all(cv.var_ns >= 0) and cv.n_neighbours.min() >= 1
    s, sb = cv.summary(), buf.summary()["exponential"]
    assert cv.best() == "true" and cv.best(by="mae") == "true" and s["true"]["rmse"] < s["short"]["rmse"]
    assert s["true"]["rmse"] < sb["rmse"]                                                # what the buffer is there to expose
    assert s["true"]["r"] > s["short"]["r"] and 0.5 < s["true"]["msdr"] < 2.0 and s["true"]["n"] == cond.sum()
    span = float(np.nanmax(grid) - np.nanmin(grid))
    np.testing.assert_allclose(cv.z, grid[cond], rtol=0, atol=1e-6 * span)               # the transformer's round trip
    assert 0 < s["true"]["rmse_data"] < span
    m = cv.maps("true")
    assert np.array_equal(~np.isnan(m["est_ns"]), cond) and np.array_equal(m["n_neighbours"] > 0, cond)
    # the public call is the C ABI's: the same numbers as a direct call on the plan's scores
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        est, var, n = interpolate._cv_run(plan, [cc.E2E_TRUE, cc.E2E_WRONG], cv.cells, None, 0.0)
    assert np.array_equal(est, cv.est_ns) and np.array_equal(var, cv.var_signed) and np.array_equal(n, cv.n_neighbours)
    # a subset, folds, parameter maps and more than eight models go through
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        folds = interpolate.block_folds(grid.shape, block=(8, 9), k=4, seed=1)
        nine = [dict(cc.E2E_TRUE, major_range=r, minor_range=r) for r in np.linspace(2000.0, 10000.0, 9)]
        many = interpolate.cross_validate(xx, yy, grid, nine, folds=folds, cells=cv.cells[::3], **cc.E2E_KW)
        one = interpolate.cross_validate(xx, yy, grid, nine[8], folds=folds, cells=cv.cells[::3], **cc.E2E_KW)
        local = interpolate.cross_validate(xx, yy, grid, [_mapped(cc.E2E_TRUE, grid.shape), _mapped(cc.MODELS[2], grid.shape)],
                                           ktype="sk", exclude_radius=cc.E2E_EX, cells=cond, radius=5000.0, num_points=16)
    assert many.est_ns.shape == (9, cv.cells[::3].size) and np.isfinite(many.est_ns).all()
    assert np.array_equal(many.est_ns[8], one.est_ns[0]) and np.array_equal(many.var_ns[8], one.var_ns[0])   # the second group
    assert local.names == ["0", "1"] and np.isfinite(local.est_ns).all() and local.best() in ("0", "1")


# ---- regression: the kernels this feature stands beside ------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["a", "c", "b_mapped"])
def test_krige_scores_keeps_the_bits_of_the_parent_commit(tag):
    """krige_scores on golden F15's cases a (ordinary, Matern) and c (simple, sim_mask) and on case b with parameter maps (the
    per-cell kernel), against the maps recorded with the parent commit's library on the same kind of device
    (tests/golden/krige_cv_parent_scores.npz)."""
    from mcmc_gpu_amd import interpolate
    xx, yy, grid, cases = ic.small()
    vario, kw, _ = cases[tag[0]]
    if tag == "b_mapped":
        vario = _mapped(vario, grid.shape)
    g = np.load(GOLD / "krige_cv_parent_scores.npz", allow_pickle=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        est_ns, var_ns, n = interpolate.krige_scores(xx, yy, grid, vario, **kc.krige_kw(kw))
    assert np.array_equal(est_ns, g[f"{tag}_est"], equal_nan=True)
    assert np.array_equal(var_ns, g[f"{tag}_var"]) and np.array_equal(n, g[f"{tag}_n"])
