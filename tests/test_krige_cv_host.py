"""Host: what interpolate.cross_validate rests on without a device -- the fold builders, CrossValidation's statistics against
direct NumPy, the hold-out emulation of tests/krige_cv_common.py against a brute-force loop, the no-tie rule of its exclusion
radii, the orderings the end-to-end GPU test asserts (in the CPU restatement), and the library's two new entry points."""
import subprocess
import warnings

import numpy as np
import pytest

import krige_common as kc
import krige_cv_common as cc


# ---- fold builders --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, block, k", [((40, 36), (8, 6), 4), ((37, 41), (5, 7), 5), ((12, 12), (12, 3), 2)])
def test_block_folds_label_every_cell_once_in_contiguous_blocks(shape, block, k):
    from mcmc_gpu_amd import interpolate
    f = interpolate.block_folds(shape, block=block, k=k, seed=7)
    assert f.dtype == np.int32 and f.shape == shape and f.min() == 0 and f.max() == k - 1
    assert np.array_equal(f, interpolate.block_folds(shape, block=block, k=k, seed=7))      # deterministic per seed
    assert not np.array_equal(f, interpolate.block_folds(shape, block=block, k=k, seed=8))
    bh, bw = block
    n_blocks = 0
    for i0 in range(0, shape[0], bh):                                                   # a block is one label, all of it
        for j0 in range(0, shape[1], bw):
            assert np.unique(f[i0:i0 + bh, j0:j0 + bw]).size == 1
            n_blocks += 1
    per_fold = np.bincount([f[i0, j0] for i0 in range(0, shape[0], bh) for j0 in range(0, shape[1], bw)], minlength=k)
    assert per_fold.sum() == n_blocks and per_fold.max() - per_fold.min() <= 1
    mask = np.random.default_rng(0).random(shape) < 0.3
    g = interpolate.block_folds(shape, block=block, k=k, seed=7, mask=mask)
    assert np.array_equal(g[mask], f[mask]) and np.all(g[~mask] == -1)


def test_random_folds_label_every_data_cell_once():
    from mcmc_gpu_amd import interpolate
    mask = ~np.isnan(cc.lines_grid()[2])
    for k in (2, 5):
        f = interpolate.random_folds(mask, k=k, seed=3)
        assert f.dtype == np.int32 and f.shape == mask.shape
        assert np.all(f[~mask] == -1) and np.all((f[mask] >= 0) & (f[mask] < k))
        sizes = np.bincount(f[mask], minlength=k)
        assert sizes.sum() == mask.sum() and sizes.max() - sizes.min() <= 1
        assert np.array_equal(f, interpolate.random_folds(mask, k=k, seed=3))
        assert not np.array_equal(f, interpolate.random_folds(mask, k=k, seed=4))


def test_fold_builders_refuse_bad_arguments():
    from mcmc_gpu_amd import interpolate
    with pytest.raises(ValueError, match="k must be"):
        interpolate.block_folds((8, 8), block=(8, 8), k=2)                               # one block
    with pytest.raises(ValueError, match="positive"):
        interpolate.block_folds((8, 8), block=(0, 8), k=2)
    with pytest.raises(ValueError, match="mask"):
        interpolate.block_folds((8, 8), block=(2, 2), k=2, mask=np.ones((4, 4), bool))
    with pytest.raises(ValueError, match="bool"):
        interpolate.random_folds(np.ones((4, 4)), k=2)
    with pytest.raises(ValueError, match="k must be"):
        interpolate.random_folds(np.eye(4, dtype=bool), k=5)


# ---- CrossValidation --------------------------------------------------------------------------------------------------------------
class _FakePlan:
    """What CrossValidation takes from a _Plan: the shape, the grid in scores, and a transformer (data = 10 * score - 400)."""

    class _Nst:
        @staticmethod
        def inverse_transform(a):
            return 10.0 * a - 400.0

    def __init__(self, grid_ns):
        self.H, self.W = grid_ns.shape
        self.grid_ns = grid_ns
        self.nst = self._Nst()


def _synthetic():
    from mcmc_gpu_amd import interpolate
    r = np.random.default_rng(5)
    H, W, n = 9, 11, 40
    cells = np.sort(r.choice(H * W, n, replace=False)).astype(np.int32)
    grid_ns = np.full((H, W), np.nan)
    z = r.standard_normal(n)
    grid_ns.ravel()[cells] = z
    est = np.stack([z + 0.3 * r.standard_normal(n), z + 0.8 * r.standard_normal(n) + 0.1])
    var = np.stack([np.full(n, 0.09), r.uniform(0.2, 1.0, n)])
    var[0, 3] = 0.0                                                                      # no spread: out of the standardized figures
    var[1, 5] = -1e-12                                                                   # clipped to 0
    est[1, 7] = var[1, 7] = np.nan                                                       # a singular system
    cv = interpolate.CrossValidation(_FakePlan(grid_ns), cells, ["good", "poor"], est, var, np.full(n, 12, dtype=np.int32))
    return cv, cells, z, est, var, (H, W)


def test_cross_validation_summary_equals_numpy():
    cv, cells, z, est, var, shape = _synthetic()
    assert np.array_equal(cv.z_ns, z) and np.array_equal(cv.var_signed, var, equal_nan=True)
    assert cv.var_ns[1, 5] == 0.0 and np.isnan(cv.var_ns[1, 7]) and np.all(cv.var_ns[np.isfinite(var)] >= 0)
    np.testing.assert_array_equal(cv.z, 10.0 * z - 400.0)
    np.testing.assert_array_equal(cv.error(), est - z)
    np.testing.assert_allclose(cv.error(data_units=True), 10.0 * (est - z), rtol=1e-12, atol=1e-10)
    s = cv.standardized()
    assert np.isnan(s[0, 3]) and np.isnan(s[1, 5]) and np.isnan(s[1, 7])
    summ = cv.summary()
    assert list(summ) == ["good", "poor"]
    for m, name in enumerate(("good", "poor")):
        ok = ~np.isnan(est[m])
        e = (est[m] - z)[ok]
        sd_ok = ok & (np.where(var[m] < 0, 0, var[m]) > 0)
        st = (est[m] - z)[sd_ok] / np.sqrt(var[m][sd_ok])
        exp = dict(n=int(ok.sum()), mean_error=e.mean(), mae=np.abs(e).mean(), rmse=np.sqrt((e ** 2).mean()),
                   rmse_data=10.0 * np.sqrt((e ** 2).mean()), mean_standardized=st.mean(), msdr=(st ** 2).mean(),
                   coverage95=(np.abs(st) <= 1.96).mean(), r=np.corrcoef(est[m][ok], z[ok])[0, 1])
        assert set(summ[name]) == set(exp)
        for key, v in exp.items():
            np.testing.assert_allclose(summ[name][key], v, rtol=1e-12, atol=1e-12, err_msg=f"{name} {key}")
    assert summ["good"]["n"] == 40 and summ["poor"]["n"] == 39
    assert cv.best() == "good" and cv.best(by="mae") == "good" and cv.best(by="r") == "good"
    assert cv.best(by="msdr") == min(("good", "poor"), key=lambda k: abs(summ[k]["msdr"] - 1.0))
    with pytest.raises(ValueError, match="by must be"):
        cv.best(by="luck")


def test_cross_validation_maps_scatter_to_the_grid():
    cv, cells, z, est, var, shape = _synthetic()
    for m in (1, "poor"):
        maps = cv.maps(m)
        assert set(maps) == {"est_ns", "var_ns", "error", "standardized", "n_neighbours"}
        off = np.ones(shape, bool)
        off.ravel()[cells] = False
        for key in ("est_ns", "var_ns", "error", "standardized"):
            assert maps[key].shape == shape and np.isnan(maps[key][off]).all()
        assert np.array_equal(maps["est_ns"].ravel()[cells], est[1], equal_nan=True)
        assert np.array_equal(maps["error"].ravel()[cells], est[1] - z, equal_nan=True)
        assert maps["n_neighbours"].dtype == np.int32 and maps["n_neighbours"].sum() == 12 * cells.size
        assert np.all(maps["n_neighbours"][off] == 0)


def test_cross_validation_of_nothing_is_empty_not_an_error():
    from mcmc_gpu_amd import interpolate
    cv = interpolate.CrossValidation(_FakePlan(np.full((4, 4), np.nan)), np.zeros(0, np.int32), ["a"], np.zeros((1, 0)), np.zeros((1, 0)),
                                     np.zeros(0, np.int32))
    row = cv.summary()["a"]
    assert row["n"] == 0 and all(np.isnan(v) for k, v in row.items() if k != "n")
    with pytest.raises(ValueError, match="no model"):
        cv.best()


def test_model_lists_and_argument_errors_before_any_device_work():
    from mcmc_gpu_amd import interpolate
    a, b = cc.MODELS[0], cc.MODELS[2]
    assert interpolate._cv_models(a) == (["exponential"], [a])
    assert interpolate._cv_models({"e": a, "s": b}) == (["e", "s"], [a, b])
    assert interpolate._cv_models([a, b]) == (["0", "1"], [a, b])
    for bad in (None, [], {}, [a, 3]):
        with pytest.raises(ValueError, match="variogram"):
            interpolate._cv_models(bad)
    xx, yy, grid = cc.lines_grid()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mapped = dict(a, major_range=np.full(grid.shape, 6000.0))
        with pytest.raises(ValueError, match="all have scalar parameters or all"):
            interpolate.cross_validate(xx, yy, grid, [a, mapped], **cc.E2E_KW)
        with pytest.raises(NotImplementedError, match="Bessel"):
            interpolate.cross_validate(xx, yy, grid, [mapped, dict(cc.MODELS[3], major_range=np.full(grid.shape, 6000.0))], **cc.E2E_KW)
        for ex in (-1.0, float("nan"), "far"):
            with pytest.raises(ValueError, match="exclude_radius"):
                interpolate.cross_validate(xx, yy, grid, a, exclude_radius=ex, **cc.E2E_KW)
        with pytest.raises(ValueError, match="folds"):
            interpolate.cross_validate(xx, yy, grid, a, folds=np.zeros((3, 3), int), **cc.E2E_KW)
        with pytest.raises(ValueError, match="folds"):
            interpolate.cross_validate(xx, yy, grid, a, folds=np.zeros(grid.shape), **cc.E2E_KW)
        with pytest.raises(ValueError, match="without a value"):
            interpolate.cross_validate(xx, yy, grid, a, cells=np.flatnonzero(np.isnan(grid))[:3], **cc.E2E_KW)
        with pytest.raises(ValueError, match="outside the grid"):
            interpolate.cross_validate(xx, yy, grid, a, cells=np.array([grid.size]), **cc.E2E_KW)
        with pytest.raises(ValueError, match="cells"):
            interpolate.cross_validate(xx, yy, grid, a, cells=np.ones((2, 2), bool), **cc.E2E_KW)
        with pytest.raises(NotImplementedError, match="num_points"):
            interpolate.cross_validate(xx, yy, grid, a, radius=5000.0, num_points=64)
        with pytest.raises(ValueError, match="ktype"):
            interpolate.cross_validate(xx, yy, grid, a, radius=5000.0, ktype="uk")
        plan = kc.plan_of(xx, yy, grid, a, cc.E2E_KW)
    every = np.flatnonzero(plan.cond)
    assert np.array_equal(interpolate._cv_cells(plan, None), every) and interpolate._cv_cells(plan, None).dtype == np.int32
    assert np.array_equal(interpolate._cv_cells(plan, plan.cond), every)
    assert np.array_equal(interpolate._cv_cells(plan, every[[5, 2, 9]]), every[[5, 2, 9]])    # listed cells: as given


# ---- the tests' own hold-out emulation ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["L", "G3", "G2"])
def test_hold_out_emulation_equals_brute_force(cid):
    from mcmc_gpu_amd import interpolate
    c = cc.cases()[cid]
    xs, ys = c["xx"][0, :], c["yy"][:, 0]
    cond = ~np.isnan(c["grid"])
    H, W = cond.shape
    fold = interpolate.random_folds(cond, k=5, seed=1)
    fold.ravel()[np.flatnonzero(cond)[::9]] = -1                                         # some data in no fold
    targets = cc.pick_targets(cond)
    assert 30 <= targets.size <= 48 and cond.ravel()[targets].all() and np.all(np.diff(targets) > 0)
    for t in targets[::3]:
        for f, ex in ((None, 0.0), (None, c["ex"]), (fold, 0.0), (fold, c["ex"])):
            got = cc.excluded(xs, ys, cond, t, f, ex)
            i0, j0 = divmod(int(t), W)
            exp = np.zeros((H, W), bool)
            for i in range(H):
                for j in range(W):
                    same_fold = f is not None and f[i0, j0] >= 0 and f[i, j] == f[i0, j0]
                    near = ex > 0 and np.sqrt((xs[j0] - xs[j]) ** 2 + (ys[i0] - ys[i]) ** 2) <= ex
                    exp[i, j] = (i == i0 and j == j0) or same_fold or near
            assert np.array_equal(got, exp)
    g = cc.held_out(np.where(cond, 1.0, np.nan), xs, ys, targets[0], fold, c["ex"])
    assert np.array_equal(np.isnan(g), ~cond | cc.excluded(xs, ys, cond, targets[0], fold, c["ex"]))


def test_exclusion_radii_are_no_lattice_distance():
    for cid, c in cc.cases().items():
        xs, ys = c["xx"][0, :], c["yy"][:, 0]
        assert cc.no_tie(xs, ys, c["ex"]), cid
        assert not cc.no_tie(xs, ys, float(np.hypot(3 * (xs[1] - xs[0]), 4 * (ys[1] - ys[0])))), cid   # the check can fail
    xs, ys = cc.cases()["G3"]["xx"][0, :], cc.cases()["G3"]["yy"][:, 0]
    assert not cc.no_tie(xs, ys, 1250.0)                                                 # 5 rows of 250 m: why G3 takes 1300
    xx, yy, _ = cc.lines_grid()
    assert cc.no_tie(xx[0, :], yy[:, 0], cc.E2E_EX)


def test_buffer_changes_most_neighbour_sets_on_the_lines_grid():
    """What the lines grid is there for: under a 2.5-cell buffer most targets lose neighbours the plain hold-out takes."""
    c = cc.cases()["L"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plan = kc.plan_of(c["xx"], c["yy"], c["grid"], c["vario"], c["kw"])
    xs, ys = c["xx"][0, :], c["yy"][:, 0]
    t = np.flatnonzero(plan.cond)
    near = [(cc.excluded(xs, ys, plan.cond, k, None, c["ex"]) & plan.cond).sum() - 1 for k in t]
    assert np.mean(np.array(near) >= 2) > 0.8


def test_end_to_end_orderings_hold_in_the_cpu_restatement():
    """The two orderings tests/test_gpu_krige_cv.py asserts on the device, for its seed: the true range beats the tenfold short
    one, and plain leave-one-out looks better than the 2.5-cell buffered hold-out on line data."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        xx, yy, grid = cc.e2e_data(cc.cpu_sgs)
        plan = kc.plan_of(xx, yy, grid, cc.E2E_TRUE, cc.E2E_KW)
    t = np.flatnonzero(plan.cond)
    z = plan.grid_ns.ravel()[t]
    rmse = {}
    for name, v, ex in (("true", cc.E2E_TRUE, 0.0), ("wrong", cc.E2E_WRONG, 0.0), ("buffered", cc.E2E_TRUE, cc.E2E_EX)):
        _, est, _ = cc.cv_cpu(xx, yy, plan.grid_ns, v, cc.E2E_KW, t, ex=ex)
        rmse[name] = float(np.sqrt(np.mean((est - z) ** 2)))
    assert rmse["true"] + 0.1 < rmse["wrong"] and rmse["true"] + 0.1 < rmse["buffered"], rmse


# ---- the library ----------------------------------------------------------------------------------------------------------------------
def test_library_declares_and_exports_the_cross_validation_entries():
    import mcmc_gpu_amd
    from mcmc_gpu_amd import _lib, interpolate
    assert "krige_cv_kernel.hip" in _lib.SOURCES and (_lib.CSRC / "krige_cv_kernel.hip").exists()
    assert {"gsm_krige_cv", "gsm_krige_cv_local"} <= set(_lib.declared_symbols())
    lib = _lib.load()
    assert hasattr(lib, "gsm_krige_cv") and len(lib.gsm_krige_cv.argtypes) == 20
    assert hasattr(lib, "gsm_krige_cv_local") and len(lib.gsm_krige_cv_local.argtypes) == 18
    assert len(lib.gsm_krige_grid.argtypes) == 17 and len(lib.gsm_krige_grid_local.argtypes) == 15    # the twins they extend
    out = subprocess.run(["strings", "-n", "6", str(_lib.LIB_PATH)], capture_output=True, text=True).stdout
    assert "krige_cv_kernel" in out and "krige_cv_local_kernel" in out                     # the kernels are in the gfx950 code object
    # no handle: GSM_E_ARG, nothing is touched
    assert lib.gsm_krige_cv(None, None, None, 0, None, 0.0, None, None, 1, None, 0, 0, 1, 1.0, 8, None, None, None, None, None) == -1
    assert lib.gsm_krige_cv_local(None, None, None, 0, None, 0.0, None, None, 1, None, None, 1, 1.0, 8, None, None, None, None) == -1
    names = {"cross_validate", "CrossValidation", "block_folds", "random_folds"}
    assert names <= set(interpolate.__all__) and names <= set(mcmc_gpu_amd.__all__)
    assert mcmc_gpu_amd.cross_validate is interpolate.cross_validate
