"""Host suite of the posterior residual maps (mcmc_gpu_amd/posterior.py `residual`): the option checks, the library's symbols, the
summary's host arithmetic against NumPy's nan-statistics on random residual stacks, the fairness of the device suite's bounds,
save / load.  No device is used.  Definitions and bounds: tests/posterior_residual_common.py."""
import numpy as np
import pytest

import posterior_residual_common as rc
from mcmc_gpu_amd import _lib, posterior

H, W = 6, 9


def _options(residual, **kw):
    return posterior.check_options(dict(burn_in=0, thin=10, residual=residual, **kw), 100)


def test_option_checks():
    assert "residual" in posterior.POSTERIOR_KEYS
    assert _options(None)["residual"] is None and _options(False)["residual"] is None
    assert _options(True)["residual"] == dict(levels=())
    assert _options(dict())["residual"] == dict(levels=())
    assert _options(dict(levels=(1, 2.5)))["residual"] == dict(levels=(1.0, 2.5))
    assert _options(dict(levels=np.array([0.0, 1.0, 2.0, 3.0])))["residual"]["levels"] == (0.0, 1.0, 2.0, 3.0)
    assert posterior.check_residual(_options(dict(levels=[4.0]))["residual"]) == dict(levels=(4.0,))     # what comes back is accepted again
    for rhat in (True, False):                                                                          # with either form of the moments
        assert _options(True, rhat=rhat)["residual"] is not None
    assert _options(True, hist=dict(half_width=100.0), ess=dict(max_lag=3), cov=dict(probes=np.ones((1, H, W))))["residual"] is not None
    refused = [dict(levels=(1, 2, 3, 4, 5)), dict(levels=(-1.0,)), dict(levels=(1.0, np.nan)), dict(levels=(np.inf,)), dict(levels="ab"),
               dict(level=(1.0,)), 3, (1.0, 2.0)]
    for residual in refused:
        with pytest.raises(ValueError, match="residual"):
            _options(residual)
    with pytest.raises(ValueError, match="residual"):
        posterior.check_options(dict(burn_in=0, thin=10, residuals=True), 100)


def test_library_declares_and_exports_the_entry():
    names = _lib.declared_symbols()
    lib = _lib.load()
    assert "gsm_posterior_residual" in names and hasattr(lib, "gsm_posterior_residual")
    assert "posterior_residual_kernel.hip" in _lib.SOURCES
    assert lib.gsm_posterior_residual(None, None, None, None, 0, None, None) == -1          # no handle: GSM_E_ARG, nothing is touched


def _stack(seed=3, split=True):
    """A random residual stack r [C, T, H, W] with NaNs (one cell NaN throughout, one cell finite once), a hand-built summary of it
    and the pooled values [M N, H, W]."""
    rng = np.random.default_rng(seed)
    C, T = 3, 9
    r = 40.0 * rng.normal(size=(C, T, H, W)) + 25.0 * rng.normal(size=(H, W))
    r[rng.uniform(size=r.shape) < 0.1] = np.nan
    r[:, :, 0, 0] = np.nan
    r[:, :, 1, 1] = np.nan
    r[1, 4, 1, 1] = 7.5
    lo = rc.first_used(T, split)
    N = T // 2 if split else T
    M = (2 if split else 1) * C
    rg = 25.0 * rng.normal(size=(H, W))
    levels = (10.0, 60.0)
    ref = rc.reference_sums(r, rg, levels, lo)
    planes = np.stack([ref["cnt"], ref["s1"], ref["s2"], *ref["above"]]).astype(np.float64)
    mask = np.ones((H, W), dtype=bool)
    mask[:, :3] = False
    zero = np.zeros((H, W))
    s = posterior.PosteriorSummary(mean=zero, sd=zero, rhat=None, within_var=None, between_var_over_n=None, n_chains=C, n_sequences=M,
                                   n_per_sequence=N, snapshot_iterations=np.arange(T) * 10, burn_in=0, thin=10, split=split,
                                   residual_sums=planes, residual_ref=rg, residual_levels=np.asarray(levels), residual_sigma_mc=5.0,
                                   residual_mc_mask=mask)
    return s, r[:, lo:].reshape((M * N, H, W)), ref, mask, levels


@pytest.mark.parametrize("split", [True, False])
def test_summary_formulas_against_numpy(split):
    s, pooled, ref, mask, levels = _stack(split=split)
    n = pooled.shape[0]
    assert n == s.n_sequences * s.n_per_sequence
    fin = np.isfinite(pooled)
    cnt = fin.sum(axis=0)
    assert np.array_equal(s.residual_count(), cnt) and s.residual_count().dtype == np.int64 and cnt[0, 0] == 0 and cnt[1, 1] == 1
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                                     # nanmean / nanstd of an all-NaN cell
        mean, sd = np.nanmean(pooled, axis=0), np.nanstd(pooled, axis=0, ddof=1)
        rms = np.sqrt(np.nanmean(pooled * pooled, axis=0))
    sd[cnt < 2] = np.nan
    scale = np.nanmax(np.abs(pooled))
    for name, got, exp in (("mean", s.residual_mean(), mean), ("sd", s.residual_sd(), sd), ("rms", s.residual_rms(), rms)):
        assert np.array_equal(np.isnan(got), np.isnan(exp)), name
        ok = ~np.isnan(exp)
        assert (np.abs(got[ok] - exp[ok]) <= 1e-12 * scale).all(), (name, np.abs(got[ok] - exp[ok]).max())
    assert np.isnan(s.residual_mean()[0, 0]) and np.isnan(s.residual_sd()[1, 1]) and abs(s.residual_mean()[1, 1] - 7.5) <= 1e-13
    for lv in levels:
        exp = np.where(cnt > 0, (fin & (np.abs(np.where(fin, pooled, 0.0)) > lv)).sum(axis=0) / np.maximum(cnt, 1), np.nan)
        assert np.array_equal(s.prob_residual_above(lv), exp, equal_nan=True)
    with pytest.raises(KeyError):
        s.prob_residual_above(11.0)
    # the loss as the reference computes it, state by state, and its mean
    per_state = np.array([np.nansum(np.square(p[mask])) / (2 * 5.0 ** 2) for p in pooled])
    assert abs(s.expected_loss() - per_state.mean()) <= 1e-12 * per_state.mean()
    dens = s.loss_density()
    assert np.isnan(dens[0, 0]) and (dens[:, :3][cnt[:, :3] > 0] == 0).all() and abs(np.nansum(dens) - s.expected_loss()) <= 1e-12 * s.expected_loss()
    rc.check_summary(s, ref, f"hand-built split={split}")
    bare = posterior.PosteriorSummary(mean=s.mean, sd=s.sd, rhat=None, within_var=None, between_var_over_n=None, n_chains=3, n_sequences=6,
                                      n_per_sequence=4, snapshot_iterations=s.snapshot_iterations, burn_in=0, thin=10, split=True)
    for method in (bare.residual_mean, bare.residual_sd, bare.residual_rms, bare.residual_count, bare.loss_density, bare.expected_loss):
        with pytest.raises(ValueError, match="residual"):
            method()
    with pytest.raises(ValueError, match="residual"):
        bare.prob_residual_above(10.0)


def test_residual_field_is_the_gradient_form():
    f = rc.fields(7, 11, seed=2)
    x, g = rc.beds(1, 2, 7, 11, 5, f32=False, nan_bed=False)
    got = posterior.residual_field(x[0, 0], f["surf"], f["velx"], f["vely"], f["dhdt"], f["smb"], f["resolution"])
    assert np.array_equal(got, rc.residual_numpy(x[0, 0], f))
    # one-sided at the borders, centred inside, by hand at three cells
    q = f["velx"] * (f["surf"] - x[0, 0])
    p = f["vely"] * (f["surf"] - x[0, 0])
    h = f["resolution"]
    by_hand = {(0, 0): (q[0, 1] - q[0, 0]) / h + (p[1, 0] - p[0, 0]) / h, (3, 4): (q[3, 5] - q[3, 3]) / (2 * h) + (p[4, 4] - p[2, 4]) / (2 * h),
               (6, 10): (q[6, 10] - q[6, 9]) / h + (p[6, 10] - p[5, 10]) / h}
    for (i, j), v in by_hand.items():
        assert abs(got[i, j] - (v + f["dhdt"][i, j] - f["smb"][i, j])) <= 1e-12 * abs(v)


@pytest.mark.parametrize("H_,W_,C,T,split", rc.CASES)
def test_bounds_are_fair(H_, W_, C, T, split):
    """The device suite's cases in plain float64 NumPy, summed in another order than the reference's (snapshot by snapshot, chains from
    the last to the first): the error uses at most half of each bound."""
    x, g, f = rc.case_data(H_, W_, C, T)
    lo = rc.first_used(T, split)
    r = rc.residual_numpy(x, f)
    rg = rc.shift(g, f)
    ref = rc.reference_sums(r, rg, rc.LEVELS, lo)
    s1, s2 = np.zeros((H_, W_)), np.zeros((H_, W_))
    with np.errstate(invalid="ignore"):
        for t in range(lo, T):
            for c in reversed(range(C)):
                d = np.where(np.isfinite(r[c, t]), r[c, t] - rg, 0.0)
                s1 = s1 + d
                s2 = s2 + d * d
    planes = np.stack([ref["cnt"].astype(np.float64), s1, s2, *ref["above"].astype(np.float64)])
    shares = rc.check_sums(planes, ref, f"float64 NumPy {H_}x{W_} C={C} T={T} split={split}")
    print(f"shares of the bounds used by a plain float64 accumulation: S1 {shares[0]:.3f}, S2 {shares[1]:.3f}")
    assert max(shares) <= 0.5, shares
    assert ref["cnt"].max() == C * (T - lo)


def test_split_plan_of_the_device_cases():
    """The regimes the device cases are there for, on a device of 256 compute units."""
    assert rc.split_plan(37, 41, 5, False, 256) == dict(vec=1, lx=32, ly=8, tiles_x=2, tiles_y=5, parts=1, cpp=5, last=5, empty=0)
    for f32, vec, lx in ((False, 2, 32), (True, 4, 16)):
        p = rc.split_plan(64, 64, 6, f32, 256)
        assert (p["vec"], p["lx"], p["tiles_x"]) == (vec, lx, 1) and p["vec"] * (4 if f32 else 8) == 16
    assert rc.split_plan(3, 130, 3, False, 256)["tiles_x"] == 3 and rc.split_plan(70, 3, 3, False, 256)["ly"] == 64
    p = rc.split_plan(16, 24, 130, False, 256)
    assert (p["parts"], p["cpp"], p["last"], p["empty"]) == (16, 9, 4, 1)
    p = rc.split_plan(16, 24, 390, True, 256)
    assert (p["parts"], p["cpp"], p["last"], p["empty"]) == (48, 9, 3, 4)
    p = rc.split_plan(256, 256, 1024, False, 256)                                            # the headline shape: 8 rows x 64 columns, 8 parts
    assert (p["lx"], p["ly"], p["tiles_x"] * p["tiles_y"], p["parts"], p["cpp"]) == (32, 8, 128, 8, 128)


def test_save_load_round_trip(tmp_path):
    s, _, _, _, levels = _stack()
    s.save(tmp_path / "with.npz")
    got = posterior.PosteriorSummary.load(tmp_path / "with.npz")
    for name in ("residual_sums", "residual_ref", "residual_levels", "residual_mc_mask"):
        assert np.array_equal(getattr(got, name), getattr(s, name)), name
    assert got.residual_sigma_mc == 5.0 and isinstance(got.residual_sigma_mc, float)
    for name in ("residual_mean", "residual_sd", "residual_rms", "residual_count", "loss_density"):
        assert np.array_equal(getattr(got, name)(), getattr(s, name)(), equal_nan=True), name
    assert got.expected_loss() == s.expected_loss()
    assert np.array_equal(got.prob_residual_above(levels[1]), s.prob_residual_above(levels[1]), equal_nan=True)
    # a file written without the fields, as every file before them was
    old = {k: np.asarray(v) for k, v in dict(mean=s.mean, sd=s.sd, n_chains=3, n_sequences=6, n_per_sequence=4,
                                             snapshot_iterations=s.snapshot_iterations, burn_in=0, thin=10, split=True).items()}
    np.savez_compressed(tmp_path / "old.npz", **old)
    got = posterior.PosteriorSummary.load(tmp_path / "old.npz")
    assert all(getattr(got, name) is None for name in ("residual_sums", "residual_ref", "residual_levels", "residual_sigma_mc", "residual_mc_mask"))
    with pytest.raises(ValueError, match="residual"):
        got.residual_mean()
