"""Host suite of the posterior covariance of every cell with its neighbours (mcmc_gpu_amd/posterior.py `local`): the option checks,
the offset table, the library's symbol, the summary's host arithmetic against NumPy on the stack itself, the refusals of the
methods, save / load, and the fairness of the device bound on the device tests' own cases.  No device is used.  Definitions:
tests/posterior_local_common.py."""
import numpy as np
import pytest

import posterior_local_common as lc
from mcmc_gpu_amd import _lib, posterior

H, W = 9, 11


def _options(local, **kw):
    return posterior.check_options(dict(burn_in=0, thin=10, local=local, **kw), 100)


def test_option_checks():
    assert "local" in posterior.POSTERIOR_KEYS
    assert _options(None)["local"] is None and _options(False)["local"] is None
    assert _options(True)["local"] == dict(reach=1) and _options({})["local"] == dict(reach=1)
    for R in (1, 2, 3, 4, np.int64(3)):
        assert _options(dict(reach=R))["local"] == dict(reach=int(R))
    for rhat in (True, False):                                                           # works with either form of the moments
        assert _options(dict(reach=2), rhat=rhat)["local"] == dict(reach=2)
    assert _options(dict(reach=2), hist=dict(half_width=50.0), ess=dict(max_lag=3), residual=True, cov=dict(probes=np.ones((1, 3, 3))))["local"] == dict(reach=2)
    assert posterior.check_local(_options(dict(reach=4))["local"]) == dict(reach=4)     # what check_options returns is accepted again
    for local in (dict(reach=0), dict(reach=5), dict(reach=-1), dict(reach=2.0), dict(reach="2"), dict(reach=True), dict(reach=None),
                  dict(radius=2), dict(reach=2, lags=1), 2, "yes", [2]):
        with pytest.raises(ValueError, match="local"):
            _options(local)
    with pytest.raises(ValueError, match="local"):
        posterior.check_options(dict(burn_in=0, thin=10, locals=True), 100)


@pytest.mark.parametrize("R", [1, 2, 3, 4])
def test_offset_table(R):
    t = posterior.local_offsets(R)
    K = 2 * R * R + 2 * R
    assert t.shape == (K, 2) and t.dtype == np.int64 and K == (4, 12, 24, 40)[R - 1]
    assert [tuple(o) for o in t.tolist()] == lc.offsets(R)
    assert t[:R].tolist() == [[0, dj] for dj in range(1, R + 1)]
    assert t[R:].tolist() == [[di, dj] for di in range(1, R + 1) for dj in range(-R, R + 1)]
    # the upper half plane: with the opposite offsets and (0, 0), every offset of the (2 R + 1)^2 window exactly once
    window = {tuple(o) for o in t.tolist()} | {(-di, -dj) for di, dj in t.tolist()} | {(0, 0)}
    assert len(window) == 2 * K + 1 == (2 * R + 1) ** 2
    for bad in (0, 5, 2.0, True, None):
        with pytest.raises(ValueError, match="reach"):
            posterior.local_offsets(bad)


def test_library_declares_and_exports_the_entry():
    names = _lib.declared_symbols()
    lib = _lib.load()
    assert "gsm_posterior_local" in names and hasattr(lib, "gsm_posterior_local")
    assert "posterior_local_kernel.hip" in _lib.SOURCES
    assert lib.gsm_posterior_local(None, None, None, 2, None, None) == -1                # no handle: GSM_E_ARG, nothing is touched


def _ensemble(R=3):
    """3 chains x 17 snapshots x 9 x 11 cells, split: 6 sequences of 8 snapshots, the first snapshot dropped; neighbours co-vary (a
    smooth part per state), cell (4, 6) never changes.  Returns the hand-built summary and the pooled values [48, H, W]."""
    rng = np.random.default_rng(23)
    C, T = 3, 17
    smooth = rng.normal(size=(C, T, H + 2, W + 2))
    smooth = smooth[:, :, 1:-1, 1:-1] + smooth[:, :, :-2, 1:-1] + smooth[:, :, 2:, 1:-1] + smooth[:, :, 1:-1, :-2] + smooth[:, :, 1:-1, 2:]
    x = -300.0 + 40.0 * rng.normal(size=(C, T, H, W)) + 60.0 * smooth + 30.0 * rng.normal(size=(C, T, 1, 1))
    x[:, :, 4, 6] = -250.0
    N, lo = T // 2, 1
    M = 2 * C
    pooled = x[:, lo:].reshape(M * N, H, W)
    mean, sd = pooled.mean(axis=0), pooled.std(axis=0, ddof=1)
    sd[4, 6] = 0.0
    g = mean + 0.5 * sd * rng.uniform(-1, 1, size=(H, W))                                       # within one sd of the mean
    X, _ = lc.reference(pooled, g, R)
    s = posterior.PosteriorSummary(mean=mean, sd=sd, rhat=None, within_var=None, between_var_over_n=None, n_chains=C, n_sequences=M,
                                   n_per_sequence=N, snapshot_iterations=np.arange(T) * 10, burn_in=0, thin=10, split=True,
                                   local_cross=X.astype(np.float64), local_reach=R, local_centre=g)
    return s, pooled


def _shift(a, di, dj):
    """a[..., i + di, j + dj] at [..., i, j], NaN where that is outside the grid."""
    out = np.full(a.shape, np.nan)
    sl = lc.pair_slices(a.shape[-2], a.shape[-1], di, dj)
    if sl is not None:
        out[(Ellipsis,) + sl[0]] = a[(Ellipsis,) + sl[1]]
    return out


# The conditioning of the summary's formulas.  local_covariance forms (X - n m m') / (n - 1) from X about g, with |m|, |m'| <= 0.5 sd:
# X is of the size n sd sd' (1.25 at most, by Cauchy-Schwarz plus the shift), each of its few operations rounds at 2^-53 relative to
# that, and m = mean - g carries the rounding of a subtraction of two numbers of the bed's magnitude (300 against sd of 80: a factor
# 4 on 2^-53).  1e-12 sqrt(var var') holds all of it with two orders to spare, as tests/test_posterior_cov_host.py argues for the
# same expression.  A variance formed from such covariances (difference, gradient, block mean) is a sum of at most k^4 of them, each
# within 1e-12 of the product of two sds of the window: the sd, its square root, is compared at 1e-12 sd_max^2 / (its own value).
COV_TOL = 1e-12


def test_local_covariance_against_numpy():
    R = 3
    s, pooled = _ensemble(R)
    n = pooled.shape[0]
    cov = s.local_covariance()
    assert cov.shape == (24, H, W)
    ins = lc.inside(H, W, R)
    assert np.array_equal(np.isnan(cov), ~ins)                                            # NaN exactly where the partner is outside
    dev = pooled - pooled.mean(axis=0)
    worst = 0.0
    for k, (di, dj) in enumerate(lc.offsets(R)):
        exp = (dev * _shift(dev, di, dj)).sum(axis=0) / (n - 1)
        i, j = 2, 5                                                                       # and np.cov itself at one pair per offset
        assert abs(exp[i, j] - np.cov(pooled[:, i, j], pooled[:, i + di, j + dj])[0, 1]) <= 1e-13 * s.sd[i, j] * s.sd[i + di, j + dj]
        tol = COV_TOL * s.sd * _shift(s.sd, di, dj)
        ok = ins[k] & (tol > 0)
        err = np.abs(cov[k] - exp)
        worst = max(worst, float((err[ok] / tol[ok]).max()))
        assert (err[ins[k]] <= tol[ins[k]]).all(), (k, di, dj)
    print(f"local_covariance against the stack: largest error {worst:.3e} of 1e-12 sd sd'")
    # the same expression at offset (0, 0) is sd^2
    m = s.mean - s.local_centre
    X0 = ((pooled - s.local_centre) ** 2).sum(axis=0)
    assert (np.abs((X0 - n * m * m) / (n - 1) - s.sd ** 2) <= COV_TOL * s.sd ** 2).all()
    rho = s.local_correlation()
    live = s.sd > 0
    for k, (di, dj) in enumerate(lc.offsets(R)):
        both = ins[k] & live & (_shift(s.sd, di, dj) > 0)
        assert np.array_equal(np.isnan(rho[k]), ~both)                                    # NaN where either sd is 0 (and outside)
        assert (np.abs(rho[k][both]) <= 1 + 1e-12).all()
    assert np.median(rho[0][~np.isnan(rho[0])]) > 0.2                                     # the smooth part: neighbours go together


def test_difference_gradient_and_block_mean_against_numpy():
    R = 3
    s, pooled = _ensemble(R)
    sd_max2 = float(s.sd.max()) ** 2

    def close(got, exp, label):
        assert got.shape == exp.shape, (label, got.shape, exp.shape)
        assert np.array_equal(np.isnan(got), np.isnan(exp)), label
        ok = ~np.isnan(exp)
        # |sqrt(a) - sqrt(b)| = |a - b| / (sqrt(a) + sqrt(b)); a variance of 0 (the constant cell against itself) is met exactly
        tol = np.where(exp[ok] > 0, 16 * COV_TOL * sd_max2 / np.maximum(exp[ok], 1e-300), 1e-5 * np.sqrt(sd_max2))
        err = np.abs(got[ok] - exp[ok])
        print(f"{label}: largest error {float((err / tol).max()):.3e} of the tolerance")
        assert (err <= tol).all(), label

    for di in range(-R, R + 1):
        for dj in range(-R, R + 1):
            exp = (_shift(pooled, di, dj) - pooled).std(axis=0, ddof=1)
            close(s.difference_sd(di, dj), exp, f"difference_sd({di}, {dj})")
    assert (s.difference_sd(0, 0) == 0).all()
    h = 500.0
    g0, g1 = s.gradient_sd(h)
    grads = np.stack([np.stack(np.gradient(b, h)) for b in pooled])                      # [n, 2, H, W]: what np.gradient takes
    e0, e1 = grads[:, 0].std(axis=0, ddof=1), grads[:, 1].std(axis=0, ddof=1)
    e0[[0, -1], :] = np.nan                                                               # one-sided there: not covered
    e1[:, [0, -1]] = np.nan
    close(g0 * h, e0 * h, "gradient_sd axis 0")
    close(g1 * h, e1 * h, "gradient_sd axis 1")
    for k in (1, 2, 3, 4):
        means = np.stack([pooled[:, a:a + H - k + 1, b:b + W - k + 1] for a in range(k) for b in range(k)]).mean(axis=0)
        exp = means.std(axis=0, ddof=1)
        got = s.block_mean_sd(k)
        assert got.shape == (H - k + 1, W - k + 1)
        close(got, exp, f"block_mean_sd({k})")


def test_refusals_of_the_methods():
    s, _ = _ensemble(1)
    bare = posterior.PosteriorSummary(mean=s.mean, sd=s.sd, rhat=None, within_var=None, between_var_over_n=None, n_chains=3, n_sequences=6,
                                      n_per_sequence=8, snapshot_iterations=s.snapshot_iterations, burn_in=0, thin=10, split=True)
    for call in (bare.local_covariance, bare.local_correlation, lambda: bare.difference_sd(0, 1), lambda: bare.gradient_sd(500.0),
                 lambda: bare.block_mean_sd(2)):
        with pytest.raises(ValueError, match="local"):
            call()
    s.difference_sd(1, -1), s.difference_sd(-1, 0), s.block_mean_sd(2), s.block_mean_sd(1)  # within reach 1
    for call in (lambda: s.difference_sd(0, 2), lambda: s.difference_sd(-2, 1), lambda: s.gradient_sd(500.0), lambda: s.block_mean_sd(3)):
        with pytest.raises(ValueError, match="reach"):
            call()
    s2, _ = _ensemble(2)
    s2.gradient_sd(500.0), s2.block_mean_sd(3)
    for call in (lambda: s2.block_mean_sd(4), lambda: s2.difference_sd(3, 0)):
        with pytest.raises(ValueError, match="reach"):
            call()
    for call in (lambda: s2.block_mean_sd(0), lambda: s2.block_mean_sd(2.0), lambda: s2.gradient_sd(0.0), lambda: s2.gradient_sd(np.nan)):
        with pytest.raises(ValueError):
            call()
    s4, _ = _ensemble(4)
    with pytest.raises(ValueError, match="does not fit"):
        posterior.PosteriorSummary(**{**vars(s4), "mean": s4.mean[:3], "sd": s4.sd[:3], "local_cross": s4.local_cross[:, :3],
                                      "local_centre": s4.local_centre[:3]}).block_mean_sd(4)


def test_save_load_round_trip(tmp_path):
    s, _ = _ensemble(2)
    s.save(tmp_path / "with.npz")
    got = posterior.PosteriorSummary.load(tmp_path / "with.npz")
    assert got.local_reach == 2 and isinstance(got.local_reach, int)
    for name in ("local_cross", "local_centre", "mean", "sd"):
        assert np.array_equal(getattr(got, name), getattr(s, name)), name
    assert np.array_equal(got.local_covariance(), s.local_covariance(), equal_nan=True)
    assert np.array_equal(got.block_mean_sd(3), s.block_mean_sd(3), equal_nan=True)
    # a file written without the fields, as every file before them was
    old = {k: np.asarray(v) for k, v in dict(mean=s.mean, sd=s.sd, n_chains=3, n_sequences=6, n_per_sequence=8,
                                             snapshot_iterations=s.snapshot_iterations, burn_in=0, thin=10, split=True).items()}
    np.savez_compressed(tmp_path / "old.npz", **old)
    got = posterior.PosteriorSummary.load(tmp_path / "old.npz")
    assert got.local_cross is None and got.local_reach is None and got.local_centre is None
    with pytest.raises(ValueError, match="local"):
        got.local_covariance()


def test_cases_and_plan_of_the_device_tests():
    """What the device tests rely on, where it can be checked without a device: on 256 compute units the few-chain cases run one
    chain per part, the many-chain cases reach the regimes they are listed for, every reach meets a grid of several tiles in both
    directions, and the restated rule bounds the slab."""
    for (Hh, Ww, R, Cn, state) in lc.FEW:
        plan = lc.split_plan(Hh, Ww, R, Cn, 256)
        assert (plan["parts"], plan["cpp"], plan["empty"]) == (Cn, 1, 0), ((Hh, Ww, R, Cn), plan)
    for key, exp in lc.MANY.items():
        plan = lc.split_plan(*key[:4], 256)
        assert (plan["parts"], plan["cpp"], plan["last"], plan["empty"]) == exp, (key, plan)
    assert any(v[2] < v[1] and v[3] >= 1 for v in lc.MANY.values()) and {k[3] for k in lc.MANY} == {101, 390}
    for R in (1, 2, 3, 4):
        assert any(r == R and -(-Hh // 8) > 1 and -(-Ww // 64) > 1 for (Hh, Ww, r, _, _) in lc.FEW), R
    assert {k[4] for k in lc.FEW} == {"f64", "f32"} and all(3 <= c[3] <= 8 for c in lc.FEW)
    assert lc.split_plan(256, 256, 4, 1024, 256) == dict(parts=4, cpp=256, last=256, empty=0)
    assert lc.split_plan(256, 256, 1, 1024, 256)["parts"] == 8                             # the device-filling rule where the slab is small
    assert lc.split_plan(1024, 1024, 4, 64, 4096)["parts"] == 3                             # a larger device: 3 x 40 planes of 8 MiB stay within 1 GiB
    assert lc.split_plan(1800, 1800, 4, 64, 4096)["parts"] == 1 and 40 * 1800 * 1800 <= 1 << 27 < 40 * 1900 * 1900   # beyond: refused


def test_device_bound_is_fair():
    """A plain float64 NumPy accumulation in chain order -- rounded differences, rounded products, rounded sums, nothing fused -- lies
    within the bound the device is held to, on every case the device tests feed."""
    worst = 0.0
    for case in lc.all_cases():
        Hh, Ww, R, Cn, state, nan_cells = case
        x, g = lc.case_beds(*case)
        got = lc.plain_float64(x, g, R)
        worst = max(worst, lc.check(got, x, g, R, label=f"plain float64 {Hh}x{Ww} R={R} C={Cn} {state}"))
        if nan_cells:
            assert np.array_equal(np.isnan(got), lc.nan_entries(Hh, Ww, R, nan_cells))
    print(f"plain float64 accumulation: at most {worst:.3f} of the device bound")
    assert worst <= 1.0
