"""Host suite of the posterior covariance with linear functionals (mcmc_gpu_amd/posterior.py `cov`): the option checks, the
library's symbols, the summary's host arithmetic against np.cov on a small ensemble, save / load, and the probe helpers.  No device
is used.  Definitions: tests/posterior_cov_common.py."""
import numpy as np
import pytest

import posterior_cov_common as cc
from mcmc_gpu_amd import _lib, posterior

H, W = 5, 7


def _options(cov, **kw):
    return posterior.check_options(dict(burn_in=0, thin=10, cov=cov, **kw), 100)


def test_option_checks():
    assert "cov" in posterior.POSTERIOR_KEYS
    assert _options(None)["cov"] is None
    rng = np.random.default_rng(0)
    P = rng.normal(size=(3, H, W))
    opt = _options(dict(probes=P))
    assert np.array_equal(opt["cov"]["probes"], P) and opt["cov"]["probes"].dtype == np.float64 and opt["cov"]["names"] is None
    assert _options(dict(probes=P[0]))["cov"]["probes"].shape == (1, H, W)               # one field [H, W]
    assert _options(dict(probes=P.astype(np.float32), names=["a", "b", "c"]))["cov"]["names"] == ("a", "b", "c")
    assert _options(dict(probes=rng.normal(size=(15, H, W))))["cov"]["probes"].shape == (15, H, W)
    for rhat in (True, False):                                                           # works with either form of the moments
        assert _options(dict(probes=P), rhat=rhat)["cov"] is not None
    assert posterior.check_cov(opt["cov"], H, W)["probes"].shape == (3, H, W)            # what check_options returns is accepted again
    bad_inf, bad_zero = P.copy(), P.copy()
    bad_inf[1, 2, 3] = np.inf
    bad_zero[2] = 0.0
    refused = [dict(probes=np.zeros((0, H, W))), dict(probes=rng.normal(size=(16, H, W))), dict(probes=rng.normal(size=(H * W,))),
               dict(probes=rng.normal(size=(2, 3, H, W))), dict(probes=bad_inf), dict(probes=np.where(P > 1, np.nan, P)), dict(probes=bad_zero),
               dict(probes=P, names=["a", "b"]), dict(probes=P, names="abc"), dict(probes=P, weights=1), dict(names=["a"]), P, True]
    for cov in refused:
        with pytest.raises(ValueError, match="cov"):
            _options(cov)
    with pytest.raises(ValueError, match="cov"):                                          # the grid's shape, where it is known
        posterior.check_cov(dict(probes=P), H, W + 1)
    with pytest.raises(ValueError, match="cov"):
        posterior.check_options(dict(burn_in=0, thin=10, covariance=dict(probes=P)), 100)


def test_library_declares_and_exports_the_entries():
    names = _lib.declared_symbols()
    lib = _lib.load()
    for name in ("gsm_posterior_project", "gsm_posterior_cross"):
        assert name in names and hasattr(lib, name), name
    assert "posterior_cov_kernel.hip" in _lib.SOURCES


def _ensemble(split=True):
    """3 chains x 17 snapshots x 5 x 7 cells, split: 6 sequences of 8 snapshots, the first snapshot dropped; cell (4, 6) never
    changes.  Returns the hand-built summary, the pooled values [48, H, W] and the pooled functionals [48, K]."""
    rng = np.random.default_rng(11)
    C, T, K = 3, 17, 3
    x = -300.0 + 100.0 * rng.normal(size=(C, T, H, W)) + 40.0 * rng.normal(size=(C, T, 1, 1))     # a common part: cells co-vary
    x[:, :, 4, 6] = -250.0
    N, lo = T // 2, 1
    M = 2 * C
    pooled = x[:, lo:].reshape(M * N, H, W)
    mean, sd = pooled.mean(axis=0), pooled.std(axis=0, ddof=1)
    sd[4, 6] = 0.0
    g = mean + 0.5 * sd * rng.uniform(-1, 1, size=(H, W))                                       # within one sd of the mean
    mask = np.zeros((H, W), dtype=bool)
    mask[1:4, 2:6] = True
    probes = np.concatenate([posterior.point_probes(H, W, [2 * W + 3]), posterior.region_mean_probes(mask), rng.normal(size=(1, H, W))])
    p, _, _ = cc.projection_reference(x, g, probes)
    cross, _ = cc.cross_sums(x, g, p, p, lo)
    values = np.einsum("khw,cthw->ckt", probes, x)
    s = posterior.PosteriorSummary(mean=mean, sd=sd, rhat=None, within_var=None, between_var_over_n=None, n_chains=C, n_sequences=M,
                                   n_per_sequence=N, snapshot_iterations=np.arange(T) * 10, burn_in=0, thin=10, split=True,
                                   probes=probes, probe_names=("point", "block", "gauss"), probe_values=values,
                                   probe_cross=cross.astype(np.float64), probe_centre=g)
    return s, pooled, values[:, :, lo:].transpose(0, 2, 1).reshape(M * N, K)


def test_host_arithmetic_against_numpy():
    s, pooled, f = _ensemble()
    n, K = f.shape
    var_f = f.var(axis=0, ddof=1)
    live = s.sd > 0
    exp = np.empty((K, H, W))
    for k in range(K):
        for i in range(H):
            for j in range(W):
                exp[k, i, j] = np.cov(pooled[:, i, j], f[:, k])[0, 1]
    cov = s.covariance()
    tol = 1e-12 * np.sqrt(np.square(s.sd)[None] * var_f[:, None, None])
    err = np.abs(cov - exp)
    print(f"covariance against np.cov: largest error {(err[:, live] / tol[:, live]).max():.3e} of 1e-12 sqrt(var_cell var_f)")
    assert (err[:, live] <= tol[:, live]).all()
    np.testing.assert_allclose(cov[:, live], cc.covariance_formula(s)[:, live], rtol=1e-13, atol=0)
    st = s.probe_stats()
    assert np.allclose(st["mean"], f.mean(axis=0), rtol=1e-13, atol=0)
    assert np.allclose(st["sd"], np.sqrt(var_f), rtol=1e-13, atol=0)
    full = np.cov(f.T)
    assert (np.abs(st["cov"] - full) <= 1e-12 * np.sqrt(np.outer(var_f, var_f))).all()
    # split R-hat of the functionals with the maps' conventions: 6 sequences of 8
    seq = f.reshape(s.n_sequences, s.n_per_sequence, K)
    Wv, B = seq.var(axis=1, ddof=1).mean(axis=0), seq.mean(axis=1).var(axis=0, ddof=1)
    N = s.n_per_sequence
    assert np.allclose(st["rhat"], np.sqrt(((N - 1) / N * Wv + B) / Wv), rtol=1e-13, atol=0)
    # a point probe at its own cell: the cell's variance, correlation 1
    assert abs(cov[0, 2, 3] - s.sd[2, 3] ** 2) <= tol[0, 2, 3]
    rho = s.correlation()
    assert abs(rho[0, 2, 3] - 1.0) <= 1e-12
    assert np.array_equal(np.isnan(rho), np.broadcast_to(~live, rho.shape)) and (np.abs(rho[:, live]) <= 1 + 1e-12).all()
    probes, c2 = s.sketch()
    assert np.array_equal(probes, s.probes) and np.array_equal(c2, cov, equal_nan=True)


def test_nan_mean_and_missing_probes():
    s, _, _ = _ensemble()
    s.mean = s.mean.copy()
    s.mean[0, 0] = np.nan
    cov = s.covariance()
    assert np.isnan(cov[:, 0, 0]).all() and np.isnan(cov).sum() == cov.shape[0]
    bare = posterior.PosteriorSummary(mean=s.mean, sd=s.sd, rhat=None, within_var=None, between_var_over_n=None, n_chains=3, n_sequences=6,
                                      n_per_sequence=8, snapshot_iterations=s.snapshot_iterations, burn_in=0, thin=10, split=True)
    for method in (bare.covariance, bare.correlation, bare.probe_stats, bare.sketch):
        with pytest.raises(ValueError, match="probes"):
            method()


def test_save_load_round_trip(tmp_path):
    s, _, _ = _ensemble()
    s.save(tmp_path / "with.npz")
    got = posterior.PosteriorSummary.load(tmp_path / "with.npz")
    for name in ("probes", "probe_values", "probe_cross", "probe_centre", "mean", "sd"):
        assert np.array_equal(getattr(got, name), getattr(s, name)), name
    assert got.probe_names == ("point", "block", "gauss") and got.rhat is None
    assert np.array_equal(got.covariance(), s.covariance())
    s.probe_names = None                                                                 # names are optional
    s.save(tmp_path / "unnamed.npz")
    assert posterior.PosteriorSummary.load(tmp_path / "unnamed.npz").probe_names is None
    # a file written without the fields, as every file before them was
    old = {k: np.asarray(v) for k, v in dict(mean=s.mean, sd=s.sd, n_chains=3, n_sequences=6, n_per_sequence=8,
                                             snapshot_iterations=s.snapshot_iterations, burn_in=0, thin=10, split=True).items()}
    np.savez_compressed(tmp_path / "old.npz", **old)
    got = posterior.PosteriorSummary.load(tmp_path / "old.npz")
    assert got.probes is None and got.probe_names is None and got.probe_values is None and got.probe_cross is None
    with pytest.raises(ValueError, match="probes"):
        got.covariance()


def test_probe_helpers():
    P = posterior.point_probes(H, W, [0, 2 * W + 3, H * W - 1])
    assert P.shape == (3, H, W) and P.dtype == np.float64 and (P.sum(axis=(1, 2)) == 1).all()
    assert P[0, 0, 0] == 1 and P[1, 2, 3] == 1 and P[2, H - 1, W - 1] == 1 and (P != 0).sum() == 3
    for cells in ([H * W], [-1], [3, H * W + 2], []):
        with pytest.raises(ValueError, match="outside the grid"):
            posterior.point_probes(H, W, cells)
    masks = np.zeros((2, H, W), dtype=int)
    masks[0, 1:3, 2:5] = 1
    masks[1, :, 0] = 7                                                                   # non-zero = inside
    R = posterior.region_mean_probes(masks)
    assert R.shape == (2, H, W) and np.array_equal(R[0] != 0, masks[0] != 0) and np.array_equal(R[1] != 0, masks[1] != 0)
    assert (R[0][masks[0] != 0] == 1.0 / 6).all() and (R[1][masks[1] != 0] == 1.0 / H).all()
    assert posterior.region_mean_probes(masks[0]).shape == (1, H, W)
    with pytest.raises(ValueError, match="region_mean_probes"):
        posterior.region_mean_probes(np.zeros((2, H, W)))
    posterior.check_cov(dict(probes=np.concatenate([P, R])), H, W)                        # both are valid probes as they come
