"""NumPy restatement of the posterior definitions (mcmc_gpu_amd/posterior.py's docstring) and the tolerances of the posterior
tests.  Shares nothing with the package.

Tolerances (derived, not tuned).  With u = 2^-53, T terms and |d| <= D after the shift, recursive sums give
|err(s1)| <= T^2 u D, so a sequence mean is off by at most T u D + u |x|; the variance formula cancels s2 against s1^2 / N, both
<= N D^2, so its absolute error is a few u D^2.  In these tests T <= 20, D <= 1e3 m, |x| <= 1e6 + 10: the mean's error is bounded
near 1e-10 m and a variance's near 1e-10 m^2.  Asserted: mean within 1e-9 m (conditioning case: 1e-8 m, u |x| being 1e-10
there), variances (sd^2, W, B_over_N) within 1e-9 relative plus 1e-9 m^2, rhat within 1e-7 relative."""
import numpy as np

MEAN_ATOL = 1e-9
VAR_RTOL, VAR_ATOL = 1e-9, 1e-9
RHAT_RTOL = 1e-7


def sequences(x, split):
    """x [C, T, H, W] -> the sequences [M, N, H, W] of the definitions (split: the last 2N snapshots, two halves per chain)."""
    x = np.asarray(x, dtype=np.float64)
    C, T = x.shape[:2]
    if not split:
        return x
    N = T // 2
    return x[:, T - 2 * N:].reshape((2 * C, N) + x.shape[2:])


def posterior_reference(x, split):
    """mean, sd, within_var (W), between_var_over_n, rhat per cell from the stacked snapshots x [C, T, H, W].  The variance of
    a sequence whose values are all equal is 0 (np.var may give ~1e-33 for it: the mean of N equal values need not be that
    value in floating point), so rhat is NaN exactly where every sequence is constant."""
    s = sequences(x, split)
    M, N = s.shape[:2]
    flat = s.reshape((M * N,) + s.shape[2:])
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.mean(flat, axis=0)
        var = np.var(flat, axis=0, ddof=1)
        mu = np.mean(s, axis=1)
        v = np.where((s == s[:, :1]).all(axis=1), 0.0, np.var(s, axis=1, ddof=1))
        W = np.mean(v, axis=0)
        B = np.var(mu, axis=0, ddof=1)
        rhat = np.where(W == 0, np.nan, np.sqrt(((N - 1) / N * W + B) / W))
    return dict(mean=mean, sd=np.sqrt(var), within_var=W, between_var_over_n=B, rhat=rhat, M=M, N=N)


def numpy_partials(x, split, g):
    """[3, H, W] partials of the chains x [C, T, H, W] as gsm_posterior_partials defines them, in NumPy."""
    s = sequences(x, split)
    a = np.mean(s, axis=1) - g
    v = np.where((s == s[:, :1]).all(axis=1), 0.0, np.var(s, axis=1, ddof=1))
    return np.stack([a.sum(axis=0), (a * a).sum(axis=0), v.sum(axis=0)])


def numpy_pooled_partials(x, split, g):
    """[3, H, W] partials of the pooled form (rhat=False): sum d, sum d^2 over all used values, d = x - g; third field 0."""
    s = sequences(x, split)
    d = s.reshape((-1,) + s.shape[2:]) - g
    return np.stack([d.sum(axis=0), (d * d).sum(axis=0), np.zeros(g.shape)])


def _err(got, exp, what):
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    assert got.shape == exp.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(exp)), f"{what}: NaN cells differ ({np.isnan(got).sum()} vs {np.isnan(exp).sum()})"
    ok = ~np.isnan(exp)
    return np.abs(got[ok] - exp[ok]), np.abs(exp[ok])


def check_maps(summary, ref, mean_atol=MEAN_ATOL, rhat=True, label=""):
    """Assert the maps of a PosteriorSummary against posterior_reference's within the module's tolerances; prints and returns
    the largest errors."""
    out = {}
    e, _ = _err(summary.mean, ref["mean"], "mean")
    out["mean_abs"] = float(e.max())
    pairs = [("sd^2", np.square(summary.sd), np.square(ref["sd"]))]
    if rhat:
        pairs += [("W", summary.within_var, ref["within_var"]), ("B_over_N", summary.between_var_over_n, ref["between_var_over_n"])]
    worst = {}
    for name, got, exp in pairs:
        e2, mag = _err(got, exp, name)
        worst[name] = (e2, mag)
        out[name + "_rel"] = float((e2[mag > 0] / mag[mag > 0]).max())
        out[name + "_abs"] = float(e2.max())
    if rhat:
        er, mr = _err(summary.rhat, ref["rhat"], "rhat")
        out["rhat_rel"] = float((er / mr).max()) if er.size else 0.0
    print(f"posterior errors {label}: " + ", ".join(f"{k}={v:.3e}" for k, v in out.items()))
    assert out["mean_abs"] <= mean_atol, out
    for name, (e2, mag) in worst.items():
        assert (e2 <= VAR_RTOL * mag + VAR_ATOL).all(), (name, out)
    if rhat:
        assert out["rhat_rel"] <= RHAT_RTOL, out
    return out
