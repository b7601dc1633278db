"""NumPy restatement of the posterior definitions (mcmc_gpu_amd/posterior.py's docstring) and the tolerances of the posterior
tests.  Shares nothing with the package.

Tolerances (derived, not tuned).  With u = 2^-53, T terms and |d| <= D after the shift, recursive sums give
|err(s1)| <= T^2 u D, so a sequence mean is off by at most T u D + u |x|; the variance formula cancels s2 against s1^2 / N, both
<= N D^2, so its absolute error is a few u D^2.  In these tests T <= 20, D <= 1e3 m, |x| <= 1e6 + 10: the mean's error is bounded
near 1e-10 m and a variance's near 1e-10 m^2.  Asserted: mean within 1e-9 m (conditioning case: 1e-8 m, u |x| being 1e-10
there), variances (sd^2, W, B_over_N) within 1e-9 relative plus 1e-9 m^2, rhat within 1e-7 relative.

Dependence on the chain count C (tests/test_gpu_posterior_many_chains.py: C up to 390, T <= 5).  P0 = sum_m a_m is a sum of M = 2C
sequence means of size <= D, taken chain by chain inside a part and part by part after it; whatever the order, its error is at
most M u sum|a_m| <= M^2 u D, so mean = g + P0 / M is off by at most M u D + u |x|: n u D with n = M N values in the pooled form.
For M = 780, N = 2, D = 1e3 m that is 780 * 1.1e-16 * 1e3 = 9e-11 m and 2e-10 m for n = 1950, under the 1e-9 m asserted; the
bound does not grow with the number of parts.  ss_between = P1 - P0^2 / M cancels two terms <= M D^2, each known to M u
relative: absolute error <= 2 M^2 u D^2 against a value near M var(mu), i.e. a relative error near M u D^2 / var(mu) = 1e-13 for
D^2 / var(mu) <= 10; P2 is a sum of non-negative terms, relative error <= M u = 9e-14.  These are worst cases for errors that
all point one way.  The kernels' own order (per-chain shifted sums, close, per-part sums in chain order, parts in part order,
posterior.finalize) emulated in NumPy by emulate_partials below, on the shapes and draws of the many-chain tests, is off from
posterior_reference by at most: mean 1.2e-12 m, variances 1.4e-10 m^2 absolute and 1.5e-14 relative, rhat 3.1e-15 relative.  So
the reference and the summation order together use under a thousandth of every tolerance at these chain counts, and the tolerances
stay as they are (tests/test_posterior_host.py keeps that checked without a device)."""
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


def _chain_split(cell_blocks, n_chains, n_cu, vec):
    parts = max(1, min(-(-4 * n_cu // cell_blocks), n_chains))
    cpp = -(-n_chains // parts)
    filled = -(-n_chains // cpp)                                 # parts with c0 < n_chains
    return dict(vec=vec, parts=parts, cpp=cpp, last=n_chains - (filled - 1) * cpp, empty=parts - filled)


def split_plan(H, W, n_chains, f32_state, n_cu):
    """How the kernels divide n_chains beds of H x W on a device of n_cu compute units, restated from the comments of
    posterior_kernel.hip and gsm_api_posterior.hip (nothing of the library is called).  The pooled and the partials form cut
    the chain axis into parts = min(ceil(4 n_cu / cell_blocks), n_chains) of cpp = ceil(n_chains / parts) chains, cell_blocks
    workgroups of 256 lanes with vec cells per lane (pooled: 16 bytes per lane where H W allows; partials: one cell); `last`
    is the chain count of the last part that holds a chain and `empty` the number of parts after it.  The per-chain accumulate
    runs flat over n = n_chains H W in groups of V = 16 bytes / state size cells, 512 groups per workgroup and trip, on
    min(workgroups wanted, 8 n_cu) workgroups: `trips` is the largest trip count of a workgroup, `last_trip_blocks` how many
    workgroups take the last trip (< grid: partly live), `last_block_groups` the groups of the last wanted workgroup (< 512:
    some of its lanes are dead in that trip) and `tail` = n % V."""
    plane = H * W
    vec = (4 if plane % 4 == 0 else 2 if plane % 2 == 0 else 1) if f32_state else (2 if plane % 2 == 0 else 1)
    V = 4 if f32_state else 2
    n = n_chains * plane
    groups = n // V
    want = -(-groups // 512)
    grid = max(1, min(want, 8 * n_cu))
    trips = max(1, -(-want // grid))
    return dict(pooled=_chain_split((plane // vec + 255) // 256, n_chains, n_cu, vec),
                partials=_chain_split((plane + 255) // 256, n_chains, n_cu, 1),
                accumulate=dict(V=V, grid=grid, trips=trips, last_trip_blocks=want - (trips - 1) * grid,
                                last_block_groups=groups - (want - 1) * 512, tail=n % V))


def many_chain_data(C, T, H, W, seed, f32=True):
    """(x [C, T, H, W], g [H, W]) of the many-chain tests, drawn as test_kernels_against_numpy draws them: x = -300 + 100 N(0, 1)
    (rounded to float with f32, so that both state types see the same values), g = -300 + 10 N(0, 1); cells [10:14, 10:20]
    constant within every chain, cells [20:22, 5:9] constant within each half of every chain with a step between the halves,
    and one NaN at cell (5, 7) of the last chain (it lies in the last part that holds chains, the ragged one) at snapshot T - 2."""
    rng = np.random.default_rng(seed)
    x = -300.0 + 100.0 * rng.normal(size=(C, T, H, W))
    x[:, :, 10:14, 10:20] = x[:, :1, 10:14, 10:20]
    half = T - T // 2
    x[:, :half, 20:22, 5:9] = x[:, :1, 20:22, 5:9]
    x[:, half:, 20:22, 5:9] = x[:, half:half + 1, 20:22, 5:9]
    x[C - 1, T - 2, 5, 7] = np.nan
    g = -300.0 + 10.0 * rng.normal(size=(H, W))
    if f32:
        x = x.astype(np.float32).astype(np.float64)
    return x, g


def constant_cells(H, W, split):
    """Cells of many_chain_data where every sequence is constant: W == 0 and rhat NaN exactly."""
    const = np.zeros((H, W), dtype=bool)
    const[10:14, 10:20] = True
    const[20:22, 5:9] = split
    return const


def emulate_partials(x, g, split, rhat, parts, cpp):
    """[3, ...] partials of x [C, T, ...] summed in the kernels' own order, in float64 NumPy.  rhat: per chain and sequence the
    sums of d = x - ref (ref: the sequence's first snapshot) snapshot by snapshot, a = (ref - g) + s1 / N and v = (s2 - s1^2 / N) /
    (N - 1), then per part a, a^2 and v added chain by chain and sequence by sequence, the parts added in part order.  Without:
    per snapshot and part d = x - g and d^2 added chain by chain, the parts added in part order onto the running sums."""
    x = np.asarray(x, dtype=np.float64)
    C, T = x.shape[:2]
    n_seq = 2 if split else 1
    N = T // 2 if split else T
    used = x[:, T - n_seq * N:]
    zero = lambda: np.zeros(x.shape[2:])
    out = [zero(), zero(), zero()]
    with np.errstate(invalid="ignore"):
        if rhat:
            a, v = np.empty((C, n_seq) + x.shape[2:]), np.empty((C, n_seq) + x.shape[2:])
            for k in range(n_seq):
                ref = used[:, k * N]
                s1, s2 = np.zeros_like(ref), np.zeros_like(ref)
                for t in range(k * N, (k + 1) * N):
                    d = used[:, t] - ref
                    s1 = s1 + d
                    s2 = s2 + d * d
                a[:, k] = (ref - g) + s1 / N
                v[:, k] = (s2 - s1 * s1 / N) / (N - 1.0)
            for p in range(parts):
                slab = [zero(), zero(), zero()]
                for c in range(p * cpp, min(C, (p + 1) * cpp)):
                    for k in range(n_seq):
                        slab[0] = slab[0] + a[c, k]
                        slab[1] = slab[1] + a[c, k] * a[c, k]
                        slab[2] = slab[2] + v[c, k]
                out = [o + s for o, s in zip(out, slab)]
        else:
            for t in range(used.shape[1]):
                tot = [zero(), zero()]
                for p in range(parts):
                    slab = [zero(), zero()]
                    for c in range(p * cpp, min(C, (p + 1) * cpp)):
                        d = used[c, t] - g
                        slab[0] = slab[0] + d
                        slab[1] = slab[1] + d * d
                    tot = [o + s for o, s in zip(tot, slab)]
                out[0], out[1] = out[0] + tot[0], out[1] + tot[1]
    return np.stack(out)


def extended_pooled_sums(x, split, g):
    """(sum d, sum |d|, sum d^2, n) per cell over the n used values of x [C, T, H, W], d = x - g, in np.longdouble, chain by chain."""
    C, T = x.shape[:2]
    N = T // 2 if split else T
    lo = T - (2 * N if split else N)
    gl = np.asarray(g, dtype=np.longdouble)
    s, sa, sq = (np.zeros(g.shape, dtype=np.longdouble) for _ in range(3))
    for c in range(C):
        d = x[c, lo:].astype(np.longdouble) - gl
        s += d.sum(axis=0)
        sa += np.abs(d).sum(axis=0)
        sq += (d * d).sum(axis=0)
    return s, sa, sq, C * (T - lo)
