"""NumPy restatement of the effective-sample-size definitions (mcmc_gpu_amd/posterior.py's docstring, `ess`) and the bound of the
lagged sums' tests.  Shares nothing with the package; the sequences are those of tests/posterior_common.py.

Per cell and lag t = 1 .. K:  S_t = sum_m sum_{n=0}^{N-1-t} (x[n+t, m] - x[n, m])^2 over the M sequences, V_t = S_t / (M (N - t)),
var+ = (N - 1)/N W + B/N, rho_t = 1 - V_t / (2 var+), rho_0 = 1.  Geyer pairs P_k = rho_2k + rho_(2k+1), k = 0 .. (K - 1)/2; k* the
first k with P_k < 0; tau = -1 + 2 sum_{k < k*} P_k (all pairs, and `truncated`, when none is negative), floored at 1 / log10(M N);
ess = M N / tau, mcse = sd / sqrt(ess); NaN where W == 0 and where the cell saw a NaN.

Bound of the device sums (derived, not tuned).  With u = 2^-53 a term fl(fl(a - b)^2) carries one rounding in the difference,
doubled by the square, and one in the product; n_t = M (N - t) non-negative terms are added with at most n_t - 1 roundings in
any order; one unit covers the second-order terms: |S_t(device) - S_t| <= (n_t + 4) u S_t.  With fp32 state the reference sees
the same float values cast to double, so the bound is unchanged.  Cells constant within every sequence give exactly 0."""
import math

import numpy as np

import posterior_common as pc

U = 2.0 ** -53


def lag_sqdiff_reference(x, split, K):
    """[K, H, W] np.longdouble S_t of the snapshots x [C, T, H, W]: differences, squares and sums in extended precision,
    sequence by sequence."""
    s = pc.sequences(x, split)
    M, N = s.shape[:2]
    out = np.zeros((K,) + s.shape[2:], dtype=np.longdouble)
    for m in range(M):
        sm = s[m].astype(np.longdouble)
        for t in range(1, K + 1):
            if t < N:
                d = sm[t:] - sm[:N - t]
                out[t - 1] += (d * d).sum(axis=0)
    return out


def check_lag_sqdiff(got, ref, M, N, label=""):
    """Assert got [K, H, W] float64 against lag_sqdiff_reference within (n_t + 4) u relative, atol 0; NaN cells must agree.
    Prints and returns the largest error as a share of the bound."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    worst = 0.0
    for t in range(1, ref.shape[0] + 1):
        g, r = got[t - 1], ref[t - 1]
        assert np.array_equal(np.isnan(g), np.isnan(r)), f"{label} lag {t}: NaN cells differ ({np.isnan(g).sum()} vs {np.isnan(r).sum()})"
        ok = ~np.isnan(r)
        n_t = M * (N - t)
        err = np.abs(g[ok].astype(np.longdouble) - r[ok])
        bound = (n_t + 4) * U * r[ok]
        share = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
        worst = max(worst, share)
        print(f"lag_sqdiff {label} lag {t}: n_t={n_t}, largest error {share:.3e} of the bound (n_t + 4) u S_t")
        assert (err <= bound).all(), f"{label} lag {t}: {int((err > bound).sum())} cells beyond (n_t + 4) u S_t, worst {share:.3e} of it"
    return worst


def ess_loop(lag_sqdiff, W, B_over_N, mean, sd, M, N):
    """(rho [K, H, W], ess, truncated, mcse, tau before the floor) cell by cell in plain Python floats."""
    S = np.asarray(lag_sqdiff, dtype=np.float64)
    K, H, Wd = S.shape
    rho = np.full((K, H, Wd), np.nan)
    ess = np.full((H, Wd), np.nan)
    mcse = np.full((H, Wd), np.nan)
    tau_raw = np.full((H, Wd), np.nan)
    trunc = np.zeros((H, Wd), dtype=bool)
    floor = 1.0 / math.log10(M * N)
    for i in range(H):
        for j in range(Wd):
            w, b = float(W[i, j]), float(B_over_N[i, j])
            if w == 0 or math.isnan(w) or math.isnan(float(mean[i, j])):
                continue
            vp = (N - 1) / N * w + b
            r = [1.0] + [1.0 - float(S[t - 1, i, j]) / (M * (N - t)) / (2.0 * vp) for t in range(1, K + 1)]
            rho[:, i, j] = r[1:]
            if any(math.isnan(v) for v in r):
                continue
            tau, cut = -1.0, False
            for k in range((K + 1) // 2):
                p = r[2 * k] + r[2 * k + 1]
                if p < 0:
                    cut = True
                    break
                tau += 2.0 * p
            tau_raw[i, j] = tau
            trunc[i, j] = not cut
            tau = max(tau, floor)
            ess[i, j] = M * N / tau
            mcse[i, j] = float(sd[i, j]) / math.sqrt(ess[i, j])
    return rho, ess, trunc, mcse, tau_raw


def lag_split_plan(H, W, n_chains, f32_state, n_cu):
    """How gsm_posterior_lagged divides n_chains beds of H x W on a device of n_cu compute units, restated from the comments of
    posterior_lag_kernel.hip (nothing of the library is called): vec cells per lane (16 bytes where H W allows), cell_blocks
    workgroups of 256 lanes, and the chain axis cut by the rule of posterior_parts, as pc.split_plan restates it."""
    plane = H * W
    vec = (4 if plane % 4 == 0 else 2 if plane % 2 == 0 else 1) if f32_state else (2 if plane % 2 == 0 else 1)
    return pc._chain_split((plane // vec + 255) // 256, n_chains, n_cu, vec)


def ar1_chains(phi, M, N, cells, burn, seed=3):
    """[M, N, cells] AR(1) sequences with coefficient phi after `burn` discarded steps: noise from default_rng(seed).normal(size=(M,
    N + burn, cells)), the first value of each chain equal to its first noise value."""
    e = np.random.default_rng(seed).normal(size=(M, N + burn, cells))
    x = np.empty_like(e)
    x[:, 0] = e[:, 0]
    for n in range(1, N + burn):
        x[:, n] = phi * x[:, n - 1] + e[:, n]
    return x[:, burn:]
