"""NumPy restatement of the posterior covariance sums (mcmc_gpu_amd/posterior.py's docstring, `cov`) and the bounds of their
tests.  Shares nothing with the package; the sequences are those of tests/posterior_common.py.

Definitions.  x [C, T, H, W] the snapshots, g [H, W] the common field, d = x - g, Omega [K, H, W] the probes, m_k the number of
non-zero weights of probe k.  Projection p[c, k, t] = sum over the cells with Omega_k != 0 of Omega_k d (zero weights are skipped:
a NaN outside the support does not touch p, one inside makes it NaN).  Cross sum Y[k, cell] = sum over the chains and the
snapshots that belong to a sequence of d[c, t, cell] p[c, k, t]; a NaN d or p makes the entry NaN.

Bounds (derived, not tuned), u = 2^-53, references in np.longdouble on the bits the device sees (f32 data cast to f64).
  projection   a term fl(Omega fl(x - g)) carries one rounding in the difference and at most one in the product; the m_k terms are
               added with at most m_k - 1 roundings in any order (the terms of zero weight are exact zeros, and adding one is exact);
               one further unit covers the second-order terms.  With A = sum |Omega_k| |x - g|:
                   |p^ - p| <= (m_k + 3) u A
  cross, given the device's own p^ as input bits: a term carries one rounding in d and at most one in the product (none separate
               when the multiply-add is fused), n terms are added with at most n - 1 roundings in any order, one unit for the
               second order:
                   |Y^ - sum d p^| <= (n + 4) u sum |d| |p^|
  cross, end to end against the independent reference: the two composed,
                   |Y^ - Y| <= (n + 4) u sum |d| |p^| + sum_{c,t} |d| (m_k + 3) u A[c, t, k]
n is the number of terms added into a cell in all: chains x snapshots that belong to a sequence (x calls, for the C entry)."""
import math

import numpy as np

import posterior_common as pc

U = 2.0 ** -53
LD = np.longdouble


def first_used(T, split):
    """Index of the first snapshot that belongs to a sequence."""
    return T - 2 * (T // 2) if split else 0


def projection_reference(x, g, probes):
    """(p [C, K, T], A [C, K, T], m [K]) in np.longdouble: the projections, sum |Omega| |x - g| over the support, the support sizes."""
    x, g, probes = np.asarray(x, dtype=np.float64), np.asarray(g, dtype=np.float64), np.asarray(probes, dtype=np.float64)
    C, T = x.shape[:2]
    K = probes.shape[0]
    p, A = np.empty((C, K, T), dtype=LD), np.empty((C, K, T), dtype=LD)
    m = np.empty(K, dtype=np.int64)
    for k in range(K):
        nz = probes[k] != 0
        m[k] = nz.sum()
        w = probes[k][nz].astype(LD)
        d = x[:, :, nz].astype(LD) - g[nz].astype(LD)                # [C, T, m_k]
        p[:, k] = (w * d).sum(axis=-1)
        A[:, k] = (np.abs(w) * np.abs(d)).sum(axis=-1)
    return p, A, m


def _share(err, bound):
    ok = bound > 0
    return float((err[ok] / bound[ok]).max()) if ok.any() else 0.0


def check_projection(got, p, A, m, label=""):
    """Assert got [C, K, T] float64 against projection_reference within (m_k + 3) u A, NaN sets equal; prints and returns the
    largest error as a share of the bound."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == p.shape, (got.shape, p.shape)
    worst = 0.0
    for k in range(p.shape[1]):
        gk, rk = got[:, k], p[:, k]
        assert np.array_equal(np.isnan(gk), np.isnan(rk)), f"{label} probe {k}: NaN projections differ ({np.isnan(gk).sum()} vs {np.isnan(rk).sum()})"
        ok = ~np.isnan(rk)
        err = np.abs(gk[ok].astype(LD) - rk[ok])
        bound = (int(m[k]) + 3) * U * A[:, k][ok]
        share = _share(err, bound)
        worst = max(worst, share)
        print(f"projection {label} probe {k}: m_k={int(m[k])}, largest error {share:.3e} of the bound (m_k + 3) u A")
        assert (err <= bound).all(), f"{label} probe {k}: {int((err > bound).sum())} projections beyond (m_k + 3) u A, worst {share:.3e} of it"
    return worst


def cross_sums(x, g, plain, absolute, lo=0):
    """(sum d plain [Ka, H, W], sum |d| |absolute| [Kb, H, W]) in np.longdouble over all chains and the snapshots t >= lo, chain by
    chain; plain [C, Ka, T] and absolute [C, Kb, T] in any float type."""
    x, gl = np.asarray(x, dtype=np.float64), np.asarray(g, dtype=np.float64).astype(LD)
    plain, absolute = np.asarray(plain), np.asarray(absolute)
    s = np.zeros((plain.shape[1],) + gl.shape, dtype=LD)
    sa = np.zeros((absolute.shape[1],) + gl.shape, dtype=LD)
    with np.errstate(invalid="ignore"):
        for c in range(x.shape[0]):
            d = x[c, lo:].astype(LD) - gl                            # [T', H, W]
            s += np.tensordot(plain[c, :, lo:].astype(LD), d, axes=1)
            sa += np.tensordot(np.abs(absolute[c, :, lo:].astype(LD)), np.abs(d), axes=1)
    return s, sa


def check_cross(got, ref, bound, label=""):
    """Assert got [K, H, W] float64 against ref within bound (both np.longdouble), NaN sets equal; prints and returns the largest
    error as a share of the bound."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    worst = 0.0
    for k in range(ref.shape[0]):
        gk, rk = got[k], ref[k]
        assert np.array_equal(np.isnan(gk), np.isnan(rk)), f"{label} probe {k}: NaN cells differ ({np.isnan(gk).sum()} vs {np.isnan(rk).sum()})"
        ok = ~np.isnan(rk)
        err = np.abs(gk[ok].astype(LD) - rk[ok])
        share = _share(err, bound[k][ok])
        worst = max(worst, share)
        print(f"cross {label} probe {k}: largest error {share:.3e} of the bound")
        assert (err <= bound[k][ok]).all(), f"{label} probe {k}: {int((err > bound[k][ok]).sum())} cells beyond the bound, worst {share:.3e} of it"
    return worst


def check_cross_given(got, x, g, p_hat, lo, n, label=""):
    """got against sum d p^ with the device's own projections as input bits: (n + 4) u sum |d| |p^|."""
    ref, mag = cross_sums(x, g, p_hat, p_hat, lo)
    return check_cross(got, ref, (n + 4) * U * mag, label + " given p^")


def check_cross_both(got, x, g, ref_pam, p_hat, lo, n, label=""):
    """got against sum d p^ (the device's own projections as input bits) and against the independent reference, whose bound is
    (n + 4) u sum |d| |p^| + sum |d| (m_k + 3) u A; ref_pam = projection_reference(x, g, probes).  One pass over the snapshots
    serves both.  Returns the end-to-end bound [K, H, W]."""
    p, A, m = ref_pam
    K = p.shape[1]
    p_hat = np.asarray(p_hat, dtype=LD)
    refs, mags = cross_sums(x, g, np.concatenate([p_hat, p], axis=1), np.concatenate([p_hat, (m[None, :, None] + 3) * A], axis=1), lo)
    check_cross(got, refs[:K], (n + 4) * U * mags[:K], label + " given p^")
    bound = (n + 4) * U * mags[:K] + U * mags[K:]
    check_cross(got, refs[K:], bound, label + " end to end")
    return bound


def covariance_formula(s):
    """[K, H, W] (Y_k - S1 q_k / n) / (n - 1) from the summary's own fields, S1 = n (mean - g), q_k the sum of the projections
    over the M N values; NaN where mean is NaN."""
    n = s.n_sequences * s.n_per_sequence
    g, P = np.asarray(s.probe_centre, dtype=np.float64), np.asarray(s.probes, dtype=np.float64)
    T = s.probe_values.shape[2]
    used = s.probe_values[:, :, first_used(T, s.split):]
    out = np.empty_like(P)
    with np.errstate(invalid="ignore"):
        for k in range(P.shape[0]):
            nz = P[k] != 0
            off = (P[k][nz] * g[nz]).sum()
            q = math.fsum(used[:, k].reshape(-1) - off)                  # exactly rounded, whatever the order
            out[k] = (s.probe_cross[k] - n * (s.mean - g) * q / n) / (n - 1)
    out[:, np.isnan(s.mean)] = np.nan
    return out


# (H, W, chains, state) of MANY in tests/test_gpu_posterior_ess.py that this suite runs, and what the cross pass must reach on a
# device of 256 compute units: (vec, parts, cpp)
MANY_PLAN = {
    (128, 128, 390, "f32"): (4, 64, 7),
    (126, 129, 200, "f32"): (2, 32, 7),
    (127, 129, 101, "f64"): (1, 16, 7),
}


def cross_split_plan(H, W, n_chains, f32_state, n_cu):
    """How gsm_posterior_cross divides n_chains beds of H x W on a device of n_cu compute units, restated from the comments of
    posterior_cov_kernel.hip (nothing of the library is called): vec cells per lane (16 bytes of bed where H W allows), workgroups
    of 256 lanes along the cells, and the chain axis cut by the rule of posterior_parts, as pc.split_plan restates it."""
    plane = H * W
    vec = (4 if plane % 4 == 0 else 2 if plane % 2 == 0 else 1) if f32_state else (2 if plane % 2 == 0 else 1)
    return pc._chain_split((plane // vec + 255) // 256, n_chains, n_cu, vec)
