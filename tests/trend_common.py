"""Shared by tests/test_trend_host.py and tests/test_gpu_trend.py: the cases of the Gaussian trend filter, a numpy.longdouble
restatement of its two passes, and the bar both scipy and the device are held to.

The restatement takes the very float64 weights the device takes (sgs.gaussian_weights: scipy's NumPy arithmetic) and computes, per
axis, out[i] = sum_k w[k] x[refl(i + k - lw)] with every product and sum in long double (64-bit mantissa on x86: its own rounding,
about taps * 2^-64, is 2^-11 of the bar and is ignored).  Axis 0 first, then axis 1 on the long-double result.

The bar, per cell: a float64 sum of `taps` products, in ANY order and with or without fused multiply-adds, is within
(taps + 1) 2^-53 of sum |w||x| to first order (taps - 1 additions, one rounding per product, (1 + u)^n growth absorbed by the spare
unit).  The second pass filters the first pass's rounded result -- its error passes through the second filter, whose weights are
positive and sum to 1 -- and adds its own.  So
    B = (taps0 + 2 + taps1 + 2) 2^-53 F(|x|),        F = the same filter applied to |x| in long double,
which is 2 (taps + 2) 2^-53 F(|x|) when both axes share a sigma.  It follows from the number format and the length of the sums alone,
not from any implementation's measured error; scipy (which pairs the symmetric taps) and the device (one ascending chain of fused
multiply-adds) must both lie within it, and then within 2 B of each other."""
import numpy as np

from mcmc_gpu_amd.sgs import gaussian_weights

# (H, W, sigma) -- sigma a number or (sigma_rows, sigma_columns).  At sigma = 10 the half-width is 40 cells (81 taps).
HOST_CASES = [(1, 7, 10), (7, 1, 10), (2, 3, 10), (13, 37, 10), (40, 41, 10), (41, 40, 10), (81, 17, 10), (64, 64, 10), (96, 130, 10),
              (33, 100, 3), (50, 20, 0.7)]
#   (1, 7) (7, 1) (2, 3)   an axis of one cell; axes far shorter than the half-width: the reflection folds up to 40 times
#   (13, 37)               both axes shorter than the half-width, odd
#   (40, 41) (41, 40)      an axis of exactly lw and lw + 1 cells
#   (81, 17)               an axis of exactly `taps` cells; two row chunks of the axis-0 kernel (64 rows each)
#   (64, 64)               exactly one column tile and one row chunk
#   (96, 130)              three column tiles (64) with a ragged last one, a ragged second row chunk, W even
#   (33, 100) sigma 3      lw = 12; (50, 20) sigma 0.7: lw = 3, fewer taps (7) than the axis-0 kernel's run of 16 outputs
GPU_CASES = HOST_CASES + [(65, 130, 10), (40, 80, 10), (45, 70, (3, 10))]
#   (65, 130)              one row past a row chunk, one wavefront's run of 16 rows holding a single row
#   (40, 80)               H = lw
#   (45, 70) (3, 10)       a different half-width per axis


def case_id(c):
    return f"{c[0]}x{c[1]}-s{c[2]}".replace(" ", "")


def sigmas(sigma):
    s = np.atleast_1d(np.asarray(sigma, dtype=np.float64))
    return float(s[0]), float(s[-1])


def fields(H, W, n=3, seed=0):
    """n distinct fields of a bed's magnitude: a smooth part of hundreds of metres and roughness, both signs."""
    rng = np.random.default_rng([seed, H, W])
    i, j = np.mgrid[0:H, 0:W]
    out = [300.0 * np.sin(0.07 * i + 0.3 * r) * np.cos(0.05 * j - r) + 40.0 * rng.standard_normal((H, W)) - 150.0 * r for r in range(n)]
    return np.ascontiguousarray(np.stack(out))


def refl(i, n):
    """scipy's mode='reflect' (half-sample symmetric, d c b a | a b c d | d c b a), any integer i."""
    m = np.mod(i, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def _pass(x, w, axis):
    lw = w.size // 2
    n = x.shape[axis]
    idx = refl(np.arange(n)[:, None] + np.arange(w.size)[None, :] - lw, n)          # [i, k]
    xm = np.moveaxis(x, axis, 0)                                                     # [n, rest]
    wl = w.astype(np.longdouble).reshape((1, -1) + (1,) * (xm.ndim - 1))
    return np.moveaxis((xm[idx] * wl).sum(axis=1), 0, axis)


def restatement(x, sigma, truncate=4.0):
    """The filter of one field [H, W] in long double; returns a longdouble array."""
    s0, s1 = sigmas(sigma)
    return _pass(_pass(np.asarray(x, dtype=np.longdouble), gaussian_weights(s0, truncate), 0), gaussian_weights(s1, truncate), 1)


def bar(x, sigma, truncate=4.0):
    """B of the module docstring for one field, float64 [H, W]."""
    s0, s1 = sigmas(sigma)
    t0, t1 = gaussian_weights(s0, truncate).size, gaussian_weights(s1, truncate).size
    return np.asarray((t0 + t1 + 4) * 2.0 ** -53 * restatement(np.abs(x), sigma, truncate), dtype=np.float64)


def worst_ratio(got, x, sigma):
    """max over cells of |got - restatement| / B."""
    err = np.abs(np.asarray(got, dtype=np.longdouble) - restatement(x, sigma))
    return float(np.max(err / bar(x, sigma)))
