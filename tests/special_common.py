"""CPU-only: inputs, references and bounds for the scalar special functions of csrc/normal_score.h, csrc/truncnorm.h and
local_cov_of (csrc/sgs_search.h), shared by tests/test_special_host.py (the g++ build: the bar is fair) and
tests/test_gpu_special.py (gsm_debug_special: the device compiler and its libm).

Point sets: the generators of tests/test_normal_score.py and tests/test_interp_sgs_host.py (same seeds, same regimes) plus every
switch point of the functions with both neighbours by nextafter, infinities and NaN.
References: scipy 1.15 (the contract of these functions is "as scipy computes it"); for truncnorm.ppf also mpmath at 70 digits,
Phi^-1(Phi(a) + q (Phi(b) - Phi(a))), in survival form for a >= 0; for local_cov_of mpmath on the same doubles.
Bounds: the ones the host tests hold, never tuned to a build.  Every `*_ratio` function returns |error| / bound per element
(NaN where the bound's own exclusion rule leaves the element out) after asserting what must hold exactly (NaN and infinities)."""
import functools

import mpmath as mp
import numpy as np
import scipy.special as sp
import scipy.stats as st

EPS = float(np.finfo(np.float64).eps)
EXP_M2 = 0.13533528323661269189                  # ndtri's switch between the central and the asymptotic form
Y_EXPM1 = -0.14541345786885906                   # ndtri_exp's switch to -ndtri(-expm1(y)): log1p(-exp(-2))
PPF_REGIMES = ("general", "deep_right", "deep_left", "infinite", "narrow")
MP_POINTS = 600                                   # points per regime that go to mpmath


def around(*vals):
    """Each value with both neighbours by nextafter."""
    v = np.asarray(vals, dtype=np.float64)
    return np.concatenate([np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)])


# ---- point sets ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def normal_score_points():
    """(p for ndtri, x for ndtr and erfc): tests/test_normal_score.py's, then the switch points."""
    rng = np.random.default_rng(0)
    p = np.concatenate([rng.random(200000), 10.0 ** rng.uniform(-300, 0, 50000), 1.0 - 10.0 ** rng.uniform(-16, 0, 50000),
                        [0.0, 1.0, 0.5, 0.13533528323661269, 1 - 0.13533528323661269, 1e-7, 1 - 1e-7],
                        around(EXP_M2, 1.0 - EXP_M2, np.exp(-32.0)), [5e-324, 2.2250738585072014e-308, -0.25, 1.25, np.nan]])
    x = np.concatenate([rng.normal(0, 3, 200000), rng.uniform(-40, 40, 50000), [0.0, -1.0, 1.0, np.sqrt(2), -np.sqrt(2), 8 * np.sqrt(2)],
                        around(np.sqrt(2), -np.sqrt(2), 8 * np.sqrt(2), -8 * np.sqrt(2), 1.0, -1.0, 8.0, -8.0),
                        [np.inf, -np.inf, np.nan]])
    return p, x


@functools.lru_cache(maxsize=None)
def truncnorm_scalar_points():
    """(x for log_ndtr, y for ndtri_exp, y for erfcx_pos): tests/test_interp_sgs_host.py's, then the switch points."""
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.uniform(-40, 10, 100000), -(10.0 ** rng.uniform(0, 3, 20000)), [0.0, -1.0, 1.0, -38.0, np.inf, -np.inf],
                        around(-1.0, -np.sqrt(2), -8 * np.sqrt(2)),
                        [-1e30, -1e51, -1e60, -1e154, -1e155, -1e200, -1e308, np.nan]])   # erfcx_pos beyond 1e50: y^6 would overflow
    y = np.concatenate([-(10.0 ** rng.uniform(-300, 300, 100000)), rng.uniform(-3, 0, 50000), [-2.0, Y_EXPM1, 0.0, -np.inf],
                        around(-2.0, Y_EXPM1, -32.0), [np.nan]])
    e = np.concatenate([rng.uniform(0, 12, 100000), 10.0 ** rng.uniform(-300, 8, 50000), [0.0], around(1.0, 8.0, 1e50),
                        [1e51, 2e51, 1e60, 1e154, 1e300, np.inf, np.nan]])
    return x, y, e


@functools.lru_cache(maxsize=None)
def ppf_points(region):
    """(q, a, b) of one regime of test_truncnorm_ppf_equals_scipy; "edges": the branch and mass-case switches a = 0 and b = 0
    with their neighbours, the extreme q, infinite bounds and NaN in every argument."""
    rng = np.random.default_rng(7)
    n = 60000
    q = np.concatenate([rng.random(n), 10.0 ** rng.uniform(-300, 0, n), 1.0 - 10.0 ** rng.uniform(-16, 0, n),
                        [0.0, 1.0, 1e-300, 1.0 - 1e-16, 0.5]])
    m = q.size
    if region == "general":
        a = rng.uniform(-6, 3, m); b = a + 10.0 ** rng.uniform(-3, 1.5, m)
    elif region == "deep_right":
        a = rng.uniform(0, 30, m); b = np.where(rng.random(m) < 0.5, np.inf, a + rng.uniform(0.1, 10, m))
    elif region == "deep_left":
        b = rng.uniform(-30, 0, m); a = np.where(rng.random(m) < 0.5, -np.inf, b - rng.uniform(0.1, 10, m))
    elif region == "infinite":
        a, b = np.full(m, -np.inf), np.full(m, np.inf)
    elif region == "narrow":
        a = rng.uniform(-8, 8, m); b = a + 1e-8
    else:
        assert region == "edges"
        z = around(0.0)
        ab = ([(v, v + 1.0) for v in z] + [(v, 7.0) for v in z] + [(v, np.inf) for v in z] + [(v, 1e-8) for v in z[:2]] +
              [(-1.5, v) for v in z] + [(-9.0, v) for v in z] + [(-np.inf, v) for v in z] + [(-1e-8, v) for v in z[1:]] +
              [(-np.inf, 1.0), (-1.0, np.inf), (-np.inf, np.inf), (2.0, np.inf), (-np.inf, -2.0), (6.0, np.inf), (-np.inf, -6.0),
               (30.0, np.inf), (-np.inf, -30.0)])
        qs = [0.0, 1.0, 1e-300, 1.0 - 1e-16, 5e-324, 0.1, 0.5, 0.9]
        tri = [(u, lo, hi) for lo, hi in ab for u in qs]
        tri += [(np.nan, -1.0, 1.0), (0.3, np.nan, 1.0), (0.3, -1.0, np.nan), (0.3, np.nan, -1.0), (0.3, 1.0, np.nan), (np.nan, np.nan, np.nan)]
        q, a, b = (np.array(v, dtype=np.float64) for v in zip(*tri))
    return tuple(np.ascontiguousarray(v) for v in (q, a, b))


def mp_subset(region):
    """Indices of the regime's points that go to mpmath: evenly spread over the three families of q, the listed q included."""
    m = ppf_points(region)[0].size
    return np.arange(m) if m <= MP_POINTS else np.unique(np.concatenate([np.linspace(0, m - 6, MP_POINTS - 5).astype(int), np.arange(m - 5, m)]))


@functools.lru_cache(maxsize=None)
def local_cov_points():
    """(h2, c0, sill) for local_cov_of: h in {0, 1e-160, 1 -+ ulp, 1} (as h2 = h * h, and h2 = 1 +- ulp itself), h log-uniform in
    [1e-8, 15] (exponent arguments down to -45 / -675), then h up to exp arguments of -700, and beyond (underflow)."""
    rng = np.random.default_rng(11)
    h = np.concatenate([[0.0, 1e-160], around(1.0), 10.0 ** rng.uniform(-8, np.log10(15.0), 4000), rng.uniform(0.0, 1.0, 1000),
                        rng.uniform(14.0, 15.275, 500),                        # Gaussian: -3 h^2 in [-700, -588]
                        rng.uniform(200.0, 233.33, 500),                       # exponential: -3 h in [-700, -600]
                        rng.uniform(233.4, 260.0, 200), [15.3, 16.0, 1e3, 1e155]])
    with np.errstate(over="ignore"):                                       # 1e155^2: h2 = inf
        h2 = np.concatenate([h * h, around(1.0)])
    c0 = np.concatenate([[1.0, 0.75], rng.uniform(0.1, 3.0, h2.size - 2)])
    sill = c0 + np.concatenate([[0.0, 0.25], rng.uniform(0.0, 0.5, h2.size - 2)])
    return tuple(np.ascontiguousarray(v) for v in (h2, c0, sill))


# ---- bounds against scipy ---------------------------------------------------------------------------------------------------
def _same_nonfinite(got, ref):
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin), "finite where scipy is not, or the reverse"
    np.testing.assert_array_equal(got[~fin], ref[~fin])
    return fin


def ndtri_ratio(p, got):
    """1e-14 relative everywhere; absolutely 4e-16 max(1, |x|) in the central form (exp(-2) <= p <= 1 - exp(-2): a rational
    function of p - 1/2, no libm call) and 4 eps (|x| + 1) in the asymptotic form, where 4e-16 max(1, |x|) is not a bound any two
    correct builds meet: the result is x0 - x1 on s = sqrt(-2 log p) >= 2, so an ulp of log(p) (eps s / 2 in s), the roundings of
    the square root, of x0 and of the quotient x1 put 2 eps s on each build, s <= |x| + 1 (s - |x| = log(s) / s + x1 < 0.92).
    scipy itself is up to 2.9 ulp (1.45 x 4e-16 max(1, |x|)) from mpmath at |x| in [1.1, 2.2] (3000 points, 50 digits), with
    glibc's correctly rounded log.  Infinities and NaN as scipy's."""
    with np.errstate(all="ignore"):
        ref = sp.ndtri(p)
    fin = _same_nonfinite(got, ref)
    err = np.abs(got[fin] - ref[fin])
    tol = ndtri_tolerance(p[fin], ref[fin])
    r = np.full(p.shape, np.nan)
    r[fin] = np.maximum(err / tol, err / (1e-14 * np.maximum(np.abs(ref[fin]), 1e-300)))
    return r


def ndtri_tolerance(p, ref):
    asym = (p < EXP_M2) | (p > 1.0 - EXP_M2)
    return np.where(asym, 4 * EPS * (np.abs(ref) + 1.0), 4e-16 * np.maximum(1.0, np.abs(ref)))


@functools.lru_cache(maxsize=None)
def ndtri_mpmath():
    """(indices into normal_score_points()[0], Phi^-1 by mpmath at 50 digits): 300 points of each family of p (uniform, towards
    0, towards 1), 600 with |x| in [1.1, 2.2] -- where the asymptotic form loses most -- and the switch points."""
    p = normal_score_points()[0]
    with np.errstate(all="ignore"):
        ref = sp.ndtri(p)
    mid = np.flatnonzero((np.abs(ref[:200000]) >= 1.1) & (np.abs(ref[:200000]) <= 2.2))[:600]
    idx = np.unique(np.concatenate([np.arange(0, 200000, 667), np.arange(200000, 250000, 167), np.arange(250000, 300000, 167), mid,
                                    np.arange(300000, p.size)]))
    idx = idx[np.isfinite(ref[idx])]
    out = []
    with mp.workdps(50):
        for i in idx:
            P, y = mp.mpf(p[i]), mp.mpf(ref[i])
            for _ in range(100):
                d = (mp.ncdf(y) - P) / mp.npdf(y)
                y -= d
                if abs(d) <= mp.mpf(10) ** -40 * max(1, abs(y)):
                    break
            else:
                raise AssertionError(f"no convergence at p={p[i]!r}")
            out.append(y)
    return idx, out


def ndtri_mp_ratio(got, elementwise=False):
    """|got - mpmath| / bound over ndtri_mpmath()'s points at ndtri_ratio's absolute bounds; elementwise: at 4e-16 max(1, |x|)
    everywhere, the bound that the asymptotic form cannot meet."""
    p = normal_score_points()[0]
    idx, val = ndtri_mpmath()
    ref = np.array([float(v) for v in val])
    tol = 4e-16 * np.maximum(1.0, np.abs(ref)) if elementwise else ndtri_tolerance(p[idx], ref)
    with mp.workdps(50):
        return np.array([float(abs(mp.mpf(got[i]) - v) / mp.mpf(t)) for i, v, t in zip(idx, val, tol)])


def ndtr_ratio(x, got):
    """1e-14 relative."""
    ref = sp.ndtr(x)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    return np.abs(got - ref) / np.maximum(ref, 1e-300) / 1e-14


def erfc_ratio(x, got):
    """1e-14 relative, ndtr's bound: ndtr(x) is erfc(|x| / sqrt 2) / 2 outside the centre, and scipy's erfc is the same Cephes
    routine (only exp's last bit can differ)."""
    ref = sp.erfc(x)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    return np.abs(got - ref) / np.maximum(ref, 1e-300) / 1e-14


def log_ndtr_ratio(x, got):
    """16 ulp; infinities and NaN as scipy's."""
    ref = sp.log_ndtr(x)
    fin = _same_nonfinite(got, ref)
    r = np.full(x.shape, np.nan)
    r[fin] = np.abs(got[fin] - ref[fin]) / np.spacing(np.abs(ref[fin])) / 16.0
    return r


def erfcx_ratio(y, got):
    """16 eps relative against scipy.special.erfcx (the Faddeeva package): log_ndtr's branch x < -1 is log(erfcx_pos / 2) - t^2
    with |log_ndtr| >= 1.8 there, so the 16 ulp held for log_ndtr are at least 16 eps relative in erfcx_pos."""
    ref = sp.erfcx(y)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    r = np.full(y.shape, np.nan)
    r[ok] = np.abs(got[ok] - ref[ok]) / np.maximum(ref[ok], 1e-300) / (16 * EPS)
    return r


def ndtri_exp_ratio(y, got):
    """The ppf model with the log-mass term set to 1: 4 eps (max(1, |x|) + c(x)), c = Phi(x) / phi(x) = dx/dy -- y carries eps
    absolutely.  Above the expm1 switch the function evaluates -ndtri(p) on p = -expm1(y), which carries eps relatively:
    dx = eps p / phi(x), so c = Phi(-x) / phi(x) there (<= 0.45; the other form would allow anything as y -> 0).
    Infinities and NaN as scipy's."""
    with np.errstate(all="ignore"):
        ref = sp.ndtri_exp(y)
        fin = _same_nonfinite(got, ref)
        c = np.exp(np.where(y > Y_EXPM1, sp.log_ndtr(-ref), sp.log_ndtr(ref)) - st.norm.logpdf(ref))
        c = np.where(np.isfinite(c), c, 0.0)               # |x| > 1e150: phi underflows, c(x) ~ 1 / |x| is nothing beside |x|
        tol = 4 * EPS * (np.maximum(1.0, np.abs(ref)) + c)
    r = np.full(y.shape, np.nan)
    r[fin] = np.abs(got[fin] - ref[fin]) / tol[fin]
    return r


def ppf_model(q, a, b, ref):
    """(tolerance, kept) of test_truncnorm_ppf_equals_scipy: 4 eps (max(1, |x|) + (1 + |log Phi(far bound)|) c(x)); left out where
    Phi(x) rounds to 1 in scipy's left branch (eps c(x) > 1e-6).  Where the far bound is infinite its log-CDF is -inf and adds
    nothing to log_sum, so its term is 0 there (the ndtri_exp model) -- not the infinity the formula would give, which would
    let any finite value pass."""
    with np.errstate(all="ignore"):
        left = a < 0
        c = np.where(left, np.exp(sp.log_ndtr(ref) - st.norm.logpdf(ref)), np.exp(sp.log_ndtr(-ref) - st.norm.logpdf(ref)))
        far = np.where(left, sp.log_ndtr(a), sp.log_ndtr(-b))
        y = 1.0 + np.where(np.isneginf(far), 0.0, np.abs(far))
        tol = 4 * EPS * (np.maximum(1.0, np.abs(ref)) + y * c)
        keep = np.isfinite(ref) & ~(left & (EPS * c > 1e-6))
    assert np.all(np.isfinite(tol[keep]) & (tol[keep] > 0))
    return tol, keep


@functools.lru_cache(maxsize=None)
def ppf_scipy(region):
    q, a, b = ppf_points(region)
    with np.errstate(all="ignore"):
        ref = st.truncnorm.ppf(q, a, b)
    return ref, *ppf_model(q, a, b, ref)


def ppf_ratio(region, got):
    """Against scipy at the model bound; infinities where scipy returns them (q = 0 / 1 at an infinite bound; not scipy's inf /
    nan for q near 1 below a finite b); NaN arguments give NaN."""
    q, a, b = ppf_points(region)
    ref, tol, keep = ppf_scipy(region)
    nan_in = np.isnan(q) | np.isnan(a) | np.isnan(b)
    assert np.all(np.isnan(got[nan_in])) and np.all(np.isnan(ref[nan_in]))
    nf = ~np.isfinite(ref) & ~((a < 0) & np.isfinite(b) & (q > 0.5))
    np.testing.assert_array_equal(got[nf], ref[nf])
    r = np.full(q.shape, np.nan)
    r[keep] = np.abs(got[keep] - ref[keep]) / tol[keep]
    r[keep & ~np.isfinite(got)] = np.inf
    return r


def log_gauss_mass_ratio(a, b, got):
    """16 eps (1 + |p|) exp(p - m) against scipy's _log_gauss_mass m, p the larger of the two log-CDFs that are subtracted (0 in
    the central case): each carries log_ndtr's 16 ulp, which is 16 eps |p| relative in P = exp(p), and the difference P - Q
    amplifies a relative error of P by P / (P - Q) = exp(p - m)."""
    from scipy.stats._continuous_distns import _log_gauss_mass       # private: imported where it is needed
    with np.errstate(all="ignore"):
        ref = _log_gauss_mass(a, b)
        p = np.where(b <= 0, sp.log_ndtr(b), np.where(a > 0, sp.log_ndtr(-a), 0.0))
        tol = 16 * EPS * (1.0 + np.abs(p)) * np.exp(p - ref)
    fin = np.isfinite(ref) & np.isfinite(tol)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    r = np.full(a.shape, np.nan)
    r[fin] = np.abs(got[fin] - ref[fin]) / tol[fin]
    r[fin & ~np.isfinite(got)] = np.inf
    return r


# ---- truncnorm.ppf against mpmath ---------------------------------------------------------------------------------------------
def _ppf_mp(q, a, b, x0):
    """Phi^-1(Phi(a) + q (Phi(b) - Phi(a))) (a < 0) or -Phi^-1(Phi(-b) + (1 - q) (Phi(-a) - Phi(-b))) (a >= 0) by Newton's
    iteration on Phi(y) = p from scipy's value."""
    Q, A, B = mp.mpf(q), mp.mpf(a), mp.mpf(b)
    if a < 0:
        p, y, sign = mp.ncdf(A) + Q * (mp.ncdf(B) - mp.ncdf(A)), mp.mpf(x0), 1
    else:
        p, y, sign = mp.ncdf(-B) + (1 - Q) * (mp.ncdf(-A) - mp.ncdf(-B)), -mp.mpf(x0), -1
    for _ in range(100):
        d = (mp.ncdf(y) - p) / mp.npdf(y)
        y -= d
        if abs(d) <= mp.mpf(10) ** -55 * max(1, abs(y)):
            return sign * y
    raise AssertionError(f"no convergence at q={q!r} a={a!r} b={b!r}")


@functools.lru_cache(maxsize=None)
def ppf_mpmath(region):
    """(indices, mpmath values) of the regime's kept points among mp_subset(region)."""
    q, a, b = ppf_points(region)
    ref, _, keep = ppf_scipy(region)
    idx = np.array([i for i in mp_subset(region) if keep[i]])
    with mp.workdps(70):
        return idx, [_ppf_mp(q[i], a[i], b[i], ref[i]) for i in idx]


def ppf_mp_ratio(region, got):
    """(|got - mpmath| / model bound over the kept points of the subset, share of the subset that is kept -- among the points where
    scipy is finite, i.e. what the exclusion rule alone removes)."""
    ref, tol, keep = ppf_scipy(region)
    idx, val = ppf_mpmath(region)
    sub = mp_subset(region)
    with mp.workdps(70):
        r = np.array([float(abs(mp.mpf(got[i]) - v) / mp.mpf(tol[i])) if np.isfinite(got[i]) else np.inf for i, v in zip(idx, val)])
    return r, idx.size / max(1, int(np.isfinite(ref[sub]).sum()))


# ---- local_cov_of against mpmath ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def local_cov_reference(vtype):
    """Per element (kind, reference, bound) on the doubles (h2, c0, sill), h = sqrt(h2) in mpmath:
      kind 0  |got - ref| <= bound: exponential / Gaussian 4 eps (1 + |t|) |ref|, t = -3 h / -3 h^2 >= -700 (one rounding per
              operation, and the roundings of t, which exp turns into a relative error |t| eps each); spherical inside the
              range 4 eps (|c0| + 1.5 h + 0.5 h^3)
      kind 1  got == ref exactly: spherical beyond the range, sill - 1 (the branch is taken on the double sqrt(h2), as the
              function takes it; IEEE sqrt is the same on both sides)
      kind 2  0 <= got <= c0 * 1e-300: t < -700."""
    h2, c0, sill = local_cov_points()
    kind, ref, bound = np.zeros(h2.size, int), np.zeros(h2.size), np.zeros(h2.size)
    with mp.workdps(60):
        for i in range(h2.size):
            h = mp.sqrt(mp.mpf(h2[i]))
            if vtype == 2:
                if np.sqrt(h2[i]) > 1.0:
                    kind[i], ref[i] = 1, sill[i] - 1.0
                else:
                    ref[i] = float(mp.mpf(c0[i]) - 1.5 * h + 0.5 * h ** 3)
                    bound[i] = 4 * EPS * float(abs(c0[i]) + 1.5 * h + 0.5 * h ** 3)
                continue
            t = -3 * h if vtype == 0 else -3 * h * h
            if t < -700:
                kind[i], bound[i] = 2, c0[i] * 1e-300
            else:
                v = mp.mpf(c0[i]) * mp.exp(t)
                ref[i], bound[i] = float(v), 4 * EPS * float((1 + abs(t)) * v)
    return kind, ref, bound


def local_cov_ratio(vtype, got):
    """|error| / bound where a bound applies (kind 0), after asserting kinds 1 and 2."""
    kind, ref, bound = local_cov_reference(vtype)
    np.testing.assert_array_equal(got[kind == 1], ref[kind == 1])
    under = got[kind == 2]
    assert np.all((under >= 0.0) & (under <= bound[kind == 2]))
    k0 = kind == 0
    r = np.full(got.shape, np.nan)
    assert np.all(bound[k0] > 0)
    r[k0] = np.abs(got[k0] - ref[k0]) / bound[k0]
    r[k0 & ~np.isfinite(got)] = np.inf
    return r


def local_cov_numpy(vtype):
    """local_cov_of operation for operation in IEEE doubles (NumPy): what the bounds promise of any build that rounds once per
    operation and has an exp good to an ulp."""
    h2, c0, sill = local_cov_points()
    with np.errstate(all="ignore"):
        h = np.sqrt(h2)
        if vtype == 0:
            return c0 * np.exp(-3.0 * h)
        if vtype == 1:
            return c0 * np.exp(-3.0 * (h * h))
        return np.where(h > 1.0, sill - 1.0, c0 - 1.5 * h + 0.5 * (h * h * h))
