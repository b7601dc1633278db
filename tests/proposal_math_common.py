"""Constructed arguments, truth and bars for the scalar arithmetic of the Philox proposal path (csrc/proposal_device.h, csrc/math_tables.h,
csrc/philox.h): shared by tests/test_proposal_math_host.py (a g++ restatement: shows that the bars are fair) and
tests/test_gpu_proposal_math.py (gsm_debug_proposal_math: the device compile, the math table read from LDS).

Truth is mpmath at 160 bits on the exact input doubles / words.  Every *_ratio function returns |error| / bar per point (inf where an
exact requirement is missed); a test asserts max <= 1.  No bar is tuned on a device:

  log_tab       3e-16 + 2.5e-16 |log x|                         math_tables.h
  sincos_tab    3e-16 absolute                                  math_tables.h
  sqrt_lean     1 ulp of the true root; arguments <= 1e-300 give exactly sqrt(1e-300) (correctly rounded)      proposal_device.h
  exp_lean      relative EXP_REL = 1.7e-16 + 3 * 2^-53 = 5.03e-16 where the true value is normal: the Taylor truncation at |r| = ln 2 / 2
                plus the rounding of r and of the last two fmas; the same plus one subnormal spacing 2^-1074 absolute below 2^-1022;
                exactly 0 for x <= -746
  normals       5e-15 absolute (the bar of test_gpu_philox.test_device_normals_match_oracle) wherever the radius uniform u < 1; at u == 1
                every component has |g| <= 1e-149 (sqrt_lean's 1e-150 stand-in for a radius of 0)
  spectral_amp  relative EXP_REL + |dx| (+ 2^-1074 absolute where the amplitude is subnormal), dx = first-order error of the exponent
                argument x as the device forms it, eps = 2^-53, LOG(L) = 3e-16 + 2.5e-16 |L| the bar of log_tab:
                  Gaussian     x = -0.25 ((aa aa) k2): three roundings                                            dx = 3 eps |x|
                  Exponential  x = -0.75 L, L = log_tab(1 + (aa aa) k2): the logarithm's error, two roundings of its argument (relative
                               to an argument >= 1, so absolute in L) and the rounding of the product
                                                                                      dx = 0.75 (LOG(L) + 2 eps) + eps |x|
                  Matern       x = fma(-(nu + 1) / 2, L, m_const), L = log_tab(m_kappa + (4 M_PI) k2): likewise with (nu + 1) / 2 for 0.75,
                               and the fma's rounding at the size of its larger term           dx = (nu + 1) / 2 (LOG(L) + 2 eps) + eps |x| + eps |m_const|
                The truth uses the double M_PI in 4 M_PI k2, as the function is defined.
  philox_draw   bit for bit
"""
import functools
import math

import mpmath
import numpy as np

import philox_oracle as po

PREC = 160
EPS = 2.0 ** -53
EXP_REL = 1.7e-16 + 3 * EPS
TINY = mpmath.mpf(2) ** -1074
MIN_NORMAL = mpmath.mpf(2) ** -1022
PHILOX, LOG_TAB, SINCOS_TAB, SQRT_LEAN, EXP_LEAN, NORMALS4_WORDS, NORMALS2_WORDS, SPECTRAL_AMP = range(8)    # GSM_PMATH_* (include/gsm.h)
GAUSSIAN, EXPONENTIAL, MATERN = 0, 1, 2                                                                       # GSM_MODEL_*

# radius words of normals4 (u = (w + 1) 2^-32: w = 2^32 - 1 gives u == 1) and the same places of normals2's 53-bit layout
RADIUS_WORDS = [0, 1, 2, 3, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 3, 2 ** 32 - 2, 2 ** 32 - 1]
RADIUS_INTS53 = [0, 1, 2, 3, 2 ** 52 - 1, 2 ** 52, 2 ** 53 - 3, 2 ** 53 - 2, 2 ** 53 - 1]


def _mpf(x):
    return mpmath.mpf(float(x))


def _ratios(got, truth, bar):
    """|got - truth| / bar per point; got: doubles, truth / bar: mpf lists.  A non-finite value counts as inf."""
    out = np.empty(len(truth))
    with mpmath.workprec(PREC):
        for i, (g, t, b) in enumerate(zip(np.asarray(got, dtype=np.float64).ravel(), truth, bar)):
            out[i] = float(abs(_mpf(g) - t) / b) if math.isfinite(g) else math.inf
    return out


# ---- spectral_amp: arguments (first: log_tab takes its k = 0 and Nyquist arguments from here) -------------------------------------------
def k2_table(bh, bw, res):
    """[bh / 2 + 1][bw / 2 + 1] values (sqrt(kx^2 + ky^2) + 1e-10)^2 as k2_table_kernel forms them."""
    def wn(n):
        k = np.arange(n // 2 + 1)
        kk = np.where(k < (n + 1) // 2, k, k - n).astype(np.float64)
        return (kk * (1.0 / (n * res))) * 2.0 * math.pi
    k = np.sqrt(wn(bw)[None, :] ** 2 + wn(bh)[:, None] ** 2) + 1e-10
    return k * k


def _aa(model, rx, ry):
    d = math.sqrt(3.0) if model == GAUSSIAN else (3.0 if model == EXPONENTIAL else 2.0)
    return math.sqrt((rx / d) * (ry / d))


MATERN_NU = (0.5, 0.9125, 1.0, 2.5)


@functools.lru_cache(maxsize=None)
def spectral_points(model, nu=0.0):
    """(aa, m_kappa, m_const, k2) arrays: ranges 10 .. 50 km at 500 m cells, k2 = the DC entry (1e-20), the first non-DC entry and the
    Nyquist corner of the 2 x 2, 2 x 12 and 50 x 80 tables; and the extremes: 50 km on the 50 x 80 table (Gaussian: x = -2.5e4) and 500 km
    at 10 m cells (Gaussian: x = -4e9, k = rint(x / ln 2) beyond -2^31)."""
    rows = []
    cases = [(500.0, (rx, ry)) for rx, ry in ((10e3, 10e3), (30e3, 30e3), (50e3, 50e3), (10e3, 50e3), (23456.7, 41234.5))] + [(10.0, (500e3, 500e3))]
    for res, (rx, ry) in cases:
        aa = _aa(model, rx, ry)
        kappa = const = 0.0
        if model == MATERN:
            n = nu if nu != 0.0 else 1.0
            const = 0.5 * math.log((4.0 * math.pi * math.gamma(n + 1.0) * (2.0 * n) ** n) / (math.gamma(n) * aa ** (2.0 * n)))
            kappa = 2.0 * n / (aa * aa)
        for bh, bw in ((2, 2), (2, 12), (50, 80)):
            t = k2_table(bh, bw, res).ravel()
            for k2 in (t[0], t[1], t[-1]):
                rows.append((aa, kappa, const, float(k2)))
    a = np.array(rows, dtype=np.float64)
    return tuple(np.ascontiguousarray(a[:, j]) for j in range(4))


def _spectral_x(model, nu, aa, kappa, const, k2):
    """(true exponent argument x on these doubles, its logarithm L or None) in mpf"""
    aa, kappa, const, k2 = _mpf(aa), _mpf(kappa), _mpf(const), _mpf(k2)
    if model == GAUSSIAN:
        return -aa * aa * k2 / 4, None
    if model == EXPONENTIAL:
        L = mpmath.log(1 + aa * aa * k2)
        return -0.75 * L, L
    n = _mpf(nu if nu != 0.0 else 1.0)
    L = mpmath.log(kappa + _mpf(4.0 * math.pi) * k2)
    return const - (n + 1) / 2 * L, L


@functools.lru_cache(maxsize=None)
def spectral_truth(model, nu=0.0):
    """(true amplitudes, bars) as mpf lists"""
    truth, bar = [], []
    with mpmath.workprec(PREC):
        for aa, kappa, const, k2 in zip(*spectral_points(model, nu)):
            x, L = _spectral_x(model, nu, aa, kappa, const, k2)
            if model == GAUSSIAN:
                dx = 3 * EPS * abs(x)
            else:
                f = mpmath.mpf(0.75) if model == EXPONENTIAL else (_mpf(nu if nu != 0.0 else 1.0) + 1) / 2
                dx = f * (3e-16 + 2.5e-16 * abs(L) + 2 * EPS) + EPS * abs(x) + (EPS * abs(_mpf(const)) if model == MATERN else 0)
            t = mpmath.exp(x)
            truth.append(t)
            bar.append((EXP_REL + dx) * t + (TINY if t < MIN_NORMAL else 0))
    return truth, bar


def spectral_ratio(model, nu, got):
    return _ratios(got, *spectral_truth(model, nu))


# ---- log_tab ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def log_points():
    """Every boundary of the 128 mantissa intervals +- 2 ulp for exponents -53 .. 40; the radius uniforms of RADIUS_WORDS; 1 - j 2^-53,
    j = 0 .. 64; the arguments 1 + aa^2 k2 and m_kappa + 4 pi k2 of spectral_amp at k = 0 (k2 = 1e-20), the first entry and Nyquist."""
    e = np.arange(-53, 41, dtype=np.int64)[:, None, None]
    i = np.arange(128, dtype=np.int64)[None, :, None]
    d = np.arange(-2, 3, dtype=np.int64)[None, None, :]
    b = (((e + 1023) << 52) | (i << 45)) + d
    xs = [b.ravel().view(np.float64)]
    xs.append((np.array(RADIUS_WORDS, dtype=np.float64) + 1.0) * 2.0 ** -32)
    xs.append(1.0 - np.arange(65, dtype=np.float64) * 2.0 ** -53)
    aa, _, _, k2 = spectral_points(EXPONENTIAL)
    xs.append(1.0 + (aa * aa) * k2)
    for nu in MATERN_NU:
        _, kappa, _, k2 = spectral_points(MATERN, nu)
        xs.append(kappa + 4.0 * math.pi * k2)
    return np.ascontiguousarray(np.concatenate(xs))


def log_interval(x):
    """(exponent, top seven mantissa bits) as log_tab splits its argument"""
    b = np.asarray(x, dtype=np.float64).view(np.int64)
    return (b >> 52) - 1023, (b >> 45) & 127


@functools.lru_cache(maxsize=None)
def log_truth():
    with mpmath.workprec(PREC):
        t = [mpmath.log(_mpf(x)) for x in log_points()]
        return t, [3e-16 + 2.5e-16 * abs(v) for v in t]


def log_ratio(got):
    return _ratios(got, *log_truth())


# ---- sincos_tab -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sincos_points():
    """Every table node j / 64 and every rint tie (j + 1/2) / 64 with the neighbours at 1, 2, 3 steps of 2^-32 and of 2^-53 on either side;
    0, 1 - 2^-32, 1 - 2^-53.  (Below 1/2 the doubles are finer than 2^-53: every point is exact.)"""
    base = np.arange(128, dtype=np.float64) / 128.0
    steps = np.array([0.0] + [s * m * h for h in (2.0 ** -32, 2.0 ** -53) for m in (1, 2, 3) for s in (1, -1)])
    u = (base[:, None] + steps[None, :]).ravel()
    u = np.concatenate([u, [0.0, 1.0 - 2.0 ** -32, 1.0 - 2.0 ** -53]])
    return np.ascontiguousarray(u[(u >= 0.0) & (u < 1.0)])


@functools.lru_cache(maxsize=None)
def sincos_truth():
    t = []
    with mpmath.workprec(PREC):
        for u in sincos_points():
            a = 2 * mpmath.pi * _mpf(u)
            t += [mpmath.sin(a), mpmath.cos(a)]
    return t, [mpmath.mpf(3e-16)] * len(t)


def sincos_ratio(got):
    """got: [n, 2] = (sin, cos)"""
    return _ratios(got, *sincos_truth())


# ---- sqrt_lean --------------------------------------------------------------------------------------------------------------------------
SQRT_FLOOR = 1e-300


@functools.lru_cache(maxsize=None)
def sqrt_points():
    """0, -0, arguments below the floor, 1e-300, 2.4e-17 (-2 log_tab(1) before the table's log c_0 was nudged), exact squares, -2 log u of the radius
    words, a geometric sweep, 73.5 (the largest -2 log u), 2^499 (the stated limit is 2^500)."""
    t = [0.0, -0.0, 5e-324, 1e-310, 1e-301, 1e-300, 2.4e-17, 73.5, 2.0 ** 499]
    t += [float(k * k) for k in range(1, 65)] + [4.0 ** m for m in range(-60, 240, 13)]
    with mpmath.workprec(PREC):
        for w in RADIUS_WORDS[:-1]:
            t.append(float(-2 * mpmath.log(mpmath.mpf(w + 1) / 2 ** 32)))
        for m in RADIUS_INTS53[:-1]:
            t.append(float(-2 * mpmath.log(mpmath.mpf(m + 1) / 2 ** 53)))
    t += list(10.0 ** (np.arange(400) * (440.0 / 400) - 289.877))
    return np.array(t, dtype=np.float64)


def sqrt_ratio(got):
    """|got - sqrt(t)| / ulp(sqrt(t)); arguments <= 1e-300: 0 if got is exactly the correctly rounded sqrt(1e-300), else inf"""
    t = sqrt_points()
    got = np.asarray(got, dtype=np.float64)
    out = np.empty(t.size)
    with mpmath.workprec(PREC):
        floor = float(mpmath.sqrt(_mpf(SQRT_FLOOR)))
        for i, (x, g) in enumerate(zip(t, got)):
            if x <= SQRT_FLOOR:
                out[i] = 0.0 if g == floor else math.inf
            else:
                r = mpmath.sqrt(_mpf(x))
                out[i] = float(abs(_mpf(g) - r) / _mpf(np.spacing(float(r)))) if math.isfinite(g) else math.inf
    return out


# ---- exp_lean ---------------------------------------------------------------------------------------------------------------------------
EXP_ZERO_BELOW = -746.0


@functools.lru_cache(maxsize=None)
def exp_points():
    """0 and +- tiny arguments; both sides of every reduction tie (k + 1/2) ln 2, k = -1021 .. 1009, at one ulp and at 5e-10; 2048 points of
    [-708, 0]; 512 of the subnormal range [-745.2, -708]; the zero results -746, -2.5e4, -2.2e9 (k beyond -2^31), -1e300."""
    x = [0.0, -0.0, 5e-324, -5e-324, 1e-300, -1e-300, 2.0 ** -53, -2.0 ** -53, 1e-20, -1e-20, 1e-9, -1e-9]
    with mpmath.workprec(PREC):
        ties = np.array([float((k + mpmath.mpf(0.5)) * mpmath.ln2) for k in range(-1021, 1010)])
    x += list(np.nextafter(ties, np.inf)) + list(np.nextafter(ties, -np.inf)) + list(ties + 5e-10) + list(ties - 5e-10)
    x += list(-708.0 * ((np.arange(2048) + 0.381966) / 2048.0))
    x += list(-708.0 - 37.2 * ((np.arange(512) + 0.618034) / 512.0))
    x += [EXP_ZERO_BELOW, -2.5e4, -2.2e9, -1e300]
    return np.array(x, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def exp_truth():
    truth, bar = [], []
    with mpmath.workprec(PREC):
        for x in exp_points():
            t = mpmath.exp(_mpf(x))
            truth.append(t)
            bar.append(EXP_REL * t + (TINY if t < MIN_NORMAL else 0))
    return truth, bar


def exp_ratio(got):
    r = _ratios(got, *exp_truth())
    z = exp_points() <= EXP_ZERO_BELOW
    r[z] = np.where(np.asarray(got, dtype=np.float64)[z] == 0.0, 0.0, math.inf)
    return r


# ---- normals4 / normals2 on words ----------------------------------------------------------------------------------------------------
def _angle_ints(bits):
    """nodes j / 64 and ties (j + 1/2) / 64 of a `bits`-bit angle integer, each with its neighbours at +- 1, 2 (modulo 2^bits)"""
    a = (np.arange(128, dtype=np.int64) << (bits - 7))[:, None] + np.arange(-2, 3, dtype=np.int64)[None, :]
    return a.ravel() & ((1 << bits) - 1)


@functools.lru_cache(maxsize=None)
def normals4_points():
    """[n, 4] uint32 blocks: the cross product of RADIUS_WORDS with the angle words on nodes, ties and +- 2 around them, in (x, y); (z, w)
    holds the same product in another order.  (u, angle) = ((x + 1) 2^-32, y 2^-32), ((z + 1) 2^-32, w 2^-32)."""
    ang = _angle_ints(32)
    r = np.array(RADIUS_WORDS, dtype=np.int64)
    x, y = [v.ravel() for v in np.meshgrid(r, ang, indexing="ij")]
    z, w = np.roll(r, 4)[np.searchsorted(r, x)], np.roll(y, 321)
    return np.ascontiguousarray(np.stack([x, y, z, w], axis=1).astype(np.uint32))


@functools.lru_cache(maxsize=None)
def normals2_points():
    """[n, 4] uint32 blocks of the 53-bit layout, u = (((y << 32 | x) >> 11) + 1) 2^-53, angle = ((w << 32 | z) >> 11) 2^-53: the same cross
    product; the eleven discarded low bits are set to a pattern."""
    ang = _angle_ints(53)
    r = np.array(RADIUS_INTS53, dtype=np.int64)
    m, a = [v.ravel() for v in np.meshgrid(r, ang, indexing="ij")]
    v1, v2 = (m.astype(np.uint64) << np.uint64(11)) | np.uint64(0x5A5), (a.astype(np.uint64) << np.uint64(11)) | np.uint64(0x2D2)
    lo, hi = np.uint64(0xFFFFFFFF), np.uint64(32)
    return np.ascontiguousarray(np.stack([v1 & lo, v1 >> hi, v2 & lo, v2 >> hi], axis=1).astype(np.uint32))


def _pairs(layout):
    """(numerator of u, numerator of the angle, bits) of every Box-Muller pair, in the order of the output array"""
    if layout == 4:
        p = normals4_points().astype(np.int64)
        return [(int(a) + 1, int(b), 32) for row in p for a, b in ((row[0], row[1]), (row[2], row[3]))]
    p = normals2_points().astype(np.uint64)
    v1, v2 = (p[:, 1] << np.uint64(32)) | p[:, 0], (p[:, 3] << np.uint64(32)) | p[:, 2]
    return [(int(a >> np.uint64(11)) + 1, int(b >> np.uint64(11)), 53) for a, b in zip(v1, v2)]


def radius_is_one(layout):
    """per pair: u == 1"""
    return np.array([nu == 1 << bits for nu, _, bits in _pairs(layout)])


@functools.lru_cache(maxsize=None)
def normals_truth(layout):
    """(g_cos, g_sin) per pair, flattened in the order of the output array"""
    t = []
    with mpmath.workprec(PREC):
        for nu, na, bits in _pairs(layout):
            rad = mpmath.sqrt(-2 * mpmath.log(mpmath.mpf(nu) / 2 ** bits))
            a = 2 * mpmath.pi * mpmath.mpf(na) / 2 ** bits
            t += [rad * mpmath.cos(a), rad * mpmath.sin(a)]
    return t


def normals_ratio(layout, got):
    """got: [n, 4] (layout 4) or [n, 2] (layout 2).  |error| / 5e-15 where u < 1; at u == 1: 0 if |g| <= 1e-149, else |g| / 1e-149"""
    t = normals_truth(layout)
    r = _ratios(got, t, [mpmath.mpf(5e-15)] * len(t)).reshape(-1, 2)
    one = radius_is_one(layout)
    g = np.abs(np.asarray(got, dtype=np.float64).reshape(-1, 2)[one])
    r[one] = np.where(g <= 1e-149, 0.0, g / 1e-149)
    return r.ravel()


# ---- philox_draw ------------------------------------------------------------------------------------------------------------------------
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),                 # Random123 kat_vectors, philox4x32-10
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),  # (as tests/test_host_api.py holds them)
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@functools.lru_cache(maxsize=None)
def philox_points():
    """([n, 6] uint32 rows (seed lo, seed hi, step lo, step hi, stream, idx), [n, 4] expected words): the known-answer vectors (counter =
    (idx, stream, step lo, step hi), key = seed), then counters with idx = 2^32 - 1, steps >= 2^32, negative steps and seeds with the high
    word set, expected from oracle/philox_oracle.draw (which the same vectors pin)."""
    rows = [(k[0], k[1], c[2], c[3], c[1], c[0]) for c, k, _ in KAT]
    exp = [e for _, _, e in KAT]
    for seed in (7, 2 ** 40 + 12345, 2 ** 63 + 99, 2 ** 64 - 1):
        for step in (0, 10 ** 9 + 7, 2 ** 32, 2 ** 32 + 5, 2 ** 45 + 3, -1, -(2 ** 33) - 17):
            for stream in (0, 1, 2, 3):
                for idx in (0, 1, 4000000000, 2 ** 32 - 1):
                    s = step & (2 ** 64 - 1)
                    rows.append((seed & 0xFFFFFFFF, seed >> 32, s & 0xFFFFFFFF, s >> 32, stream, idx))
                    exp.append(tuple(int(v) for v in po.draw(seed, s, stream, np.array(idx))))
    return np.array(rows, dtype=np.uint32), np.array(exp, dtype=np.uint32)
