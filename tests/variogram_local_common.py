"""NumPy checker of the local variogram maps (gsm_variogram_local, mcmc_gpu_amd.variogram.local_variogram_map), independent of
the kernel: per offset the difference field, the midpoint tile of every pair from the rule
    ti = (2 i + di) // (2 T),  tj = (2 j + dj) // (2 T),
math.fsum per (tile, offset), and windows by summing tiles.  Also the two-regime field of the end-to-end tests and the bar that
the device's fits are held to.  Shared by tests/test_variogram_local_host.py (CPU) and tests/test_gpu_variogram_local.py; every
case, table and bar is made once per process."""
import functools
import math

import numpy as np

U = 2.0 ** -53

# tag: (H, W, T, ks, mi, mj, R) -- what each exercises is in tests/test_gpu_variogram_local.py
CASES = {
    "ragged": (37, 70, 8, (0, 1), 9, 40, 3),
    "odd": (23, 19, 5, (2,), 22, 18, 2),
    "one": (24, 20, 64, (0,), 8, 8, 3),
    "thin": (4, 260, 16, (1,), 3, 100, 2),
    "tile2": (12, 12, 2, (1,), 5, 5, 2),
    "lines": (48, 48, 16, (0, 1), 10, 10, 2),
}
RUNS = [(tag, k) for tag, c in CASES.items() for k in c[3]]


@functools.lru_cache(maxsize=None)
def case(tag):
    """(fields [R, H, W], mask [H, W] bool or None): values N(300, 50), 30 % of the cells NaN, drawn independently per field.
    'lines': values on every 6th row and on three columns only, and a mask that removes a rectangle."""
    H, W, _, _, _, _, R = CASES[tag]
    rng = np.random.default_rng(sorted(CASES).index(tag) + 177)
    f = rng.normal(300.0, 50.0, (R, H, W))
    mask = None
    if tag == "lines":
        keep = np.zeros((H, W), dtype=bool)
        keep[::6, :] = True
        keep[:, [5, 20, 41]] = True
        f[:, ~keep] = np.nan
        mask = np.ones((H, W), dtype=bool)
        mask[10:31, 15:26] = False
    else:
        f[rng.random((R, H, W)) < 0.3] = np.nan
    f.setflags(write=False)
    return f, mask


def lattice(H, W, T):
    return -(-H // T), -(-W // T)


def tile_tables(z, mi, mj, T, mask=None):
    """(sum, count) [Ty, Tx, mi + 1, 2 mj + 1] of one field: every pair of the half plane in the tile of its midpoint."""
    H, W = z.shape
    Ty, Tx = lattice(H, W, T)
    z = np.where(np.isfinite(z), z, np.nan)
    if mask is not None:
        z = np.where(np.asarray(mask) != 0, z, np.nan)
    S = np.zeros((Ty, Tx, mi + 1, 2 * mj + 1))
    C = np.zeros(S.shape, dtype=np.int64)
    for di in range(min(mi, H - 1) + 1):
        for dj in range(-min(mj, W - 1), min(mj, W - 1) + 1):
            if di == 0 and dj <= 0:
                continue
            i = np.arange(H - di)[:, None]
            j = np.arange(max(0, -dj), min(W, W - dj))[None, :]
            d = z[i, j] - z[i + di, j + dj]
            ok = np.isfinite(d)
            tile = np.broadcast_to((2 * i + di) // (2 * T) * Tx + (2 * j + dj) // (2 * T), d.shape)[ok]
            sq = (d * d)[ok]
            order = np.argsort(tile, kind="stable")
            tile, sq = tile[order], sq[order]
            cuts = np.flatnonzero(np.diff(tile)) + 1
            for t, terms in zip(tile[np.concatenate([[0], cuts])] if tile.size else [], np.split(sq, cuts)):
                S[t // Tx, t % Tx, di, dj + mj] = math.fsum(terms)
                C[t // Tx, t % Tx, di, dj + mj] = terms.size
    return S, C


def windows(S, C, k):
    """Window tables from tile tables: the (2 k + 1)^2 tiles centred on each tile, clipped at the lattice's edge."""
    if k == 0:
        return S, C
    Ty, Tx = S.shape[:2]
    WS, WC = np.zeros_like(S), np.zeros_like(C)
    for a in range(Ty):
        for b in range(Tx):
            sl = (slice(max(0, a - k), min(Ty, a + k + 1)), slice(max(0, b - k), min(Tx, b + k + 1)))
            part = S[sl].reshape((-1,) + S.shape[2:])
            WS[a, b] = np.array([math.fsum(col) for col in part.reshape(part.shape[0], -1).T]).reshape(S.shape[2:])
            WC[a, b] = C[sl].sum(axis=(0, 1))
    return WS, WC


@functools.lru_cache(maxsize=None)
def tiles_of(tag):
    """Per field of a case: the checker's tile tables, ([R, Ty, Tx, mi + 1, 2 mj + 1] sum, count)."""
    _, _, T, _, mi, mj, _ = CASES[tag]
    f, mask = case(tag)
    out = [tile_tables(z, mi, mj, T, mask) for z in f]
    return np.array([s for s, _ in out]), np.array([c for _, c in out])


@functools.lru_cache(maxsize=None)
def reference(tag, k):
    """Per field of a case: the checker's window tables at half window k."""
    S, C = tiles_of(tag)
    out = [windows(s, c, k) for s, c in zip(S, C)]
    return np.array([s for s, _ in out]), np.array([c for _, c in out])


# ---- the two-regime field and the bar of the end-to-end test ----------------------------------------------------------------------

TWO = dict(n=128, dx=500.0, T=16, k=1, m=10, major=9000.0, minor=3000.0, az=(30.0, 120.0), seeds=(1, 2), vtype="exponential")


def _exponential_field(n, major, minor, az, dx, seed):
    """A standardised n x n Gaussian field with an exponential covariance exp(-3 h') of practical ranges major / minor along /
    across azimuth az (degrees counter-clockwise from +x, y ascending with the row): white noise on a 2 n periodic lattice
    filtered with the square root of the 2-D spectrum (1 + |k'|^2)^(-3/2), one quadrant kept."""
    rng = np.random.default_rng(seed)
    N = 2 * n
    k = 2.0 * np.pi * np.fft.fftfreq(N, d=dx)
    kx, ky = np.meshgrid(k, k)
    th = np.radians(az)
    ku = (kx * np.cos(th) + ky * np.sin(th)) * (major / 3.0)
    kv = (-kx * np.sin(th) + ky * np.cos(th)) * (minor / 3.0)
    amp = (1.0 + ku * ku + kv * kv) ** -0.75
    f = np.fft.ifft2(np.fft.fft2(rng.normal(size=(N, N))) * amp).real[:n, :n]
    return (f - f.mean()) / f.std()


@functools.lru_cache(maxsize=None)
def two_regime():
    """(xx, yy, field [128, 128]): azimuth 30 degrees in the left half, 120 in the right, 9 km / 3 km, joined at the middle column."""
    n, dx = TWO["n"], TWO["dx"]
    left = _exponential_field(n, TWO["major"], TWO["minor"], TWO["az"][0], dx, TWO["seeds"][0])
    right = _exponential_field(n, TWO["major"], TWO["minor"], TWO["az"][1], dx, TWO["seeds"][1])
    field = np.where(np.arange(n)[None, :] < n // 2, left, right)
    xx, yy = np.meshgrid(1000.0 + dx * np.arange(n), -2000.0 + dx * np.arange(n))
    for a in (xx, yy, field):
        a.setflags(write=False)
    return xx, yy, field


def local_map(xx, yy, T, k, m, S, C, total=None):
    """A LocalVariogramMap of one field from (window) tables; total: the whole field's (sum, count), default the tables' own sum."""
    from mcmc_gpu_amd import variogram
    from mcmc_gpu_amd.sgs import _axes
    xs, ys, dx, dy = _axes(np.asarray(xx), np.asarray(yy))
    ts, tc = total if total is not None else (S.sum(axis=(0, 1)), C.sum(axis=(0, 1)))
    return variogram._local_result(xs, ys, dx, dy, m[0], m[1], T, k, S[None], C[None], ts[None], tc[None])


@functools.lru_cache(maxsize=None)
def two_regime_tables():
    """The checker's tables of the two-regime field: (tile sum, tile count, window sum, window count, whole sum, whole count)."""
    _, _, field = two_regime()
    S, C = tile_tables(field, TWO["m"], TWO["m"], TWO["T"])
    WS, WC = windows(S, C, TWO["k"])
    flat = S.reshape((-1,) + S.shape[2:])
    whole = np.array([math.fsum(col) for col in flat.reshape(flat.shape[0], -1).T]).reshape(S.shape[2:])
    return S, C, WS, WC, whole, C.sum(axis=(0, 1))


@functools.lru_cache(maxsize=None)
def two_regime_fit():
    """fit_local on the checker's window tables."""
    from mcmc_gpu_amd import variogram
    xx, yy, _ = two_regime()
    _, _, WS, WC, ts, tc = two_regime_tables()
    return variogram.fit_local(local_map(xx, yy, TWO["T"], TWO["k"], (TWO["m"], TWO["m"]), WS, WC, (ts, tc)), TWO["vtype"])


PARAMS = ("major_range", "minor_range", "sill", "azimuth")


def window_change(a, b):
    """Per parameter the [Ty, Tx] relative change between two lattices of window fits; the azimuth in units of 180 degrees, modulo 180."""
    out = {}
    for p in PARAMS:
        x = np.array([[w[p] for w in row] for row in a], dtype=np.float64)
        y = np.array([[w[p] for w in row] for row in b], dtype=np.float64)
        if p == "azimuth":
            out[p] = np.abs((x - y + 90.0) % 180.0 - 90.0) / 180.0
        else:
            out[p] = np.abs(x - y) / np.abs(y)
    return out


AZIMUTH_EXCLUDE = 1e-6            # a window whose azimuth moves by more than this (x 180 degrees) under the perturbation is nearly isotropic


@functools.lru_cache(maxsize=None)
def fairness_bar():
    """The bar of the device's end-to-end test, measured on the checker alone.  The device's tables may differ from the checker's by
    (n + 3) 2^-53 relative per entry, so: perturb the checker's window tables by random signs times that bound (8 draws, fixed
    seed), refit every window, and take the largest relative change of each parameter (of the azimuth in units of 180 degrees)
    over the windows and the draws.  The bar is 4 x that maximum: both sides may be off by the bound, and the fit is not linear.
    Windows whose azimuth moves by more than AZIMUTH_EXCLUDE are left out of the azimuth comparison (and of its bar).
    Returns (bar {parameter: float}, keep_azimuth [Ty, Tx] bool)."""
    from mcmc_gpu_amd import variogram
    xx, yy, _ = two_regime()
    _, _, WS, WC, ts, tc = two_regime_tables()
    base = two_regime_fit()
    rng = np.random.default_rng(2024)
    worst = {p: np.zeros(base.windows.shape) for p in PARAMS}
    for _ in range(8):
        sign = rng.choice([-1.0, 1.0], size=WS.shape)
        sign_t = rng.choice([-1.0, 1.0], size=ts.shape)
        lm = local_map(xx, yy, TWO["T"], TWO["k"], (TWO["m"], TWO["m"]), WS * (1.0 + sign * (WC + 3) * U), WC,
                       (ts * (1.0 + sign_t * (tc + 3) * U), tc))
        fit = variogram.fit_local(lm, TWO["vtype"], _start=base.windows)      # Gauss-Newton from the unperturbed fit: the same stationary point
        assert np.array_equal(fit.fitted, base.fitted)
        for p, ch in window_change(fit.windows, base.windows).items():
            worst[p] = np.maximum(worst[p], ch)
    keep = worst["azimuth"] <= AZIMUTH_EXCLUDE
    bar = {p: 4.0 * float(np.max(worst[p][keep] if p == "azimuth" else worst[p])) for p in PARAMS}
    print("fairness bar (4 x the largest change under the table bound):", bar, "azimuth windows excluded:", int((~keep).sum()))
    return bar, keep
