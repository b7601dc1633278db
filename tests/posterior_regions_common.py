"""Cases, the NumPy restatement and the bounds of the posterior region functionals (gsm_posterior_regions, posterior.py `regions`).

Restatement.  terms() forms every per-cell term in the operation order include/gsm.h fixes (a difference, a compare and a select; a
product and a sum kept apart), in fp64: every term is bit for bit the device's, whatever order the device adds them in.
reference() sums the terms of every chain and region in np.longdouble and counts exactly.

Bound.  Slots 1 .. 3 are sums of m bit-equal fp64 terms t in some fixed tree: any summation order of m terms is within (m - 1) u
sum |t| of the exact sum to first order, u = 2^-53; (m + 3) u sum |t| covers the higher orders for m << 2^26 and the long-double
reference's own rounding (2^-64 relative per addition).  Slots 0, 4, 5 (counts), 6, 7 (min, max) and every hypsometry counter are
exact: asserted equal."""
import functools

import numpy as np

U = 2.0 ** -53
SEA, RHO_ICE, RHO_WATER = 1.5, 917.0, 1028.0          # a sea level that fp32 holds exactly: beds exactly at it exist in both state types
RATIO = RHO_WATER / RHO_ICE
HYPS_LO, HYPS_HI = -512.0, 512.0                      # bin widths 512, 64 and 16 m at 2, 16 and 64 bins: every edge is exact in fp32
BINS = (0, 2, 16, 64)
GRIDS = ((37, 53), (64, 130), (3, 257))               # none a multiple of a wave, a 16-byte pack times 256 lanes or a plane part; the
#                                                       last is the thinnest grid a handle admits (3 rows: gsm_set_static refuses fewer)
CHAINS = (5, 70)
NAN_CHAINS = (1, 3)                                   # the chains whose beds are NaN on all of region 5


def masks8(H, W):
    """[8, H, W] bool: 0 the whole domain; 1 a basin; 2 a rectangle that overlaps it; 3 empty; 4 one cell; 5 two cells that are NaN
    beds for the chains NAN_CHAINS; 6 a patch that holds the NaN of surf; 7 scattered cells."""
    m = np.zeros((8, H, W), dtype=bool)
    m[0] = True
    m[1, : max(2, 2 * H // 3), W // 5: 3 * W // 5] = True
    m[2, H // 3:, W // 2:] = True
    m[4, H - 1, W - 1] = True
    m[5, 1, 2:4] = True
    m[6, 0:2, W - 6: W - 2] = True
    m[7] = np.random.default_rng(5).random((H, W)) < 0.3
    return m


def surf_nan_cell(H, W):
    return 1, W - 4


@functools.lru_cache(maxsize=None)
def case(H, W, C, f32):
    """(x [C, H, W] float64 holding values the state type represents, fields of set_static, masks [8, H, W]); computed once, read-only."""
    rng = np.random.default_rng(1000 * H + W + C)
    ii, jj = np.mgrid[0:H, 0:W]
    surf = 450.0 + 430.0 * np.sin(0.11 * ii + 0.3) * np.cos(0.07 * jj) + rng.normal(0, 5, (H, W))     # 20 .. 880 m: thin and thick ice
    surf = np.maximum(surf, 8.0)
    x = 650.0 * np.sin(0.05 * jj + 0.13 * ii)[None] + rng.normal(0, 60, (C, H, W))                     # -830 .. 830: both sides of SEA,
    #                                                              above the surface in places, floating and grounded below sea level
    x[:, 2, 5:9] = SEA                                             # exactly at sea level: b == 0 is not below
    x[:, 2, 9] = np.nextafter(np.float32(SEA), np.float32(-1e9))   # and one fp32 step below it
    for j, e in enumerate((-512.0, -448.0, 0.0, 64.0, 496.0, 512.0)):
        x[:, 0, 10 + j] = e                                        # exactly at bin edges, the first and the last one included
    surf[2, 20:30] = 12.0                                          # thin ice over a deep bed, on every grid: afloat (q < 0 with b < 0)
    x[:, 2, 20:30] = -400.0 + rng.normal(0, 20, (C, 10))
    x[:, 0, 3] = -3000.0                                           # far into both overflow slots
    x[:, 0, 4] = 3000.0
    x[0, H // 2, W // 2] = np.nan
    x[2 % C, H - 1, 0] = np.inf                                    # not finite: not valid, whatever its sign
    for c in NAN_CHAINS:
        x[c, 1, 2:4] = np.nan
    surf[surf_nan_cell(H, W)] = np.nan
    if f32:
        x = x.astype(np.float32).astype(np.float64)
    f = dict(surf=surf, velx=rng.normal(0, 50, (H, W)), vely=rng.normal(0, 50, (H, W)), dhdt=rng.normal(0, 1, (H, W)),
             smb=rng.normal(0, 1, (H, W)), mc_mask=np.ones((H, W), dtype=np.uint8), resolution=500.0, sigma_mc=5.0)
    m = masks8(H, W)
    for a in (x, surf, m):
        a.setflags(write=False)
    return x, f, m


def terms(x, surf, sea=SEA, ratio=RATIO):
    """The per-cell terms of beds x [..., H, W] (fp64) in the operation order of include/gsm.h."""
    x = np.asarray(x, dtype=np.float64)
    s = np.broadcast_to(np.asarray(surf, dtype=np.float64), x.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        valid = np.isfinite(x) & np.isfinite(s)
        h = s - x
        t_thick = np.where(h > 0, h, 0.0)
        b = x - sea
        p = ratio * np.where(b < 0, b, 0.0)
        q = h + p
        t_haf = np.where(q > 0, q, 0.0)
        below = b < 0
    return dict(valid=valid, x=x, t_thick=t_thick, t_haf=t_haf, below=below, marine=below & (t_haf > 0))


def reference(x, surf, masks, sea=SEA, ratio=RATIO):
    """(func [C, K, 8] np.longdouble: the exact counts, the long-double sums of the restated terms, min and max;  A [C, K, 8] the sums
    of |term| of slots 1 .. 3 (0 elsewhere)) of beds x [C, H, W] over the regions masks [K, H, W]."""
    t = terms(x, surf, sea, ratio)
    C, K = x.shape[0], masks.shape[0]
    func = np.zeros((C, K, 8), dtype=np.longdouble)
    A = np.zeros((C, K, 8), dtype=np.longdouble)
    for c in range(C):
        for k in range(K):
            sel = t["valid"][c] & masks[k]
            xs = t["x"][c][sel]
            func[c, k, 0] = sel.sum()
            for f, name in ((1, "x"), (2, "t_thick"), (3, "t_haf")):
                v = t[name][c][sel].astype(np.longdouble)
                func[c, k, f] = v.sum()
                A[c, k, f] = np.abs(v).sum()
            func[c, k, 4] = (t["below"][c] & sel).sum()
            func[c, k, 5] = (t["marine"][c] & sel).sum()
            func[c, k, 6] = xs.min() if xs.size else np.inf
            func[c, k, 7] = xs.max() if xs.size else -np.inf
    return func, A


def hyps_reference(x, surf, masks, lo, inv_w, bins):
    """[C, K, bins + 2] int64: the valid cells of every chain and region per slot, kf = floor((x - lo) * inv_w) in fp64."""
    x = np.asarray(x, dtype=np.float64)
    valid = np.isfinite(x) & np.isfinite(surf)
    with np.errstate(invalid="ignore", over="ignore"):
        kf = np.floor((x - lo) * inv_w)
    slot = np.where(kf < 0, 0, np.where(kf >= bins, bins + 1, np.where(valid, kf, 0).astype(np.int64) + 1)).astype(np.int64)
    out = np.zeros((x.shape[0], masks.shape[0], bins + 2), dtype=np.int64)
    for c in range(x.shape[0]):
        for k in range(masks.shape[0]):
            sel = valid[c] & masks[k]
            out[c, k] = np.bincount(slot[c][sel], minlength=bins + 2)
    return out


def check_func(got, ref, A, label):
    """got [C, K, 8] against reference(): the exact slots equal, the sums within (m + 3) u sum |t|.  Returns the largest share of
    the bound a sum took."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, f"{label}: shape {got.shape} != {ref.shape}"
    for f in (0, 4, 5, 6, 7):
        assert np.array_equal(got[..., f], ref[..., f].astype(np.float64)), f"{label}: slot {f} differs from the restatement"
    m = ref[..., 0]
    worst = 0.0
    for f in (1, 2, 3):
        err = np.abs(got[..., f].astype(np.longdouble) - ref[..., f])
        bound = (m + 3) * U * A[..., f]
        with np.errstate(invalid="ignore", divide="ignore"):
            share = float(np.max(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))))
        print(f"{label}: slot {f} worst share of (m + 3) u sum|t| = {share:.3e}")
        assert (err <= bound).all(), f"{label}: slot {f}: {int((err > bound).sum())} sums beyond (m + 3) u sum|t|, worst {share:.3e} of it"
        worst = max(worst, share)
    return worst
