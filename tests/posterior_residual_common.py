"""Definitions, synthetic cases, reference and bounds of the posterior residual tests (mcmc_gpu_amd/posterior.py's docstring,
`residual`).  Shares nothing with the package; the sequences are those of tests/posterior_common.py.

Definitions.  x [C, T, H, W] the snapshots, r [C, T, H, W] their mass-conservation residuals (on the device: gsm_residual's output
for the fed bed; on the host: the np.gradient form below), rg [H, W] a shift, d = fl64(r - rg).  Per cell over the values with
finite r of the snapshots that belong to a sequence: cnt, S1 = sum d, S2 = sum d d, A_l = #(|r| > level_l).

Bounds (derived, not tuned), u = 2^-53, references in np.longdouble on the bits of d, n = cnt.
  exact     cnt and A_l are counts decided on the same bits of r: equal.
  S1        n terms added with at most n - 1 roundings in any order; four further units cover the second-order terms:
                |S1^ - sum d| <= (n + 3) u sum |d|
  S2        each square is rounded once, then as above:
                |S2^ - sum d d| <= (n + 4) u sum d d
  summary   with b1, b2 these two bounds and Q = S2 + 2 rg S1 + cnt rg^2 = sum r^2 (evaluated with at most four roundings per term):
                mean = rg + S1 / cnt                    b1 / cnt + 2 u (|rg| + |S1| / cnt)
                Q                                       bQ = b2 + 2 |rg| b1 + 4 u (S2 + 2 |rg| |S1| + cnt rg^2)
                rms = sqrt(Q / cnt)                     bQ / (2 cnt rms) + 3 u rms
                V = S2 - S1^2 / cnt                     bV = b2 + (2 |S1| b1 + b1^2) / cnt + 3 u (S2 + S1^2 / cnt)
                sd = sqrt(V / (cnt - 1))                bV / (2 (cnt - 1) sd) + 3 u sd
                loss density = Q / (2 sigma^2 M N)      bQ / (2 sigma^2 M N) + 3 u density
                expected loss = sum over the mask       the sum of the density bounds + (cells) u (the sum of the densities)
The synthetic fields keep every term of these sums of one size (beds -300 +- 100 m, surf - bed positive, velocities near 100 m/a):
a plain float64 accumulation in another order then uses well under half of the two sum bounds (tests/test_posterior_residual_host.py
asserts it)."""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble
NAN_BED = (5, 7)          # one NaN bed at chain 2, snapshot T - 2, this interior cell
NAN_BED_BORDER = (0, 20)  # and, where the grid is wide enough, one at chain 0, snapshot T - 1, this cell of the first row
NAN_VELX = (20, 30)       # one NaN in velx at this interior cell
LEVELS = (30.0, 120.0)
RESOLUTION, SIGMA_MC = 500.0, 5.0


def first_used(T, split):
    """Index of the first snapshot that belongs to a sequence."""
    return T - 2 * (T // 2) if split else 0


def fields(H, W, seed=0, nan_velx=False, partial_mask=True):
    """Static fields of a synthetic glacier: surf 700 .. 900 m (well above every bed), velocities near 100 m/a, small dhdt and smb, and a
    loss mask that covers part of the grid."""
    rng = np.random.default_rng(1000 + seed)
    f = dict(surf=800.0 + 30.0 * rng.normal(size=(H, W)).clip(-3, 3), velx=100.0 + 30.0 * rng.normal(size=(H, W)),
             vely=-80.0 + 30.0 * rng.normal(size=(H, W)), dhdt=0.5 * rng.normal(size=(H, W)), smb=1.0 + 0.5 * rng.normal(size=(H, W)),
             resolution=RESOLUTION, sigma_mc=SIGMA_MC)
    mask = np.ones((H, W), dtype=np.uint8)
    if partial_mask:
        mask[: H // 3] = 0
        mask[:, W - max(1, W // 4):] = 0
    f["mc_mask"] = mask
    if nan_velx:
        f["velx"][NAN_VELX] = np.nan
    return f


def beds(C, T, H, W, seed, f32=True, nan_bed=True):
    """(x [C, T, H, W], g [H, W]): x = -300 + 100 N(0, 1), rounded to float32 with f32 so that both state types see the same values;
    g = -300 + 10 N(0, 1); with nan_bed one NaN at chain 2 (the last chain if there are fewer), snapshot T - 2, cell NAN_BED, and one at
    chain 0, snapshot T - 1, cell NAN_BED_BORDER."""
    rng = np.random.default_rng(seed)
    x = -300.0 + 100.0 * rng.normal(size=(C, T, H, W))
    g = -300.0 + 10.0 * rng.normal(size=(H, W))
    if nan_bed:
        x[min(2, C - 1), T - 2, NAN_BED[0], NAN_BED[1]] = np.nan
        if W > NAN_BED_BORDER[1] + 1:
            x[0, T - 1, NAN_BED_BORDER[0], NAN_BED_BORDER[1]] = np.nan
    if f32:
        x = x.astype(np.float32).astype(np.float64)
    return x, g


def residual_numpy(bed, f):
    """Mass-conservation residual of bed [..., H, W] in np.gradient's form (Topography.py:592-600)."""
    thick = f["surf"] - np.asarray(bed, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return (np.gradient(f["velx"] * thick, f["resolution"], axis=-1) + np.gradient(f["vely"] * thick, f["resolution"], axis=-2)
                + f["dhdt"] - f["smb"])


def shift(g, f):
    """rg: the residual of the common field, non-finite values 0."""
    rg = residual_numpy(g, f)
    rg[~np.isfinite(rg)] = 0.0
    return rg


def reference_sums(r, rg, levels, lo=0):
    """dict of the per-cell references over r[:, lo:] [C, T', H, W]: cnt and above [L] int64 (exact), s1, s2, abs1 (sum |d|) in
    np.longdouble of d = fl64(r - rg), chain by chain."""
    r = np.asarray(r, dtype=np.float64)[:, lo:]
    shape = r.shape[2:]
    cnt = np.zeros(shape, dtype=np.int64)
    above = np.zeros((len(levels),) + shape, dtype=np.int64)
    s1, s2, abs1 = (np.zeros(shape, dtype=LD) for _ in range(3))
    with np.errstate(invalid="ignore"):
        for c in range(r.shape[0]):
            fin = np.isfinite(r[c])
            d = np.where(fin, r[c] - rg, 0.0).astype(LD)          # the float64 difference, then widened
            cnt += fin.sum(axis=0)
            s1 += d.sum(axis=0)
            s2 += (d * d).sum(axis=0)
            abs1 += np.abs(d).sum(axis=0)
            for l, lv in enumerate(levels):
                above[l] += (fin & (np.abs(r[c]) > lv)).sum(axis=0)
    return dict(cnt=cnt, above=above, s1=s1, s2=s2, abs1=abs1)


def sum_bounds(ref):
    """(b1, b2) [H, W] np.longdouble: (n + 3) u sum |d| and (n + 4) u sum d d."""
    n = ref["cnt"].astype(LD)
    return (n + 3) * U * ref["abs1"], (n + 4) * U * ref["s2"]


def _share(err, bound):
    ok = bound > 0
    return float((err[ok] / bound[ok]).max()) if ok.any() else 0.0


def check_sums(got, ref, label=""):
    """Assert the planes got [3 + L, H, W] float64 against reference_sums: counts equal, S1 and S2 within the two bounds (and exactly 0
    where the bound is 0); prints and returns the largest errors as shares of the bounds."""
    got = np.asarray(got, dtype=np.float64)
    L = ref["above"].shape[0]
    assert got.shape == (3 + L,) + ref["cnt"].shape, (got.shape, L)
    assert np.array_equal(got[0], ref["cnt"]), f"{label}: cnt differs in {(got[0] != ref['cnt']).sum()} cells"
    for l in range(L):
        assert np.array_equal(got[3 + l], ref["above"][l]), f"{label}: A_{l} differs in {(got[3 + l] != ref['above'][l]).sum()} cells"
    assert np.isfinite(got).all(), f"{label}: a plane holds a non-finite value"
    b1, b2 = sum_bounds(ref)
    e1, e2 = np.abs(got[1].astype(LD) - ref["s1"]), np.abs(got[2].astype(LD) - ref["s2"])
    shares = (_share(e1, b1), _share(e2, b2))
    print(f"residual sums {label}: n <= {int(ref['cnt'].max())}, S1 error {shares[0]:.3e} of (n + 3) u sum|d|, S2 error {shares[1]:.3e} of (n + 4) u sum d^2")
    assert (e1 <= b1).all(), f"{label}: {int((e1 > b1).sum())} cells of S1 beyond the bound, worst {shares[0]:.3e} of it"
    assert (e2 <= b2).all(), f"{label}: {int((e2 > b2).sum())} cells of S2 beyond the bound, worst {shares[1]:.3e} of it"
    return shares


def summary_reference(ref, rg, levels, mc_mask, sigma_mc, n_values):
    """The summary's maps from reference_sums in np.longdouble and their bounds (the module docstring): dict name -> (value, bound)
    with NaN where the map is undefined; 'expected_loss' -> (scalar, bound); 'prob' -> [L, H, W] exact ratios."""
    cnt = ref["cnt"].astype(LD)
    s1, s2 = ref["s1"], ref["s2"]
    b1, b2 = sum_bounds(ref)
    rgl = np.asarray(rg, dtype=LD)
    nan = LD(np.nan)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(cnt > 0, rgl + s1 / cnt, nan)
        b_mean = b1 / cnt + 2 * U * (np.abs(rgl) + np.abs(s1) / cnt)
        Q = s2 + 2 * rgl * s1 + cnt * rgl * rgl
        bQ = b2 + 2 * np.abs(rgl) * b1 + 4 * U * (s2 + 2 * np.abs(rgl) * np.abs(s1) + cnt * rgl * rgl)
        rms = np.where(cnt > 0, np.sqrt(Q / cnt), nan)
        b_rms = bQ / (2 * cnt * rms) + 3 * U * rms
        V = s2 - s1 * s1 / cnt
        bV = b2 + (2 * np.abs(s1) * b1 + b1 * b1) / cnt + 3 * U * (s2 + s1 * s1 / cnt)
        sd = np.where(cnt > 1, np.sqrt(np.maximum(V, 0) / (cnt - 1)), nan)
        b_sd = bV / (2 * (cnt - 1) * sd) + 3 * U * sd
        scale = 2 * LD(sigma_mc) ** 2 * n_values
        inside = np.asarray(mc_mask) == 1
        dens = np.where(cnt > 0, np.where(inside, Q / scale, 0), nan)
        b_dens = np.where(inside, bQ / scale + 3 * U * np.abs(Q) / scale, 0)
        live = inside & (cnt > 0)
        loss = dens[live].sum()
        b_loss = b_dens[live].sum() + int(live.sum()) * U * loss
        prob = np.where(cnt > 0, ref["above"] / cnt, nan)
    return dict(residual_mean=(mean, b_mean), residual_rms=(rms, b_rms), residual_sd=(sd, b_sd), loss_density=(dens, b_dens),
                expected_loss=(loss, b_loss), prob=prob)


def check_summary(s, ref, label=""):
    """Assert the methods of a PosteriorSummary against summary_reference within the propagated bounds; NaN sets equal."""
    levels = [float(v) for v in s.residual_levels]
    exp = summary_reference(ref, s.residual_ref, levels, s.residual_mc_mask, s.residual_sigma_mc, s.n_sequences * s.n_per_sequence)
    assert np.array_equal(s.residual_count(), ref["cnt"])
    out = {}
    for name in ("residual_mean", "residual_rms", "residual_sd", "loss_density"):
        got, (val, bound) = getattr(s, name)(), exp[name]
        assert np.array_equal(np.isnan(got), np.isnan(val.astype(np.float64))), f"{label} {name}: NaN cells differ"
        ok = ~np.isnan(got) & np.isfinite(bound.astype(np.float64))
        err = np.abs(got[ok].astype(LD) - val[ok])
        out[name] = _share(err, bound[ok])
        assert (err <= bound[ok]).all(), f"{label} {name}: {int((err > bound[ok]).sum())} cells beyond the bound, worst {out[name]:.3e} of it"
    loss, b_loss = exp["expected_loss"]
    out["expected_loss"] = float(abs(LD(s.expected_loss()) - loss) / b_loss) if b_loss > 0 else 0.0
    assert abs(LD(s.expected_loss()) - loss) <= b_loss, f"{label}: expected_loss {s.expected_loss()!r} against {loss!r}, bound {b_loss!r}"
    for l, lv in enumerate(levels):
        assert np.array_equal(s.prob_residual_above(lv), exp["prob"][l].astype(np.float64), equal_nan=True), f"{label}: prob above {lv}"
    print(f"residual summary {label}: " + ", ".join(f"{k} {v:.3e}" for k, v in out.items()) + " of the propagated bounds")
    return out


def direct_loss(r, mc_mask, sigma_mc, lo=0):
    """The mean over all chains and the snapshots t >= lo of the reference's loss nansum(r[mask]^2) / (2 sigma^2), in np.longdouble."""
    r = np.asarray(r, dtype=np.float64)[:, lo:].astype(LD)
    sq = np.where(np.isfinite(r), r * r, 0)[..., np.asarray(mc_mask) == 1]
    return sq.sum(axis=-1).mean() / (2 * LD(sigma_mc) ** 2)


def shift_rounding_bound(ref, rg, mc_mask, sigma_mc, n_values):
    """What the rounding of d = fl64(r - rg) itself can move the loss by: the sums are sums of d, and d + rg is r only to u |d|, so
    sum (d + rg)^2 differs from sum r^2 by at most 2 u sum |r| |d| <= 2 u sqrt(sum r^2 sum d^2) per cell (second order dropped: one
    further factor 1 + 2^-20 covers it).  Returned for the loss: summed over the mask and divided by 2 sigma^2 M N."""
    cnt, rgl = ref["cnt"].astype(LD), np.asarray(rg, dtype=LD)
    Q = ref["s2"] + 2 * rgl * ref["s1"] + cnt * rgl * rgl
    per_cell = 2 * U * np.sqrt(np.maximum(Q, 0) * ref["s2"]) * (1 + LD(2.0) ** -20)
    return per_cell[(np.asarray(mc_mask) == 1) & (ref["cnt"] > 0)].sum() / (2 * LD(sigma_mc) ** 2 * n_values)


def _chain_split(cells, n_chains, n_cu, min_chains):
    parts = max(1, min(-(-4 * n_cu // cells), n_chains, n_chains // min_chains))
    cpp = -(-n_chains // parts)
    filled = -(-n_chains // cpp)
    return dict(parts=parts, cpp=cpp, last=n_chains - (filled - 1) * cpp, empty=parts - filled)


def split_plan(H, W, n_chains, f32_state, n_cu):
    """How gsm_posterior_residual divides n_chains beds of H x W on a device of n_cu compute units, restated from the comments of
    posterior_residual_kernel.hip and posterior_device.h (nothing of the library is called): vec cells of a row per lane (16 bytes
    where W allows), tiles of lx lanes x ly rows (lx the power of two that holds W / vec, at most 32; ly = 256 / lx), and the chain
    axis cut into parts = min(ceil(4 n_cu / tiles), n_chains, n_chains // 8), at least 1, of cpp chains; `last` is the chain count of
    the last part that holds a chain and `empty` the number of parts after it."""
    vec = (4 if W % 4 == 0 else 2 if W % 2 == 0 else 1) if f32_state else (2 if W % 2 == 0 else 1)
    lanes = W // vec
    lx = 1
    while lx < 32 and lx < lanes:
        lx *= 2
    ly = 256 // lx
    tiles_x, tiles_y = -(-lanes // lx), -(-H // ly)
    return dict(vec=vec, lx=lx, ly=ly, tiles_x=tiles_x, tiles_y=tiles_y, **_chain_split(tiles_x * tiles_y, n_chains, n_cu, 8))


# the fed cases of the device suite, (H, W, C, T, split): the host suite shows the bounds are fair on the same draws
CASES = [(37, 41, 5, 8, True), (37, 41, 5, 9, True), (37, 41, 5, 9, False), (3, 130, 3, 4, False), (70, 3, 3, 4, False),
         (64, 64, 6, 6, False), (16, 24, 130, 2, False), (16, 24, 390, 2, False)]


def case_data(H, W, C, T, f32=True):
    """(x, g, fields) of one case: the NaN bed and the NaN velocity where the grid holds their cells."""
    big = H > NAN_VELX[0] + 1 and W > NAN_VELX[1] + 1
    x, g = beds(C, T, H, W, H * 1000 + W * 10 + T, f32=f32, nan_bed=H > NAN_BED[0] + 1 and W > NAN_BED[1] + 1)
    return x, g, fields(H, W, seed=H + W, nan_velx=big)
