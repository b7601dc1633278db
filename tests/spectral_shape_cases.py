"""Cases of tests/test_spectral_shape_cases.py (CPU) and tests/test_gpu_spectral_shapes.py: the device spectral synthesis
(proposal_device.h, through gsm_spectral_from_noise) at EVERY even block shape from 2 x 2 to 128 x 128, against
mcmc_oracle.spectral_from_draws.

Tables.  Band i (0 .. 7) holds the eight even lengths 16 i + 2 .. 16 i + 16; table (i, j) the 64 shapes with heights in band i
and widths in band j -- the 64-size limit of gsm_set_blocks.  Two more tables, EXTRA, reach the one geometry the square sweep
cannot: more than 8 MFMA tiles along a side (tile_magic's division branch) needs a length beyond 128.

Edge masks.  mask[y][x] = T[min(y, bh - 1 - y, x, bw - 1 - x)], T[d] = 0.75 + d / 256: exact in fp64, never zero and another
value on every ring, so the border cells count (the oracle's logistic taper is 0 there) and a wrong ring index shows.

Draws per shape (one set serves the three models): default_rng(1000 bh + bw); two fractions U(0.15, 0.6) ->
range_x, range_y = max(fraction min(bh, bw) res, 1.5 res), res = 500 (anisotropic, tied to the block: with the driver's
10-50 km ranges a small block's spectrum is numerically all DC and the standardisation amplifies DFT rounding noise, in the
reference as well); scale = U(50, 150) / 3; two normal planes; nug = U(0, 4) and a normal(0, sqrt(nug)) plane.

The geometry of the device code is restated here -- prop_geom, the table sizes of gsm_set_blocks, the admission test of
check_propose_ready, wide_table, strip_table_ok with strip::config -- so that the tests know which branch every shape takes and
can assert the handle's own decisions (refusals, strip_active) against the restatement."""
import functools

import numpy as np

import mcmc_oracle as orc

RES = 500.0
NU = 0.9125
GRID = 128                                   # the sweep's engine: one 128 x 128 grid
# (model, with the nugget plane) -- the three calls per table
MODELS = (("Matern", False), ("Exponential", True), ("Gaussian", False))
BAR = 1e-12                                  # x scale: the standing bar of tests/test_spectral_pin.py, flat

K_MATH_TAB, K_T1S, K_MASK1D, K_NR = 384, 128, 64, 16      # math_tables.h, proposal_device.h, gsm_internal.h, strip_step.h
K_STRIP_AUX = 16 + 32 + 16 + K_MATH_TAB + 4 * K_T1S + K_MASK1D


def band(i):
    return [16 * i + 2 * k for k in range(1, 9)]


def table_shapes(i, j):
    """(bh, bw) of table (i, j), size index = position."""
    return [(bh, bw) for bh in band(i) for bw in band(j)]


# beyond the square sweep: 9 tiles along the height (stage 2's tile rows) and along the half width (stage 1's tile columns)
EXTRA = {"tall": [(bh, bw) for bh in range(130, 145, 2) for bw in band(0)],
         "long": [(bh, bw) for bh in band(0) for bw in range(258, 273, 2)]}
EXTRA_GRID = {"tall": (144, 16), "long": (16, 272)}


def pairs_of(shapes):
    """(2, n) array of RandField.pairs: row 0 widths, row 1 heights."""
    return np.array([[bw for _, bw in shapes], [bh for bh, _ in shapes]])


def mask1d(bh, bw):
    yy, xx = np.meshgrid(np.arange(bh), np.arange(bw), indexing="ij")
    d = np.minimum(np.minimum(yy, bh - 1 - yy), np.minimum(xx, bw - 1 - xx))
    return 0.75 + d / 256.0


def draws(bh, bw):
    """The draws of a shape, in the layout of mcmc_oracle.spectral_draws."""
    rng = np.random.default_rng(1000 * bh + bw)
    fx, fy = rng.uniform(0.15, 0.6, size=2)
    range_x, range_y = (max(f * min(bh, bw) * RES, 1.5 * RES) for f in (fx, fy))
    scale = rng.uniform(50, 150) / 3.0
    n_re = rng.normal(size=(bh, bw))
    n_im = rng.normal(size=(bh, bw))
    nug = rng.uniform(0.0, 4.0)
    n_nug = rng.normal(0, np.sqrt(nug), size=(bh, bw))
    return dict(scale=scale, nug=nug, range_x=range_x, range_y=range_y, n_re=n_re, n_im=n_im, n_nug=n_nug)


def rf_params(model, nugget):
    """The ranges and the scale arrive per field (rf_scalars): only the model, nu and the nugget switch matter here."""
    p = orc.RFParams(0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 4.0 if nugget else 0.0, model, False, NU if model == "Matern" else None)
    p.resolution = RES
    return p


def raw_field(d, model, shape):
    """The reference's field before the standardisation (MCMC.py:242-247)."""
    amp = orc.spectral_amplitude(shape, RES, model, d["range_x"], d["range_y"], NU if model == "Matern" else None)
    return np.fft.ifft2((d["n_re"] + 1j * d["n_im"]) * amp).real


def expected(d, model, nugget, shape):
    """mcmc_oracle.spectral_from_draws; without the nugget the plane added is 0 (x + 0.0 == x)."""
    dd = d if nugget else dict(d, n_nug=np.zeros(shape))
    return orc.spectral_from_draws(dd, rf_params(model, nugget), shape, RES)


def longdouble_field(d, model, nugget, shape):
    """spectral_from_draws with the inverse DFT as long-double matrix products: cos / sin of 2 pi ((k j) mod n) / n evaluated in
    np.longdouble (the angle reduced in integers), the same amplitude, then the same standardisation in long double."""
    bh, bw = shape
    L = np.longdouble
    amp = orc.spectral_amplitude(shape, RES, model, d["range_x"], d["range_y"], NU if model == "Matern" else None)
    A, B = (d["n_re"] * amp).astype(L), (d["n_im"] * amp).astype(L)

    two_pi = 2 * np.arctan2(L(0), L(-1))                    # pi in long double: np.pi is a double

    def cs_ld(n):
        k = np.arange(n)
        ang = two_pi * ((k[:, None] * k[None, :]) % n).astype(L) / L(n)
        return np.cos(ang), np.sin(ang)

    Cy, Sy = cs_ld(bh)
    Cx, Sx = cs_ld(bw)
    fld = ((Cy @ A - Sy @ B) @ Cx.T - (Cy @ B + Sy @ A) @ Sx.T) / L(bh * bw)      # Re(Ey Z Ex^T) / n
    fld = (fld - fld.mean()) / (np.sqrt(((fld - fld.mean()) ** 2).mean()) + L(1e-12))
    return fld * L(d["scale"]) + (d["n_nug"].astype(L) if nugget else L(0))


# ---- the device's geometry, restated ----------------------------------------------------------------------------------------

def prop_geom(bh, bw, split2_allowed=False):
    """proposal_device.h: prop_geom (without the LDS strides and the tile magics)."""
    g = dict(bh=bh, bw=bw, hh=bh // 2, hw=bw // 2)
    g["ncol"], g["nrow"] = g["hw"] + 1, g["hh"] + 1
    g["KR"], g["NR"] = (g["nrow"] + 3) & ~3, (g["nrow"] + 15) & ~15
    g["M1"], g["Kc"] = (g["ncol"] + 15) & ~15, (g["ncol"] + 3) & ~3
    g["N1"] = (bh + 15) & ~15
    g["hq"] = g["hh"] >> 1; g["NRh"] = (g["hq"] + 16) & ~15; g["Ke"] = (g["hq"] + 4) & ~3
    g["hqx"] = g["hw"] >> 1; g["M1h"] = (g["hqx"] + 16) & ~15; g["Kce"] = (g["hqx"] + 4) & ~3
    g["split2"] = bool(split2_allowed) and (g["N1"] >> 4) * (g["M1h"] >> 4) <= 8
    return g


def _stride16mod32(v):
    while (v & 31) != 16:
        v += 1
    return v


def table_sizes(shapes):
    """gsm_set_blocks: lds_sx, lds_st, lds_x_half, lds_tt, prop_tiles, prop_tiles1 (+ the step kernels' tile_cap)."""
    gs = [prop_geom(bh, bw) for bh, bw in shapes]
    sx = _stride16mod32(max(g["M1"] for g in gs))
    st = _stride16mod32(max(g["N1"] for g in gs))
    t = dict(lds_sx=sx, lds_st=st, lds_x_half=(max(g["KR"] for g in gs) * sx + 127) & ~127, lds_tt=2 * max(g["Kc"] for g in gs) * st,
             prop_tiles=max((g["N1"] // 16) * (g["M1"] // 16) for g in gs),
             prop_tiles1=max(2 * (g["M1"] // 16) * (g["NRh"] // 16) for g in gs),          # even heights only
             tile_cap=max((bh + 2) * (bw + 2) for bh, bw in shapes),
             max_bh=max(bh for bh, _ in shapes), max_bw=max(bw for _, bw in shapes), n_sizes=len(shapes))
    t["lds_main"] = max(4 * t["lds_x_half"], t["lds_tt"])
    return t


def set_blocks_ok(t):
    """gsm_set_blocks: the (bh + 2) (bw + 2) window of the step kernels fits the 160 KiB LDS tile (step_lds_bytes)."""
    return (t["tile_cap"] + 3 * 16 + 64) * 8 <= 160 * 1024


def propose_ok(t):
    """check_propose_ready: LDS of the stand-alone proposal kernel, 4 stage-2 tiles and 4 stage-1 tiles per wave on 8 waves."""
    return (t["lds_main"] + 64 + K_MATH_TAB) * 8 <= 160 * 1024 and t["prop_tiles"] <= 32 and t["prop_tiles1"] <= 32


def wide_table(t):
    return t["prop_tiles"] > 16 or t["prop_tiles1"] > 16


def strip_config(wh, ww):
    """strip::config: (g, sr, n)."""
    g, sr = (1, 8) if ww <= 62 else (5, 6) if ww <= 70 else (3, 5) if ww <= 90 else (2, 4) if ww <= 124 else (4, 2) if ww <= 248 else (8, 1)
    return g, sr, -(-wh // sr)


def strip_table_ok(t, H, W, have_static=True, masks_1d=True):
    """chain_strip_kernel.hip: strip_table_ok (GSM_STRIP at its default)."""
    if t["max_bw"] > 496 or any(strip_config(t["max_bh"], ww)[2] > K_NR for ww in range(1, t["max_bw"] + 1)):
        return False
    lds = (max(t["lds_main"], (t["max_bh"] + 2) * (t["max_bw"] + 2)) + K_STRIP_AUX) * 8
    return (have_static and H * W * 48 <= (4 << 20) and t["n_sizes"] <= 64 and t["max_bh"] <= K_T1S and t["max_bw"] <= K_T1S and masks_1d and
            (min(t["max_bh"], t["max_bw"]) - 1) // 2 < K_MASK1D and lds <= 80 * 1024 and 2 * t["prop_tiles1"] <= 8 * 4 and t["prop_tiles"] <= 8 * 2)


@functools.lru_cache(maxsize=None)
def table_plan(key):
    """What the restatement expects of a table -- key (i, j) or a name of EXTRA -- on a handle with static fields:
    dict(shapes, sizes, admissible, wide, strip, split2: per shape)."""
    shapes = EXTRA[key] if isinstance(key, str) else table_shapes(*key)
    H, W = EXTRA_GRID[key] if isinstance(key, str) else (GRID, GRID)
    t = table_sizes(shapes)
    ok = set_blocks_ok(t) and propose_ok(t)
    strip = ok and strip_table_ok(t, H, W)
    return dict(shapes=shapes, sizes=t, admissible=ok, wide=ok and wide_table(t), strip=strip,
                split2=[prop_geom(bh, bw, strip)["split2"] for bh, bw in shapes])


ALL_TABLES = [(i, j) for i in range(8) for j in range(8)]


def last_step_rows(K_last, n_valid, n_padded):
    """The last K step of a parity-split sum (dft_stage1 / dft_stage2: kstep(K - 4, true)): lane group l4 reads the rows
    rE = 2 (K - 4 + l4) and rE + 1.  Per group: 'both' rows hold coefficients (rO < n_valid), 'one' (rE < n_valid <= rO), 'none'
    -- then either zero padding (rE < n_padded) or beyond it, where the kernel reads a clamped row and zeroes the operand."""
    out = set()
    for l4 in range(4):
        rE = 2 * (K_last - 4 + l4)
        out.add("both" if rE + 1 < n_valid else "one" if rE < n_valid else "none_padded" if rE < n_padded else "none_clamped")
    return out


def classes(bh, bw, plan=None, idx=None):
    """The geometry classes of a shape, as a set of labels (coverage counts of the tests)."""
    g = prop_geom(bh, bw, bool(plan and plan["split2"][idx]))
    c = {f"bh%4={bh % 4}", f"bw%4={bw % 4}"}
    for name in ("nrow", "ncol"):
        if g[name] % 16 == 0: c.add(f"{name}=16k")
        if g[name] % 16 == 1: c.add(f"{name}=16k+1")
    for name in ("hq", "hqx"):
        if (g[name] + 1) % 16 == 0: c.add(f"{name}+1=16k")
        if (g[name] + 1) % 16 == 1: c.add(f"{name}+1=16k+1")
    c |= {"s1_last_" + s for s in last_step_rows(g["Ke"], g["nrow"], g["KR"])}
    if g["split2"]:
        c |= {"s2_last_" + s for s in last_step_rows(g["Kce"], g["ncol"], g["Kc"])}
    if plan is not None:
        if plan["strip"]:
            c.add("strip_split2_on" if g["split2"] else "strip_split2_off")
        c.add("wide" if plan["wide"] else "narrow")
    if max(g["M1"] >> 4, g["N1"] >> 4) > 8:
        c.add("tiles_per_side>8")
    return c


REQUIRED_CLASSES = (["bh%4=0", "bh%4=2", "bw%4=0", "bw%4=2"] +
                    [f"{n}=16k{s}" for n in ("nrow", "ncol", "hq+1", "hqx+1") for s in ("", "+1")] +
                    ["s1_last_both", "s1_last_one", "s1_last_none_padded", "s1_last_none_clamped",
                     "s2_last_both", "s2_last_one", "s2_last_none_padded", "s2_last_none_clamped",
                     "strip_split2_on", "strip_split2_off", "tiles_per_side>8", "narrow", "wide"])


def count_classes(keys, static=True):
    """Class counts over the admissible shapes of the tables `keys`."""
    n = {}
    for key in keys:
        plan = table_plan(key)
        if not plan["admissible"]:
            continue
        use = plan if static else dict(plan, strip=False, split2=[False] * len(plan["shapes"]))
        for idx, (bh, bw) in enumerate(plan["shapes"]):
            for c in classes(bh, bw, use, idx):
                n[c] = n.get(c, 0) + 1
    return n


def subsample():
    """The fixed subsample of the long-double comparison: every 23rd case of the sweep's 4096 x 3 and all shapes up to 4 x 4."""
    cases = [(bh, bw, m) for (i, j) in ALL_TABLES for (bh, bw) in table_shapes(i, j) for m in range(3)]
    pick = set(cases[::23]) | {(bh, bw, m) for bh in (2, 4) for bw in (2, 4) for m in range(3)}
    return sorted(pick)
