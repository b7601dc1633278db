"""Cases of tests/test_gpu_strip_trim.py (and their CPU conditions, tests/test_strip_trim.py): the strip kernels cut every window
down to the static rectangle of gsm_set_static -- the bounding box of the update mask grown by one cell -- before they deal it into
strips (strip_step.h: make_window with the rectangle).  Centres lie anywhere (update_in_region False: the update mask is the
config's grounded_ice_mask, replaced here by the case's mask) and the loss mask is all ones, so the cells that the trimming leaves
out carry non-zero energies: the step's result is unchanged only if their recomputed energy would have equalled the carried one.

Every case derives from the recorded blocks what the trimming did to each step (restated here: rectangle, trimmed window,
strip::config of both) and asserts its conditions, so that none passes vacuously.  Masks are given as inclusive row / column
ranges."""
import functools

import numpy as np

import mcmc_oracle as orc
from gpu_common import oracle_chains
from strip_oracle_cases import config, window

N_CHAINS = 2
N_STEPS = 60


def _box(H, W, r0, r1, c0, c1):
    m = np.zeros((H, W), dtype=np.int64)
    m[r0:r1 + 1, c0:c1 + 1] = 1
    return m


def _l_shape(H, W):
    """An L against the left grid edge -- a bar of rows 18-70 x columns 0-20 and a foot of rows 50-70 x columns 0-52 -- with a hole
    of rows 55-60 x columns 5-10: only its bounding box, rows 18-70 x columns 0-52, may matter to the geometry."""
    m = _box(H, W, 18, 70, 0, 20) | _box(H, W, 50, 70, 0, 52)
    m[55:61, 5:11] = 0
    return m


# name: (H, W, bw_min, bw_max, bh_min, bh_max, update mask[, sigma_mc])
# "empty": with the standard sigma_mc = 5 the few cells of a 16 x 16 mask that a block changes hardly move the loss, and 27 of the 28
# non-empty steps are accepted (seeds 7 to 18 alike: 0.95 to 1.0); sigma_mc = 1 gives 15 of 28.  Grid, blocks and mask stay the case's.
CASES = {
    "regroup": (96, 100, 72, 90, 50, 80, lambda: _box(96, 100, 20, 75, 22, 77)),
    "deeper": (104, 72, 40, 62, 64, 94, lambda: _box(104, 72, 16, 87, 10, 61)),
    # the same table with a mask wide enough to leave some windows whole (widened until the CPU count said so: 10 of 120 steps)
    "deeper_some_whole": (104, 72, 40, 62, 64, 94, lambda: _box(104, 72, 3, 100, 2, 69)),
    "l_shape": (96, 80, 64, 70, 50, 80, lambda: _l_shape(96, 80)),
    "empty": (64, 64, 8, 16, 8, 16, lambda: _box(64, 64, 24, 39, 24, 39), 1.0),
}


def rectangle(mask):
    """[tr0, tr1) x [tc0, tc1): gsm_set_static restated."""
    H, W = mask.shape
    rows, cols = np.flatnonzero(mask.any(axis=1)), np.flatnonzero(mask.any(axis=0))
    if rows.size == 0:
        return 0, 0, 0, 0
    return max(rows[0] - 1, 0), min(rows[-1] + 2, H), max(cols[0] - 1, 0), min(cols[-1] + 2, W)


def setup(name):
    H, W, bw0, bw1, bh0, bh1, mask = CASES[name][:7]
    prob, cfg, _, _, rfp = orc.standard_setup(H, W, block_min=bw0, block_max=bw1, sigma_mc=(CASES[name] + (5.0,))[7], update_in_region=False)
    cfg.grounded_ice_mask = mask()
    assert cfg.mc_region_mask.all()
    pairs = orc.block_pairs(bw0, bw1, bh0, bh1)
    masks = orc.edge_masks(pairs, [2, 0, 6, 1], 49900.0, prob["resolution"])
    return H, W, prob, cfg, pairs, masks, rfp


def engine(name, n_chains, state="f64"):
    from mcmc_gpu_amd.engine import GsmEngine
    H, W, prob, cfg, pairs, masks, rfp = setup(name)
    eng = GsmEngine(H, W, n_chains, state_dtype=state)
    eng.set_static(cfg.surf, cfg.velx, cfg.vely, cfg.dhdt, cfg.smb, cfg.crf_data_weight, cfg.grounded_ice_mask, cfg.mc_region_mask,
                   cfg.resolution, cfg.sigma_mc)
    eng.set_blocks(pairs, masks)
    return eng, prob, cfg, pairs, masks, rfp


@functools.lru_cache(maxsize=None)
def oracle_outs(name, f32=False):
    """The oracle's chains of a case (seeds 7 and 8), computed once per state dtype and left unchanged."""
    H, W, prob, cfg, pairs, masks, rfp = setup(name)
    return oracle_chains(prob, cfg, pairs, masks, rfp, N_CHAINS, N_STEPS + 1, state_f32=f32)


def oracle_blocks(outs):
    return np.concatenate([o[6][1:] for o in outs]).astype(int), np.concatenate([o[4][1:] for o in outs]).astype(bool)


def trims(name, blocks):
    """Per step (row, col, bh, bw): dict(whole=(wh, ww), cut=(wh', ww'), empty, sides cut, decomposition and n of both)."""
    H, W = CASES[name][:2]
    tr0, tr1, tc0, tc1 = rectangle(CASES[name][6]())
    out = []
    for row, col, bh, bw in np.asarray(blocks).reshape(-1, 4):
        r0, r1, c0, c1, _ = window(row, col, bh, bw, H, W)
        q0, q1, p0, p1 = max(r0, tr0), min(r1, tr1), max(c0, tc0), min(c1, tc1)
        empty = q1 <= q0 or p1 <= p0
        wh, ww = (0, 0) if empty else (q1 - q0, p1 - p0)
        g, sr, n = config(r1 - r0, c1 - c0)
        g2, sr2, n2 = config(wh, ww)
        out.append(dict(whole=(r1 - r0, c1 - c0), cut=(wh, ww), empty=empty, trimmed=(wh, ww) != (r1 - r0, c1 - c0),
                        top=not empty and q0 > r0, bottom=not empty and q1 < r1, left=not empty and p0 > c0, right=not empty and p1 < c1,
                        dec=(g, sr), dec_cut=(g2, sr2), n=n, n_cut=n2))
    return out


def conditions(name, blocks, acc):
    """What keeps a case from passing vacuously; printed, then asserted."""
    t = trims(name, blocks)
    acc = np.asarray(acc).astype(bool).ravel()
    live = np.array([not x["empty"] for x in t])
    n_trim = sum(x["trimmed"] for x in t)
    n_empty = sum(x["empty"] for x in t)
    n_whole = len(t) - n_trim
    regroup = sum(1 for x in t if not x["empty"] and x["dec_cut"] != x["dec"])
    shallower = sum(1 for x in t if not x["empty"] and x["dec_cut"] == x["dec"] and x["n_cut"] < x["n"])
    sides = {k: sum(x[k] for x in t) for k in ("top", "bottom", "left", "right")}
    rate = float(acc.mean())
    rate_live = float(acc[live].mean()) if live.any() else float("nan")
    print(f"    {name}: {len(t)} steps, {n_trim} trimmed ({n_empty} to nothing), {n_whole} whole; cut at " +
          " / ".join(f"{k} {v}" for k, v in sides.items()) + f"; {regroup} change the decomposition, {shallower} keep it with a smaller n; "
          f"accept rate {rate:.2f} ({rate_live:.2f} over the non-empty windows)", flush=True)
    assert all(x["n_cut"] <= x["n"] for x in t)
    if name == "regroup":
        assert regroup >= 10 and all(v >= 3 for v in sides.values()) and 0.2 <= rate <= 0.9, (regroup, sides, rate)
    elif name == "deeper":
        assert shallower >= 10, shallower
    elif name == "deeper_some_whole":
        assert n_whole >= 3 and shallower >= 10, (n_whole, shallower)
    elif name == "l_shape":
        assert n_trim - n_empty >= 10, (n_trim, n_empty)
        assert 0.2 <= rate <= 0.9, rate
    elif name == "empty":
        assert n_empty >= 10 and live.sum() >= 10 and 0.2 <= rate_live <= 0.9, (n_empty, int(live.sum()), rate_live)
        assert acc[~live].all(), "a step that changes nothing was rejected"
    return t
