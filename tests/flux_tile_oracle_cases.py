"""Cases of tests/test_gpu_flux_tile_oracle.py: the oracle parity checks on the flux-tile and bed-tile step kernels.

The strip kernels take every block table that `strip_table_ok` admits, so with GSM_STRIP at its default the oracle tests of
test_gpu_parity / test_gpu_fullsize / test_gpu_fused / test_gpu_philox run the strip family.  GSM_STRIP is read when an engine is
made: the test runs `run_cases(group_cases(group))` with GSM_STRIP=0 set, and every engine the cases make is off the strip kernels.
`run_cases` prints every case before running it and stops at the first exception.

Dispatch rule restated here (step_kernel.hip: launch_step, step_flux_kernel.hip: launch_step_flux, chain_fused_kernel.hip:
launch_chain_fused), with tile_cap = max (bh + 2)(bw + 2) and max_win = max(max_bh * max_bw, tile_cap - 1024):
  tile_cap <= 7168: flux-tile, KT = 2 (tile_cap <= 2048), 4 (<= 4096) or 7;
  otherwise:        bed-tile,  KMAX = 7 (max_win <= 7168), 12 (<= 12288) or 20 (<= 20480)."""
import time
from pathlib import Path

import numpy as np

import mcmc_oracle as orc
from gpu_common import oracle_chains, replay_inputs

GOLDEN = Path(__file__).resolve().parent / "golden"
LOSS_RTOL = 1e-10          # the project's standing bar (test_gpu_parity.LOSS_RTOL)

# name: (grid, block_min, block_max, family, cells per thread, proposals per chain, needs an unclipped window)
TABLES = {
    "flux_kt2": (96, 30, 42, "flux", 2, 80, True),
    "flux_kt4": (96, 30, 60, "flux", 4, 80, True),
    "flux_kt7": (128, 50, 80, "flux", 7, 60, True),
    "bed_kmax7": (128, 70, 84, "bed", 7, 60, True),
    "bed_kmax12": (128, 96, 110, "bed", 12, 60, True),
    "bed_kmax20": (160, 112, 140, "bed", 20, 40, False),     # blocks >= 112 on 160 cells: nearly every window clips
}
STRIP_ELIGIBLE = ("flux_kt2", "flux_kt4", "flux_kt7", "bed_kmax7")   # these go to the strip kernels unless GSM_STRIP=0
N_CHAINS = 2


def route(pairs):
    """(family, cells per thread, tile_cap, max_win) of a block table under the dispatch rule in this module's docstring."""
    bw, bh = np.asarray(pairs[0], dtype=np.int64), np.asarray(pairs[1], dtype=np.int64)
    tile_cap = int(((bh + 2) * (bw + 2)).max())
    max_win = max(int(bh.max() * bw.max()), tile_cap - 1024)
    if tile_cap <= 7 * 1024:
        return "flux", (2 if tile_cap <= 2 * 1024 else 4 if tile_cap <= 4 * 1024 else 7), tile_cap, max_win
    assert max_win <= 20 * 1024, "no step kernel takes this table"
    return "bed", (7 if max_win <= 7 * 1024 else 12 if max_win <= 12 * 1024 else 20), tile_cap, max_win


def _setup(name):
    H, bmin, bmax, family, cells, steps, need_interior = TABLES[name]
    prob, cfg, pairs, masks, rfp = orc.standard_setup(H, H, block_min=bmin, block_max=bmax, update_in_region=False)
    got = route(pairs)
    print(f"    {name}: grid {H}, blocks {bmin}-{bmax}, tile_cap {got[2]}, max_win {got[3]} -> {got[0]} {got[1]}", flush=True)
    assert got[:2] == (family, cells), f"{name}: the table lands on {got[:2]}, not on {(family, cells)}"
    return H, steps, need_interior, prob, cfg, pairs, masks, rfp


def _engine(H, n_chains, cfg, pairs, masks, state):
    from mcmc_gpu_amd.engine import GsmEngine
    eng = GsmEngine(H, H, n_chains, state_dtype=state)
    eng.set_static(cfg.surf, cfg.velx, cfg.vely, cfg.dhdt, cfg.smb, cfg.crf_data_weight, cfg.grounded_ice_mask,
                   cfg.mc_region_mask, cfg.resolution, cfg.sigma_mc)
    eng.set_blocks(pairs, masks)
    assert eng.strip_active() == 0, "the table went to the strip kernels"
    return eng


def oracle_conditions(outs, H, need_interior):
    """What keeps a case from passing vacuously: the oracle accepts between 20 % and 90 % of its proposals, windows hang over
    all four edges of the grid, and (where the table allows it) at least one window lies inside the grid."""
    rate = float(np.mean([o[4][1:].mean() for o in outs]))
    b = np.concatenate([o[6][1:] for o in outs])
    row, col, bh, bw = (b[:, i] for i in range(4))
    sides = {"top": row - bh / 2 < 0, "bottom": row + bh / 2 > H, "left": col - bw / 2 < 0, "right": col + bw / 2 > H}
    clipped = np.logical_or.reduce(list(sides.values()))
    print(f"    oracle: accept rate {rate:.2f}, clipped share {clipped.mean():.2f}", flush=True)
    assert 0.2 <= rate <= 0.9, f"oracle accept rate {rate}"
    assert all(v.any() for v in sides.values()), {k: bool(v.any()) for k, v in sides.items()}
    if need_interior:
        assert (~clipped).any(), "every window is clipped"


def _bars(eng, outs, loss0, loss, acc, equal_nan=False):
    for c, o in enumerate(outs):
        assert abs(loss0[c] - o[3][0]) <= LOSS_RTOL * abs(o[3][0]), f"initial loss, chain {c}"
        assert np.array_equal(acc[c], o[4][1:].astype(np.uint8)), f"accept mask differs, chain {c}"
        np.testing.assert_allclose(loss[c], o[3][1:], rtol=LOSS_RTOL, atol=0)
        assert np.array_equal(eng.beds[c].cpu().numpy().astype(np.float64), o[0], equal_nan=equal_nan), f"final bed differs, chain {c}"
        assert np.array_equal(eng.resampled[c].cpu().numpy().astype(np.float64), o[5]), f"resampled counts differ, chain {c}"


def replay_table(name, state="f64"):
    """Replay of the oracle's draws on one block table, windows clipped on every edge (update_in_region False).  fp32 state: the
    bars of test_gpu_parity.test_f32_state_mode_matches_its_oracle_and_tracks_fp64."""
    H, steps, need_interior, prob, cfg, pairs, masks, rfp = _setup(name)
    f32 = state == "f32"
    outs = oracle_chains(prob, cfg, pairs, masks, rfp, N_CHAINS, steps + 1, state_f32=f32)
    oracle_conditions(outs, H, need_interior)
    eng = _engine(H, N_CHAINS, cfg, pairs, masks, state)
    loss0 = eng.set_state(np.stack([orc.chain_initial_bed(prob, c) for c in range(N_CHAINS)]))
    loss, acc = eng.run_replay(*replay_inputs(eng, outs))
    assert eng.beds.dtype.itemsize == eng.energy.dtype.itemsize == (4 if f32 else 8)
    _bars(eng, outs, loss0, loss, acc)
    eng.close()
    if f32:
        outs64 = oracle_chains(prob, cfg, pairs, masks, rfp, N_CHAINS, steps + 1, state_f32=False)
        for c in range(N_CHAINS):
            assert (outs64[c][4] != outs[c][4]).sum() <= 1
            np.testing.assert_allclose(outs[c][3][:50], outs64[c][3][:50], rtol=1e-6)
        cfg.state_f32 = False


def nan_inputs(name):
    """The NaN cells of test_gpu_parity.test_nan_cells_follow_nansum_semantics at this table's grid size: a NaN patch in velx and a
    NaN cell in dhdt (static fields, seen by both chains), NaN holes in the initial bed of chain 1."""
    H, steps, need_interior, prob, cfg, pairs, masks, rfp = _setup(name)
    k = lambda v: v * H // 64
    cfg.velx = cfg.velx.copy(); cfg.velx[k(30):k(33), k(40):k(44)] = np.nan
    cfg.dhdt = cfg.dhdt.copy(); cfg.dhdt[k(12), k(12)] = np.nan
    beds0 = np.stack([orc.chain_initial_bed(prob, c) for c in range(N_CHAINS)])
    beds0[1, k(20):k(22), k(20):k(25)] = np.nan
    beds0[1, k(45), k(50)] = np.nan
    return H, steps, need_interior, prob, cfg, pairs, masks, rfp, beds0


def oracle_chains_from(beds0, prob, cfg, pairs, masks, rfp, n_iter, seed0=7):
    """gpu_common.oracle_chains with given initial beds."""
    cfg.state_f32 = False
    outs = []
    for c in range(len(beds0)):
        rf = orc.OracleRandField(rfp, seed0 + c, pairs, masks, prob["resolution"])
        outs.append(orc.run_chain(cfg, beds0[c].copy(), n_iter, rf, np.random.default_rng(seed=seed0 + c), record=True))
    return outs


def replay_table_nan(name):
    """NaN residuals are ignored by the loss (nansum), NaN thickness never trips the guard: the chains replay exactly and the NaN
    cells of the bed are still NaN, and the only NaN, at the end."""
    H, steps, need_interior, prob, cfg, pairs, masks, rfp, beds0 = nan_inputs(name)
    outs = oracle_chains_from(beds0, prob, cfg, pairs, masks, rfp, steps + 1)
    assert all(np.isfinite(o[3]).all() for o in outs)
    oracle_conditions(outs, H, need_interior)
    eng = _engine(H, N_CHAINS, cfg, pairs, masks, "f64")
    loss0 = eng.set_state(beds0)
    loss, acc = eng.run_replay(*replay_inputs(eng, outs))
    _bars(eng, outs, loss0, loss, acc, equal_nan=True)
    final = eng.beds.cpu().numpy()
    assert np.array_equal(np.isnan(final), np.isnan(beds0)) and np.isnan(final[1]).sum() >= 11 and not np.isnan(final[0]).any()
    eng.close()


def guard_table(name):
    """test_gpu_parity.test_thickness_guard_rejects on this table's instantiation: zero velocities make the loss independent of the
    bed, so only the thickness guard (surf - bed_next <= 0 -> loss = inf) can reject while u is tiny.  The window lies against the
    top left corner of the grid, so that the guard cell is read from a clipped block."""
    H, _, _, prob, cfg, pairs, masks, rfp = _setup(name)
    cfg.velx = np.zeros_like(cfg.velx)
    cfg.vely = np.zeros_like(cfg.vely)
    cfg.block_type = "RF"
    cfg.crf_data_weight = None
    eng = _engine(H, 1, cfg, pairs, masks, "f64")
    bed0 = orc.chain_initial_bed(prob, 0)
    eng.set_state(bed0[None])
    bh, bw = int(pairs[1, 0]), int(pairs[0, 0])
    row, col = bh // 2 - 3, bw // 2 - 5                      # window rows [0, row + bh/2): 3 block rows and 5 block columns cut off
    gr, gc = row + 2, col + 1                                # the guard cell, and its place in the block
    fr, fc = gr - (row - bh // 2), gc - (col - bw // 2)
    thick = (cfg.surf - bed0)[gr, gc]
    f_ok = np.zeros((bh, bw)); f_ok[fr, fc] = thick - 1e-9   # 1 nm of ice left: allowed
    f_bad = np.zeros((bh, bw)); f_bad[fr, fc] = thick        # thickness == 0: guard
    u = np.array([[1e-300, 1e-300, 0.999]])
    loss, acc = eng.run_replay(np.zeros((1, 3), int), np.array([[[row, col]] * 3]), u, eng.pack_fields([[f_bad, f_ok, f_bad]]))
    mc = orc.mc_residual(bed0, cfg.surf, cfg.velx, cfg.vely, cfg.dhdt, cfg.smb, cfg.resolution)
    lp = orc.gaussian_loss(mc, cfg.mc_region_mask, cfg.sigma_mc)[0]
    bed, exp_acc = bed0, []
    for f, uu in zip((f_bad, f_ok, f_bad), u[0]):
        a, bed, mc, lp, _ = orc.mh_step(cfg, bed, mc, lp, f, row, col, uu)
        exp_acc.append(a)
    assert exp_acc == [False, True, False]
    assert acc[0].tolist() == [0, 1, 0]
    assert np.array_equal(eng.beds[0].cpu().numpy(), bed) and bed[gr, gc] != bed0[gr, gc]
    np.testing.assert_allclose(loss[0], [lp] * 3, rtol=1e-12)
    eng.close()


def table_cases(name):
    """Group B, one table: fp64 state (the 96-110 table has its fp64 test in test_gpu_fullsize), fp32 state, NaN cells, guard."""
    cases = [] if name == "bed_kmax12" else [(f"replay_table[{name}-f64]", lambda: replay_table(name, "f64"))]
    return cases + [(f"replay_table[{name}-f32]", lambda: replay_table(name, "f32")),
                    (f"replay_table_nan[{name}]", lambda: replay_table_nan(name)),
                    (f"guard_table[{name}]", lambda: guard_table(name))]


# ---- group C: Philox mode ---------------------------------------------------------------------------------------------------

def philox_table(name, state, expect_fused, fields_vs_oracle=False):
    """gsm_run_philox on the fused kernel (where the table allows it) == gsm_propose_philox + gsm_run_replay == the two-kernel
    pipeline, bit for bit; centres anywhere, so that windows clip."""
    H, _, _, prob, cfg, pairs, masks, rfp = _setup(name)
    n_chains, n = 3, 24
    rfp = orc.standard_rf_params(); rfp.resolution = prob["resolution"]
    eng = _engine(H, n_chains, cfg, pairs, masks, state)
    ones = np.ones((H, H), dtype=np.uint8)
    eng.set_centres(ones)
    seeds = [61, 2 ** 40 + 62, 63]
    beds0 = np.stack([orc.chain_initial_bed(prob, c) for c in range(n_chains)])

    def state_now():
        return (eng.beds.cpu().numpy().copy(), eng.resampled.cpu().numpy().copy(), eng.energy.cpu().numpy().copy())

    eng.set_fused(True)
    eng.set_state(beds0)
    loss, acc, blk = eng.run_philox(n, 9, seeds, rfp, batch=n)
    fused = eng.last_run_fused()
    print(f"    {name} {state}: last_run_fused() == {fused}, accept rate {acc.mean():.2f}", flush=True)
    assert fused == expect_fused
    st_a = state_now()
    assert st_a[0].dtype.itemsize == (4 if state == "f32" else 8)
    assert 0.2 <= acc.mean() <= 0.95
    row, col, bh, bw = (blk[..., i] for i in range(4))
    assert ((row - bh // 2 < 0) | (row + bh // 2 > H) | (col - bw // 2 < 0) | (col + bw // 2 > H)).any()

    eng.set_state(beds0)
    p = eng.propose_philox(n, 9, seeds, rfp)
    si, ce = p["size_idx"].cpu().numpy(), p["centre"].cpu().numpy()
    loss_r, acc_r = eng.run_replay(si, ce, p["u"].cpu().numpy(), p["fields"])
    assert np.array_equal(loss, loss_r) and np.array_equal(acc, acc_r)
    assert np.array_equal(blk[..., :2], ce) and np.array_equal(blk[..., 2], pairs[1][si]) and np.array_equal(blk[..., 3], pairs[0][si])
    for x, y in zip(st_a, state_now()):
        assert np.array_equal(x, y)

    if fused:
        eng.set_fused(False)
        eng.set_state(beds0)
        loss_p, acc_p, blk_p = eng.run_philox(n, 9, seeds, rfp, batch=7)
        assert eng.last_run_fused() == 0
        assert np.array_equal(loss, loss_p) and np.array_equal(acc, acc_p) and np.array_equal(blk, blk_p)
        for x, y in zip(st_a, state_now()):
            assert np.array_equal(x, y)

    if fields_vs_oracle:         # the direct-sum, non-Parseval proposal path against the Philox oracle, as test_proposals_256_blocks_match_oracle
        import philox_oracle as po
        centres = np.arange(H * H)
        for c in range(2):
            for s in range(6):
                e = po.proposal(seeds[c], 9 + s, rfp, pairs, masks, centres, H, prob["resolution"])
                assert int(si[c, s]) == e["size_idx"] and tuple(ce[c, s].tolist()) == e["centre"]
                fbh, fbw = e["field"].shape
                f = p["fields"][c, s, : fbh * fbw].cpu().numpy().reshape(fbh, fbw)
                np.testing.assert_allclose(f, e["field"], rtol=0, atol=po.field_atol(e))
    eng.close()


def philox_cases():
    cases = []
    for name in ("flux_kt2", "flux_kt4", "flux_kt7"):
        for state in ("f64", "f32"):
            cases.append((f"philox_table[{name}-{state}]",
                          lambda name=name, state=state: philox_table(name, state, 1, fields_vs_oracle=(name == "flux_kt4" and state == "f64"))))
    # tile_cap 7396 > 7168: step_flux_supported is false, so fused_supported is, and gsm_run_philox takes the two-kernel pipeline
    cases.append(("philox_table[bed_kmax7-f64]", lambda: philox_table("bed_kmax7", "f64", 0)))
    return cases


# ---- group A: the existing oracle bodies ------------------------------------------------------------------------------------

def parity_cases():
    import test_gpu_fullsize as tf
    import test_gpu_parity as tp
    return [("test_gpu_parity.test_replay_standard_64", lambda: tp.test_replay_standard_64(GOLDEN)),
            ("test_gpu_parity.test_replay_variant_rf_whole_map_nugget", lambda: tp.test_replay_variant_rf_whole_map_nugget(GOLDEN)),
            ("test_gpu_parity.test_replay_256_full_size_blocks", lambda: tp.test_replay_256_full_size_blocks(GOLDEN)),
            ("test_gpu_parity.test_replay_in_segments_equals_one_call", tp.test_replay_in_segments_equals_one_call),
            ("test_gpu_parity.test_thickness_guard_rejects", tp.test_thickness_guard_rejects),
            ("test_gpu_parity.test_f32_state_mode_matches_its_oracle_and_tracks_fp64", tp.test_f32_state_mode_matches_its_oracle_and_tracks_fp64),
            ("test_gpu_parity.test_nan_cells_follow_nansum_semantics", tp.test_nan_cells_follow_nansum_semantics),
            ("test_gpu_parity.test_tiny_grid", tp.test_tiny_grid),
            ("test_gpu_fullsize.test_ragged_grid_all_edges_clipped", tf.test_ragged_grid_all_edges_clipped),
            ("test_gpu_fullsize.test_block_as_large_as_the_grid_and_single_chain", tf.test_block_as_large_as_the_grid_and_single_chain)]


_VARIANTS = [("Matern", True, 0.0, "CRF_weight", True), ("Gaussian", False, 4.0, "RF", False), ("Exponential", True, 0.0, "CRF_weight", True)]


def fused_cases():
    import test_gpu_fused as tu
    cases = [(f"test_gpu_fused.test_fused_equals_two_kernel_pipeline[{v[0]}]", lambda v=v: tu.test_fused_equals_two_kernel_pipeline(*v))
             for v in _VARIANTS]
    return cases + [("test_gpu_fused.test_fused_fp32_state_equals_two_kernel_pipeline", tu.test_fused_fp32_state_equals_two_kernel_pipeline),
                    ("test_gpu_fused.test_fused_nan_fields_and_thickness_guard_equal_two_kernel_pipeline",
                     tu.test_fused_nan_fields_and_thickness_guard_equal_two_kernel_pipeline),
                    ("test_gpu_fused.test_fused_256_headline_blocks_equal_propose_then_replay", tu.test_fused_256_headline_blocks_equal_propose_then_replay),
                    ("test_gpu_fused.test_fused_segments_reproduce_unsplit_run", tu.test_fused_segments_reproduce_unsplit_run)]


def philox_oracle_cases():
    import test_gpu_philox as th
    cases = [(f"test_gpu_philox.test_proposals_match_oracle[{v[0]}]", lambda v=v: th.test_proposals_match_oracle(*v[:3])) for v in _VARIANTS]
    return cases + [("test_gpu_philox.test_proposals_256_blocks_match_oracle", th.test_proposals_256_blocks_match_oracle),
                    ("test_gpu_philox.test_run_philox_equals_propose_then_replay", th.test_run_philox_equals_propose_then_replay)]


def group_cases(group):
    if group.startswith("table:"):
        return table_cases(group[len("table:"):])
    return {"parity": parity_cases, "fused": fused_cases, "philox_oracle": philox_oracle_cases, "philox_tables": philox_cases}[group]()


def run_cases(cases):
    for name, fn in cases:
        print(f"CASE {name}", flush=True)
        t0 = time.perf_counter()
        fn()
        print(f"  ok {time.perf_counter() - t0:.2f} s", flush=True)

