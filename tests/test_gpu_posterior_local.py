"""GPU suite of the posterior covariance of every cell with its neighbours (csrc/posterior_local_kernel.hip, gsm_posterior_local,
mcmc_gpu_amd/posterior.py `local`): the pass through the engine against the extended-precision restatement within the a-priori
bound, the border and NaN rules, every reach on grids of one and of several tiles, both state types, the cut of the chain axis, the
C entry, and the run_many and largeScaleChain_mp paths.  Definitions, cases and the bound: tests/posterior_local_common.py."""
import ctypes as C

import numpy as np
import pytest

import posterior_local_common as lc
from mcmc_gpu_amd import MCMC_gpu, driver, posterior, synthetic
from test_gpu_posterior import _stretched_snapshots, _template_with_points

pytestmark = pytest.mark.gpu


def _n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _cross(x, g, R, state, calls=1):
    """cross [K, H, W] after `calls` calls of eng.posterior_local on the beds x [Cn, H, W], from zeros."""
    import torch
    from mcmc_gpu_amd.engine import GsmEngine
    Cn, H, W = x.shape
    eng = GsmEngine(H, W, Cn, state_dtype=state)
    try:
        eng.beds = torch.as_tensor(x).to(device=eng.dev, dtype=eng.state_dtype)
        dg = torch.as_tensor(np.ascontiguousarray(g)).to(eng.dev)
        cross = torch.zeros((2 * R * R + 2 * R, H, W), dtype=torch.float64, device=eng.dev)
        for _ in range(calls):
            eng.posterior_local(dg, R, cross)
        return cross.cpu().numpy()
    finally:
        eng.close()


@pytest.mark.parametrize("H,W,R,Cn,state", lc.FEW)
def test_few_chains_one_per_part(H, W, R, Cn, state):
    """Every grid and reach with one chain per part: the bound on every entry, exact zeros where the partner is outside the grid,
    two calls add, and the same bits twice."""
    plan = lc.split_plan(H, W, R, Cn, _n_cu())
    assert plan["cpp"] == 1 and plan["parts"] == Cn, f"{H}x{W} reach {R} x {Cn} chains on {_n_cu()} compute units gives {plan}"
    x, g = lc.case_beds(H, W, R, Cn, state, [])
    label = f"{H}x{W} R={R} C={Cn} {state}"
    once = _cross(x, g, R, state)
    lc.check(once, x, g, R, label)
    if H == 3:                                                       # (3, 9) at reach 4: the offsets with di >= 3 never pair
        dead = [k for k, (di, dj) in enumerate(lc.offsets(R)) if di >= 3]
        assert len(dead) == 18 and (once[dead] == 0).all() and not lc.inside(H, W, R)[dead].any()
    twice = _cross(x, g, R, state, calls=2)
    lc.check(twice, x, g, R, label + ", two calls", scale=2)
    assert np.array_equal(twice, 2 * once)                           # the same sum added to itself: a doubling is exact
    assert np.array_equal(_cross(x, g, R, state), once)              # chains in index order, parts in part order: the same bits


@pytest.mark.parametrize("H,W,R,Cn,state", list(lc.MANY))
def test_many_chains_per_part(H, W, R, Cn, state):
    """Many chains per workgroup: multi-trip chain loops with a short last group, ragged last parts and empty parts."""
    plan = lc.split_plan(H, W, R, Cn, _n_cu())
    print(f"local split plan {H}x{W} reach {R} x {Cn} chains on {_n_cu()} CUs: {plan}")
    assert (plan["parts"], plan["cpp"], plan["last"], plan["empty"]) == lc.MANY[(H, W, R, Cn, state)], \
        f"{H}x{W} reach {R} x {Cn} chains on {_n_cu()} compute units gives {plan}, not the regime this case is here for"
    x, g = lc.case_beds(H, W, R, Cn, state, [])
    once = _cross(x, g, R, state)
    lc.check(once, x, g, R, f"{H}x{W} R={R} C={Cn} {state}")
    assert np.array_equal(_cross(x, g, R, state), once)


@pytest.mark.parametrize("H,W,R,Cn,state,cells", lc.WITH_NAN)
def test_nan_bed_reaches_exactly_its_pairs(H, W, R, Cn, state, cells):
    """The last chain's bed is NaN at an interior cell and at a corner: exactly the entries that pair those cells are NaN, the entries
    whose partner is outside the grid stay 0 (also those of the NaN corner), all others meet the bound."""
    x, g = lc.case_beds(H, W, R, Cn, state, cells)
    got = _cross(x, g, R, state)
    exp_nan = lc.nan_entries(H, W, R, cells)
    assert exp_nan.sum() > 2 * R and not (exp_nan & ~lc.inside(H, W, R)).any()
    assert np.array_equal(np.isnan(got), exp_nan)
    lc.check(got, x, g, R, f"NaN at {cells} {H}x{W} R={R} C={Cn} {state}")


def test_c_entry_refusals_leave_cross_untouched():
    import torch
    from mcmc_gpu_amd.engine import GsmEngine, _ptr
    H, W, Cn, R = 33, 130, 5, 2
    x, g = lc.beds(H, W, Cn, 3, False)
    eng = GsmEngine(H, W, Cn)
    try:
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(eng.dev)
        b, dg = dev(x), dev(g)
        cross = torch.full((12, H, W), 7.0, dtype=torch.float64, device=eng.dev)
        null, st = C.c_void_p(0), eng._stream()
        lib, E_ARG = eng.lib, -1
        off8 = C.c_void_p(b.data_ptr() + 8)
        refused = [((null, _ptr(dg), R, _ptr(cross)), b"NULL"), ((_ptr(b), null, R, _ptr(cross)), b"NULL"), ((_ptr(b), _ptr(dg), R, null), b"NULL"),
                   ((_ptr(b), _ptr(dg), 0, _ptr(cross)), b"reach"), ((_ptr(b), _ptr(dg), 5, _ptr(cross)), b"reach"),
                   ((_ptr(b), _ptr(dg), -1, _ptr(cross)), b"reach"), ((off8, _ptr(dg), R, _ptr(cross)), b"aligned")]
        for args, word in refused:
            assert lib.gsm_posterior_local(eng.h, *args, st) == E_ARG, args
            assert word in lib.gsm_last_error(eng.h), (word, lib.gsm_last_error(eng.h))
        torch.cuda.synchronize()
        assert (cross == 7.0).all()                                  # nothing was written
        assert lib.gsm_posterior_local(eng.h, _ptr(b), _ptr(dg), R, _ptr(cross), st) == 0        # ADDED to: 7 + the sums
        got = cross.cpu().numpy()
        ins = lc.inside(H, W, R)
        assert (got[~ins] == 7.0).all()                              # an entry whose partner is outside the grid keeps what it held
        X, mag = lc.reference(x, g, R)
        err = np.abs(got[ins].astype(lc.LD) - (7.0 + X[ins]))
        assert (err <= (Cn + 4) * lc.U * (7.0 + mag[ins])).all()
        eng.beds = b
        for bad in (0, 5, 2.0, True):                                # the engine method checks its arguments first
            with pytest.raises(ValueError, match="reach"):
                eng.posterior_local(dg, bad, cross)
        with pytest.raises(ValueError, match="cross"):
            eng.posterior_local(dg, 3, cross)
        with pytest.raises(ValueError, match="g must"):
            eng.posterior_local(dg[:-1].contiguous(), R, cross)
        with pytest.raises(ValueError, match="float64"):
            eng.posterior_local(dg, R, cross.float())
    finally:
        eng.close()


@pytest.mark.parametrize("state,split,rhat", [("f64", True, True), ("f32", False, False)])
def test_accumulator_takes_the_moment_snapshots(state, split, rhat):
    """PosteriorAccumulator.add() calls the pass for exactly the snapshots the moment sums take: with split and T = 9 the first
    snapshot is dropped (a NaN there touches nothing).  Beside every other option."""
    import torch
    from mcmc_gpu_amd.engine import GsmEngine
    H, W, Cn, T, R = 33, 130, 4, 9, 2
    rng = np.random.default_rng(5)
    x = (-300.0 + 100.0 * rng.normal(size=(Cn, T, H, W)) + 60.0 * rng.normal(size=(Cn, T, 1, 1))).astype(np.float32).astype(np.float64)
    g = -300.0 + 10.0 * rng.normal(size=(H, W))
    lo = T - 2 * (T // 2) if split else 0
    if lo:
        x[1, 0, 7, 9] = np.nan
    eng = GsmEngine(H, W, Cn, state_dtype=state)
    try:
        opts = dict(hist=dict(half_width=400.0), cov=dict(probes=posterior.point_probes(H, W, [5]))) if rhat else {}
        acc = posterior.PosteriorAccumulator(eng, T, 0, 1, split=split, rhat=rhat, common_ref=g, local=dict(reach=R), **opts)
        assert acc.local_cross.shape == (12, H, W) and acc.local_cross.dtype == torch.float64
        held = {k: v for k, v in vars(acc).items() if isinstance(v, torch.Tensor)}
        assert acc.device_bytes == sum(v.nbytes for v in held.values())                   # local_cross is in the memory budget
        eng.beds = torch.empty((Cn, H, W), dtype=eng.state_dtype, device=eng.dev)
        for t in range(T):
            eng.beds.copy_(torch.as_tensor(x[:, t]))
            acc.add()
        assert set(acc.local_sums()) >= {"partials_sum", "M", "local_cross"}
        s = acc.finalize()
    finally:
        eng.close()
    assert s.local_reach == R and np.array_equal(s.local_centre, g) and s.local_cross.shape == (12, H, W)
    used = x[:, lo:].reshape(Cn * (T - lo), H, W)
    assert used.shape[0] == s.n_sequences * s.n_per_sequence
    lc.check(s.local_cross, used, g, R, f"accumulator split={split} rhat={rhat} {state}")
    cov = s.local_covariance()
    dev = used - used.mean(axis=0)
    for k, (di, dj) in enumerate(lc.offsets(R)):
        (ci, cj), (pi, pj) = lc.pair_slices(H, W, di, dj)
        exp = (dev[:, ci, cj] * dev[:, pi, pj]).sum(axis=0) / (used.shape[0] - 1)
        # the tolerances of the variances (posterior_common): the same expression at another offset
        assert (np.abs(cov[k][ci, cj] - exp) <= 1e-9 * s.sd[ci, cj] * s.sd[pi, pj] + 1e-9).all(), (di, dj)


def test_run_many_end_to_end():
    """64 x 64, 8 chains, 201 iterations, thin=10, reach 2: local_cross equals the statistic of the snapshots of a run stopped at
    them; beds, accepts and all other maps are bit-identical with and without `local`; the chains' neighbours go together (the median
    lag-1 correlation inside the update region is positive: 0.0005 on the MI355X -- after 200 iterations the independent N(0, 5)
    noise the chains start from still carries most of the spread between them)."""
    prob, ch, rf, ij = _template_with_points()
    beds, seeds, n_iter, R = synthetic.initial_beds(prob, 8), list(range(21, 29)), 201, 2
    H, W = beds.shape[1:]
    opt = dict(burn_in=0, thin=10, hist=dict(half_width=400.0), ess=dict(max_lag=3), cov=dict(probes=posterior.point_probes(H, W, [30 * W + 30])),
               residual=True)
    plain, without = MCMC_gpu.run_many(ch, rf, beds, seeds, n_iter, batch=8, posterior=opt)
    res, s = MCMC_gpu.run_many(ch, rf, beds, seeds, n_iter, batch=8, posterior=dict(opt, local=dict(reach=R)))
    assert len(res) == len(plain) == 8
    for ra, rb in zip(res, plain):
        assert len(ra) == len(rb) and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(ra, rb))
    assert without.local_cross is None and without.local_reach is None and without.local_centre is None
    for name in ("mean", "sd", "rhat", "within_var", "between_var_over_n", "sample_values", "snapshot_iterations", "sample_loc", "hist_counts",
                 "level_counts", "lag_sqdiff", "probe_values", "probe_cross", "residual_sums"):
        assert np.array_equal(getattr(s, name), getattr(without, name), equal_nan=True), name
    assert s.local_reach == R and s.local_cross.shape == (12, H, W) and (s.n_sequences, s.n_per_sequence) == (16, 10)
    its = posterior.snapshot_iterations(n_iter, 0, 10)
    assert its.size == 21
    x = _stretched_snapshots(ch, rf, beds, seeds, its)               # [8, 21, H, W]: the first snapshot belongs to no sequence
    used = x[:, 1:].reshape(8 * 20, H, W)
    lc.check(s.local_cross, used, s.local_centre, R, "run_many 64x64 x 8, 20 snapshots")
    slope = s.gradient_sd(prob["resolution"])                         # reach 2 carries the central differences
    assert all(v.shape == (H, W) and np.nanmin(v) >= 0 for v in slope) and s.block_mean_sd(3).shape == (H - 2, W - 2)
    # physics: a block update moves neighbouring cells together
    region = prob["region_mask"] == 1
    rho = s.local_correlation()
    lag1 = np.concatenate([rho[0][region], rho[2 * R][region]])      # offsets (0, 1) and (1, 0)
    med = float(np.median(lag1[~np.isnan(lag1)]))
    assert med > 0, f"median lag-1 local correlation inside the update region is {med!r}, expected positive"
    print(f"median lag-1 local correlation inside the update region: {med:.4f}")
    with pytest.raises(ValueError, match="local"):
        MCMC_gpu.run_many(ch, rf, beds, seeds, n_iter, batch=8, posterior=dict(burn_in=0, thin=10, local=dict(reach=5)))


def test_driver_writes_the_fields(tmp_path):
    prob, ch, rf, ij = _template_with_points()
    ch.set_rng_mode("philox")
    seeds, beds = [31, 32, 33], list(synthetic.initial_beds(prob, 3))
    H, W = beds[0].shape
    opt = dict(burn_in=20, thin=10, local=True)
    driver.largeScaleChain_mp(3, 2, ch, rf, beds, seeds, [120] * 3, output_path=str(tmp_path), mode="philox", n_gpus=1, posterior=opt)
    got = posterior.PosteriorSummary.load(tmp_path / "LargeScaleChain" / "posterior_0k.npz")
    _, exp = MCMC_gpu.run_many(ch, rf, np.stack(beds), seeds, 120, batch=8, posterior=opt)
    assert got.local_reach == 1 and got.local_cross.shape == (4, H, W)
    for name in ("local_cross", "local_centre", "mean", "sd"):
        assert np.array_equal(getattr(got, name), getattr(exp, name), equal_nan=True), name
    for name in ("local_covariance", "local_correlation"):
        assert np.array_equal(getattr(got, name)(), getattr(exp, name)(), equal_nan=True), name
    assert np.array_equal(got.block_mean_sd(2), exp.block_mean_sd(2), equal_nan=True)
    with pytest.raises(ValueError, match="reach"):
        got.gradient_sd(500.0)
