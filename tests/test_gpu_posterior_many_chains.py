"""GPU suite of the posterior accumulator with MANY chains per workgroup (csrc/posterior_kernel.hip, gsm_api_posterior.hip).

The chain axis is cut into parts = min(ceil(4 n_cu / cell_blocks), n_chains) of cpp = ceil(n_chains / parts) chains.  With the 3
to 8 chains of tests/test_gpu_posterior.py every part holds ONE chain: the loop of post_pooled_kernel that keeps four chains in
flight and the chain loop of post_partials_kernel run at most one trip, no part is ragged or empty, and the grid-stride loop
of post_accumulate_kernel takes one trip.  Here the chain count alone moves the kernels into the regimes a production run
(1024 chains of 256 x 256: cpp = 128, 32 grid-stride trips) executes; pc.split_plan restates the split rule and every test
asserts the regime it claims BEFORE it feeds anything, so on a device with another number of compute units the tests fail
with the plan in the message (choose the chain counts with pc.split_plan then) instead of quietly running cpp == 1.
Definitions, data and tolerances: tests/posterior_common.py."""
import numpy as np
import pytest

import posterior_common as pc
from mcmc_gpu_amd import MCMC_gpu, posterior, synthetic
from test_gpu_posterior import _stretched_snapshots, _template_with_points

pytestmark = pytest.mark.gpu

U = 2.0 ** -53

# (H, W, chains, states, values rounded to float): the regimes below are those of a device with 256 compute units.  The f64 and
# f32 runs of one grid share their snapshots and their reference, which therefore hold float values; the last row is fp64 only
# and keeps all 53 bits.
GRIDS = [
    (128, 128, 390, ("f32", "f64"), True),
    (126, 129, 200, ("f32",), True),
    (127, 129, 101, ("f64", "f32"), True),
    (127, 129, 135, ("f64",), False),
]
CASES = [(H, W, Cn, st, f32) for H, W, Cn, states, f32 in GRIDS for st in states]
# in the order that lets one (grid, T) serve both state types
RUNS = [(H, W, Cn, st, f32, T) for H, W, Cn, states, f32 in GRIDS for T in (4, 5) for st in states]
# what each case must reach: (pooled, partials) as (vec, parts, cpp, last, empty) and accumulate as (trips, last_trip_blocks < grid,
# a later trip ends in a workgroup with dead lanes, tail)
REGIME = {
    (128, 128, 390, "f32"): ((4, 64, 7, 5, 8), (1, 16, 25, 15, 0), (2, True, False, 0)),     # one unrolled trip + 3; last 4 + 1; 1.5 trips
    (128, 128, 390, "f64"): ((2, 32, 13, 13, 2), (1, 16, 25, 15, 0), (4, True, False, 0)),   # three unrolled trips + 1; 3 trips + a part
    (126, 129, 200, "f32"): ((2, 32, 7, 4, 3), (1, 16, 13, 5, 0), (1, False, False, 0)),     # pooled_t<float, 2>; last part: unrolled trip only
    (127, 129, 101, "f64"): ((1, 16, 7, 3, 1), (1, 16, 7, 3, 1), (1, False, False, 1)),      # last part: remainder loop only; tail 1
    (127, 129, 101, "f32"): ((1, 16, 7, 3, 1), (1, 16, 7, 3, 1), (1, False, False, 3)),      # tail 3
    (127, 129, 135, "f64"): ((1, 16, 9, 9, 1), (1, 16, 9, 9, 1), (2, True, True, 1)),        # the second trip ends in a workgroup with dead lanes
}


def _n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _plan(H, W, Cn, state):
    return pc.split_plan(H, W, Cn, state == "f32", _n_cu())


def _regime_of(plan):
    a = plan["accumulate"]
    form = lambda f: tuple(plan[f][k] for k in ("vec", "parts", "cpp", "last", "empty"))
    return (form("pooled"), form("partials"),
            (a["trips"], a["last_trip_blocks"] < a["grid"], a["trips"] > 1 and a["last_block_groups"] < 512, a["tail"]))


def _assert_regime(H, W, Cn, state):
    plan = _plan(H, W, Cn, state)
    print(f"split plan {H}x{W} x {Cn} chains {state} on {_n_cu()} CUs: {plan}")
    assert _regime_of(plan) == REGIME[(H, W, Cn, state)], \
        f"{H}x{W} x {Cn} chains ({state}) on {_n_cu()} compute units gives {plan}, not the regime this case is here for"
    return plan


def test_cases_cover_the_split_regimes():
    """Over the set of cases, on THIS device: every loop shape of the three kernels that depends on the chain count."""
    plans = [_assert_regime(H, W, Cn, state) for H, W, Cn, state, _ in CASES]
    pooled, partials, acc = ([p[k] for p in plans] for k in ("pooled", "partials", "accumulate"))
    assert any(p["cpp"] >= 8 for p in pooled)                                   # two or more trips of the four-chain loop
    assert any(p["cpp"] % 4 != 0 and p["cpp"] > 4 for p in pooled)              # unrolled trips followed by the remainder loop
    assert any(p["last"] >= 4 and p["last"] % 4 != 0 and p["last"] < p["cpp"] for p in pooled)   # ragged last part: 4 + remainder
    assert any(p["last"] >= 4 and p["last"] % 4 == 0 and p["last"] < p["cpp"] for p in pooled)   # ragged last part: unrolled trip only
    assert any(p["last"] < 4 for p in pooled) and any(p["last"] < p["cpp"] for p in partials)    # remainder loop only; ragged partials
    assert any(p["empty"] >= 1 for p in pooled) and any(p["empty"] >= 1 for p in partials)
    assert any(p["cpp"] % 2 == 1 and p["cpp"] >= 3 for p in partials)           # the loop unrolled by 2 ends on a single chain
    assert any(a["trips"] >= 2 and a["last_trip_blocks"] < a["grid"] for a in acc)
    assert any(a["trips"] >= 2 and a["last_block_groups"] < 512 for a in acc)           # live[u] false inside a later trip
    assert {1, 3} <= {a["tail"] for a in acc}
    assert {(p["vec"], st) for p, (_, _, _, st, _) in zip(pooled, CASES)} >= {(4, "f32"), (2, "f32"), (1, "f32"), (2, "f64"), (1, "f64")}


_DATA = {}


def _data(H, W, Cn, T, f32):
    """Snapshots, common field, references and device copies of one (grid, chains, T): built once, kept until the next one is asked for."""
    key = (H, W, Cn, T, f32)
    if _DATA.get("key") != key:
        _DATA.clear()
        x, g = pc.many_chain_data(Cn, T, H, W, H * 100 + T, f32=f32)
        _DATA.update(key=key, x=x, g=g, ref={}, ext={}, dev={})
    return _DATA


def _reference(d, split):
    if split not in d["ref"]:
        d["ref"][split] = pc.posterior_reference(d["x"], split)
    return d["ref"][split]


def _device(d, state):
    import torch
    if state not in d["dev"]:
        d["dev"].clear()
        d["dev"][state] = torch.as_tensor(d["x"]).to(device="cuda:0", dtype=torch.float64 if state == "f64" else torch.float32)
    return d["dev"][state]


def _feed(dx, g, state_dtype, split, rhat, cells):
    """The snapshots dx [C, T, H, W] (on the device, state dtype) through PosteriorAccumulator.add() as test_gpu_posterior._feed
    feeds them (no chain is run: the engine's beds are set); returns the summary and the raw partials."""
    import torch
    from mcmc_gpu_amd.engine import GsmEngine
    Cn, T, H, W = dx.shape
    eng = GsmEngine(H, W, Cn, state_dtype=state_dtype)
    try:
        acc = posterior.PosteriorAccumulator(eng, T, 0, 1, split=split, rhat=rhat, common_ref=g, sample_cells=cells)
        eng.beds = torch.empty((Cn, H, W), dtype=eng.state_dtype, device=eng.dev)
        for t in range(T):
            eng.beds.copy_(dx[:, t])
            acc.add()
        with pytest.raises(RuntimeError):
            acc.add()
        return acc.finalize(), acc.partials().cpu().numpy()
    finally:
        eng.close()


@pytest.mark.parametrize("rhat", [True, False])
@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("H,W,Cn,state_dtype,f32,T", RUNS)
def test_many_chains_against_numpy(H, W, Cn, state_dtype, f32, T, split, rhat):
    _assert_regime(H, W, Cn, state_dtype)
    d = _data(H, W, Cn, T, f32)
    x, g, ref = d["x"], d["g"], _reference(d, split)
    cells = np.array([0, 5 * W + 7, H * W - 1])
    label = f"{H}x{W} C={Cn} T={T} {state_dtype} split={split} rhat={rhat}"
    s, P = _feed(_device(d, state_dtype), g, state_dtype, split, rhat, cells)
    pc.check_maps(s, ref, rhat=rhat, label=label)
    assert np.isnan(s.mean[5, 7]) and np.isnan(s.sd[5, 7]) and np.isnan(s.mean).sum() == 1
    assert (s.n_chains, s.n_sequences, s.n_per_sequence) == (Cn, ref["M"], ref["N"]) == (Cn, Cn * (2 if split else 1), T // 2 if split else T)
    assert s.sample_values.shape == (Cn, 3, T)          # at 390 chains post_sample_kernel runs on more than one workgroup
    assert np.array_equal(s.sample_values, x.reshape(Cn, T, H * W)[:, :, cells].transpose(0, 2, 1), equal_nan=True)
    if rhat:
        const = pc.constant_cells(H, W, split)          # sums of zeros over many chains and parts stay zero
        assert np.isnan(s.rhat[5, 7]) and np.isnan(s.within_var[5, 7]) and np.isnan(s.between_var_over_n[5, 7])
        assert (s.within_var[const] == 0).all() and np.isnan(s.rhat[const]).all()
        assert np.isfinite(s.rhat[~const]).sum() == H * W - const.sum() - 1
    else:
        assert s.rhat is None and s.within_var is None
        # The raw sums against extended precision.  P0 adds n values fl(x - g) (one rounding each) in some order of n - 1 additions:
        # |P0 - sum d| <= (n + 2) u sum|d|; a term of P1 carries two roundings of d and one of the product: (n + 4) u sum d^2.
        if split not in d["ext"]:
            d["ext"][split] = pc.extended_pooled_sums(x, split, g)
        sd, sabs, sq, n = d["ext"][split]
        assert n == ref["M"] * ref["N"]
        ok = ~np.isnan(sd)
        assert np.array_equal(np.isnan(P[0]), ~ok) and np.array_equal(np.isnan(P[1]), ~ok) and (~ok).sum() == 1 and (P[2] == 0).all()
        e0 = np.abs(P[0].astype(np.longdouble) - sd)[ok] / ((n + 2) * U * sabs[ok])
        e1 = np.abs(P[1].astype(np.longdouble) - sq)[ok] / ((n + 4) * U * sq[ok])
        print(f"pooled sums {label}: largest |P0 - sum d| {float(e0.max()):.3e}, |P1 - sum d^2| {float(e1.max()):.3e} of the a-priori bounds")
        assert e0.max() <= 1 and e1.max() <= 1
    # sums over chains are taken in index order and the parts in part order: a second pass gives the same bits
    s2, P2 = _feed(_device(d, state_dtype), g, state_dtype, split, rhat, cells)
    assert np.array_equal(P, P2, equal_nan=True)
    assert np.array_equal(s.mean, s2.mean, equal_nan=True) and np.array_equal(s.sd, s2.sd, equal_nan=True)


def test_run_many_posterior_end_to_end_many_chains():
    """150 chains of the 64 x 64 template: two chains per part in the pooled form, three in the partials form, empty parts in both."""
    Cn, n_iter, burn_in, thin = 150, 61, 11, 5
    plan = _plan(64, 64, Cn, "f64")
    print(f"split plan 64x64 x {Cn} chains f64 on {_n_cu()} CUs: {plan}")
    assert plan["pooled"]["cpp"] >= 2 and plan["partials"]["cpp"] >= 3 and plan["partials"]["cpp"] % 2 == 1, plan
    assert plan["pooled"]["empty"] >= 1 and plan["partials"]["empty"] >= 1, plan
    prob, ch, rf, ij = _template_with_points()
    beds, seeds = synthetic.initial_beds(prob, Cn), list(range(1000, 1000 + Cn))
    its = posterior.snapshot_iterations(n_iter, burn_in, thin)
    assert its.size == 10
    x = _stretched_snapshots(ch, rf, beds, seeds, its)
    assert x.shape == (Cn, 10, 64, 64)
    plain = MCMC_gpu.run_many(ch, rf, beds, seeds, n_iter, batch=8)
    ref = pc.posterior_reference(x, True)
    for rhat in (True, False):
        res, s = MCMC_gpu.run_many(ch, rf, beds, seeds, n_iter, batch=8, posterior=dict(burn_in=burn_in, thin=thin, split=True, rhat=rhat))
        assert len(res) == len(plain) == Cn
        for ra, rb in zip(res, plain):
            assert len(ra) == len(rb) and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(ra, rb))
        pc.check_maps(s, ref, rhat=rhat, label=f"end to end {Cn} chains rhat={rhat}")
        assert np.array_equal(s.snapshot_iterations, its) and (s.burn_in, s.thin, s.split) == (burn_in, thin, True)
        assert (s.n_chains, s.n_sequences, s.n_per_sequence) == (Cn, 2 * Cn, 5)
        assert np.array_equal(s.sample_values, x[:, :, ij[:, 0], ij[:, 1]].transpose(0, 2, 1))
        if rhat:
            seq = pc.sequences(x, True)
            still = (seq == seq[:, :1]).all(axis=(0, 1))
            assert still[2, 3] and not still[30, 30]
            assert np.isnan(s.rhat[still]).all() and np.isfinite(s.rhat[~still]).all()
            assert (s.within_var[still] == 0).all()
