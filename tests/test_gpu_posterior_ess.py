"""GPU suite of the posterior's lagged sums and effective sample size (csrc/posterior_lag_kernel.hip, gsm_posterior_lagged,
mcmc_gpu_amd/posterior.py `ess`): the kernel against the extended-precision restatement within the a-priori bound, its ring
(wrap, reset between the halves, a dropped snapshot), its vector widths and its split of the chain axis, the run_many and
largeScaleChain_mp paths, two handles, and the C entry's refusals.  Definitions and the bound: tests/posterior_ess_common.py."""
import ctypes as C

import numpy as np
import pytest

import posterior_common as pc
import posterior_ess_common as ec
from mcmc_gpu_amd import MCMC_gpu, driver, posterior, synthetic
from test_gpu_posterior import _stretched_snapshots, _template_with_points

pytestmark = pytest.mark.gpu


def _n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _feed(x, g, state_dtype, split, K):
    """x [C, T, H, W] fed snapshot by snapshot through PosteriorAccumulator.add() (no chain is run: the engine's beds are set);
    returns the summary."""
    import torch
    from mcmc_gpu_amd.engine import GsmEngine
    Cn, T, H, W = x.shape
    eng = GsmEngine(H, W, Cn, state_dtype=state_dtype)
    try:
        acc = posterior.PosteriorAccumulator(eng, T, 0, 1, split=split, rhat=True, common_ref=g, ess=dict(max_lag=K))
        assert acc.ring.shape == (K, Cn, H * W) and acc.ring.dtype == eng.state_dtype and acc.lag_sqdiff.shape == (K, H, W)
        eng.beds = torch.empty((Cn, H, W), dtype=eng.state_dtype, device=eng.dev)
        for t in range(T):
            eng.beds.copy_(torch.as_tensor(x[:, t]))
            acc.add()
        assert acc.ring is None                                  # released with the last snapshot
        with pytest.raises(RuntimeError):
            acc.add()
        return acc.finalize()
    finally:
        eng.close()


def _small_data(H, W, Cn, T, f32):
    """The draws of test_gpu_posterior.test_kernels_against_numpy: a block constant within every chain, a block constant within
    each half of every chain, one NaN at a single (chain, snapshot, cell)."""
    rng = np.random.default_rng(H * 100 + T)
    x = -300.0 + 100.0 * rng.normal(size=(Cn, T, H, W))
    x[:, :, 10:14, 10:20] = x[:, :1, 10:14, 10:20]
    half = T - T // 2
    x[:, :half, 20:22, 5:9] = x[:, :1, 20:22, 5:9]
    x[:, half:, 20:22, 5:9] = x[:, half:half + 1, 20:22, 5:9]
    x[2, T - 2, 5, 7] = np.nan
    g = -300.0 + 10.0 * rng.normal(size=(H, W))
    if f32:
        x = x.astype(np.float32).astype(np.float64)              # the reference sees the same f32 values, cast to f64
    return x, g


def _check_ess_against_loop(s, label):
    """ess(), truncated, mcse() and autocorrelation() of the summary against the cell loop on the summary's own maps."""
    M, N = s.n_sequences, s.n_per_sequence
    rho_e, ess_e, trunc_e, mcse_e, _ = ec.ess_loop(s.lag_sqdiff, s.within_var, s.between_var_over_n, s.mean, s.sd, M, N)
    ess, trunc = s.ess()
    for got, exp, name in ((s.autocorrelation(), rho_e, "rho"), (ess, ess_e, "ess"), (s.mcse(), mcse_e, "mcse")):
        assert np.array_equal(np.isnan(got), np.isnan(exp)), (label, name)
        np.testing.assert_allclose(got, exp, rtol=1e-13, atol=0, err_msg=f"{label} {name}")
    assert np.array_equal(trunc, trunc_e), label
    assert np.array_equal(np.isnan(ess), np.isnan(s.rhat)), label  # NaN where W == 0 and where the cell saw a NaN: rhat's NaN set
    return ess, trunc


@pytest.mark.parametrize("state_dtype", ["f64", "f32"])
@pytest.mark.parametrize("split,T,K", [(True, 8, 3), (True, 9, 3), (False, 9, 7), (False, 9, 1), (False, 12, 9)])
def test_small_grid_against_the_restatement(split, T, K, state_dtype):
    """37 x 41: an odd plane (scalar loads and a tail workgroup).  split, T = 8, K = 3: K = N - 1 and the ring is reset between the
    halves; T = 9: the first snapshot is dropped; unsplit, T = 9, K = 7: the ring wraps.  K = 1 and K = 9: fewer lags than the
    kernel's instantiation holds (3 and 15), a ring of one slot, and a ring of 9 that wraps."""
    H, W, Cn = 37, 41, 5
    x, g = _small_data(H, W, Cn, T, state_dtype == "f32")
    label = f"{H}x{W} C={Cn} T={T} K={K} split={split} {state_dtype}"
    s = _feed(x, g, state_dtype, split, K)
    M, N = (2 * Cn, T // 2) if split else (Cn, T)
    assert (s.n_sequences, s.n_per_sequence) == (M, N) and s.lag_sqdiff.shape == (K, H, W) and K <= N - 1
    ref = ec.lag_sqdiff_reference(x, split, K)
    ec.check_lag_sqdiff(s.lag_sqdiff, ref, M, N, label)
    assert np.isnan(s.lag_sqdiff[:, 5, 7]).any() and np.isnan(s.lag_sqdiff).any(axis=0).sum() == 1
    const = np.zeros((H, W), dtype=bool)
    const[10:14, 10:20] = True
    const[20:22, 5:9] = split                                    # constant within each half: no pair straddles the halves
    assert (s.lag_sqdiff[:, const] == 0).all() and (s.lag_sqdiff[:, ~const] != 0).all()
    pc.check_maps(s, pc.posterior_reference(x, split), label=label)
    ess, trunc = _check_ess_against_loop(s, label)
    assert np.isnan(ess[const]).all() and np.isnan(ess[5, 7]) and np.isfinite(ess[~const]).sum() == H * W - const.sum() - 1
    # chains in index order inside a part, parts in part order: a second pass gives the same bits
    s2 = _feed(x, g, state_dtype, split, K)
    assert np.array_equal(s.lag_sqdiff, s2.lag_sqdiff, equal_nan=True)


@pytest.mark.parametrize("state_dtype", ["f64", "f32"])
def test_fifteen_lags(state_dtype):
    """K = 15, the register-heaviest instantiation, at 16 bytes per lane with either state type."""
    H, W, Cn, T, K = 64, 64, 6, 17, 15
    x, g = _small_data(H, W, Cn, T, state_dtype == "f32")
    plan = ec.lag_split_plan(H, W, Cn, state_dtype == "f32", _n_cu())
    assert plan["vec"] == (4 if state_dtype == "f32" else 2), plan
    s = _feed(x, g, state_dtype, False, K)
    label = f"{H}x{W} C={Cn} T={T} K={K} {state_dtype}"
    ec.check_lag_sqdiff(s.lag_sqdiff, ec.lag_sqdiff_reference(x, False, K), Cn, T, label)
    assert (s.lag_sqdiff[:, 10:14, 10:20] == 0).all()
    _check_ess_against_loop(s, label)


# (H, W, chains, state): grids and chain counts of tests/test_gpu_posterior_many_chains.py; what each must reach on a device of 256
# compute units, as (vec, parts, cpp, last, empty)
MANY = {
    (128, 128, 390, "f32"): (4, 64, 7, 5, 8),
    (126, 129, 200, "f32"): (2, 32, 7, 4, 3),
    (127, 129, 101, "f64"): (1, 16, 7, 3, 1),
    (127, 129, 101, "f32"): (1, 16, 7, 3, 1),
}
_DATA = {}


def _many_data(H, W, Cn, T, K):
    """Snapshots and their reference for one grid: built once, shared by the state types, dropped when another grid is asked for."""
    key = (H, W, Cn, T, K)
    if _DATA.get("key") != key:
        _DATA.clear()
        x, g = pc.many_chain_data(Cn, T, H, W, H * 100 + T, f32=True)
        _DATA.update(key=key, x=x, g=g, ref=ec.lag_sqdiff_reference(x, False, K))
    return _DATA["x"], _DATA["g"], _DATA["ref"]


def _assert_regime(H, W, Cn, state):
    plan = ec.lag_split_plan(H, W, Cn, state == "f32", _n_cu())
    print(f"lag split plan {H}x{W} x {Cn} chains {state} on {_n_cu()} CUs: {plan}")
    assert tuple(plan[k] for k in ("vec", "parts", "cpp", "last", "empty")) == MANY[(H, W, Cn, state)], \
        f"{H}x{W} x {Cn} chains ({state}) on {_n_cu()} compute units gives {plan}, not the regime this case is here for"
    assert plan["cpp"] >= 5 and plan["last"] < plan["cpp"] and plan["empty"] >= 1, plan
    return plan


def test_cases_cover_the_kernel_forms():
    """Over the cases of this file, on THIS device: every vector width of either state type, many chains per workgroup with a
    ragged last part, and an empty part."""
    plans = {k: _assert_regime(*k) for k in MANY}
    widths = {(p["vec"], k[3]) for k, p in plans.items()}
    for H, W, Cn, st in ((37, 41, 5, "f64"), (37, 41, 5, "f32"), (64, 64, 6, "f64"), (64, 64, 6, "f32")):
        widths.add((ec.lag_split_plan(H, W, Cn, st == "f32", _n_cu())["vec"], st))
    assert widths >= {(4, "f32"), (2, "f32"), (1, "f32"), (2, "f64"), (1, "f64")}, widths


@pytest.mark.parametrize("H,W,Cn,state_dtype", list(MANY))
def test_many_chains_per_workgroup(H, W, Cn, state_dtype):
    T, K = 7, 5
    _assert_regime(H, W, Cn, state_dtype)
    x, g, ref = _many_data(H, W, Cn, T, K)
    s = _feed(x, g, state_dtype, False, K)
    label = f"{H}x{W} C={Cn} T={T} K={K} {state_dtype}"
    ec.check_lag_sqdiff(s.lag_sqdiff, ref, Cn, T, label)
    const = pc.constant_cells(H, W, False)
    assert (s.lag_sqdiff[:, const] == 0).all()                   # sums of zeros over many chains and parts stay zero
    assert np.isnan(s.lag_sqdiff).any(axis=0).sum() == 1 and np.isnan(s.lag_sqdiff[:, 5, 7]).any()


@pytest.mark.parametrize("split", [True, False])
def test_run_many_end_to_end(split):
    prob, ch, rf, ij = _template_with_points()
    beds, seeds, n_iter, burn_in, thin, K = synthetic.initial_beds(prob, 4), [5, 6, 7, 8], 61, 11, 5, 3
    its = posterior.snapshot_iterations(n_iter, burn_in, thin)
    assert its.size == 10
    x = _stretched_snapshots(ch, rf, beds, seeds, its)
    plain = MCMC_gpu.run_many(ch, rf, beds, seeds, n_iter, batch=8)
    opt = dict(burn_in=burn_in, thin=thin, split=split)
    _, without = MCMC_gpu.run_many(ch, rf, beds, seeds, n_iter, batch=8, posterior=opt)
    res, s = MCMC_gpu.run_many(ch, rf, beds, seeds, n_iter, batch=8, posterior=dict(opt, ess=dict(max_lag=K)))
    assert len(res) == len(plain) == 4
    for ra, rb in zip(res, plain):
        assert len(ra) == len(rb) and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(ra, rb))
    assert without.lag_sqdiff is None
    for name in ("mean", "sd", "rhat", "within_var", "between_var_over_n", "sample_values", "snapshot_iterations", "sample_loc"):
        assert np.array_equal(getattr(s, name), getattr(without, name), equal_nan=True), name
    M, N = (8, 5) if split else (4, 10)
    assert (s.n_sequences, s.n_per_sequence) == (M, N)
    label = f"end to end split={split}"
    ec.check_lag_sqdiff(s.lag_sqdiff, ec.lag_sqdiff_reference(x, split, K), M, N, label)
    seq = pc.sequences(x, split)
    still = (seq == seq[:, :1]).all(axis=(0, 1))
    assert still[2, 3] and not still[30, 30] and (s.lag_sqdiff[:, still] == 0).all()
    ess, trunc = _check_ess_against_loop(s, label)
    assert np.isnan(ess[still]).all() and np.isfinite(ess[~still]).all() and (ess[~still] > 0).all()
    with pytest.raises(ValueError, match="max_lag"):
        MCMC_gpu.run_many(ch, rf, beds, seeds, n_iter, batch=8, posterior=dict(opt, ess=dict(max_lag=2 * N - 1)))
    with pytest.raises(ValueError, match="rhat"):
        MCMC_gpu.run_many(ch, rf, beds, seeds, n_iter, batch=8, posterior=dict(opt, rhat=False, ess=True))


def test_two_handles_add(tmp_path):
    """Chains [0:a] and [a:] in two handles: their lagged sums add to the one-handle result; the driver writes lag_sqdiff."""
    H, W, Cn, T, K, a = 37, 41, 5, 9, 3, 2
    x, g = _small_data(H, W, Cn, T, False)
    one = _feed(x, g, "f64", True, K)
    two = _feed(x[:a], g, "f64", True, K).lag_sqdiff + _feed(x[a:], g, "f64", True, K).lag_sqdiff
    M, N = 2 * Cn, T // 2
    ref = ec.lag_sqdiff_reference(x, True, K)
    ec.check_lag_sqdiff(two, ref, M, N, "two handles")
    ec.check_lag_sqdiff(one.lag_sqdiff, ref, M, N, "one handle")
    # the ring's memory is counted before anything is allocated
    import torch
    from mcmc_gpu_amd.engine import GsmEngine
    eng = GsmEngine(H, W, Cn)
    try:
        base = posterior.PosteriorAccumulator(eng, T, 0, 1, common_ref=g)
        del base
        real = torch.cuda.mem_get_info
        with pytest.MonkeyPatch.context() as m:
            m.setattr(torch.cuda, "mem_get_info", lambda *a_, **k: (5 * Cn * H * W * 8 + K * Cn * H * W * 8, real(*a_, **k)[1]))
            posterior.PosteriorAccumulator(eng, T, 0, 1, common_ref=g)               # fits without the ring
            with pytest.raises(MemoryError):
                posterior.PosteriorAccumulator(eng, T, 0, 1, common_ref=g, ess=dict(max_lag=K))
    finally:
        eng.close()
    prob, ch, rf, ij = _template_with_points()
    ch.set_rng_mode("philox")
    seeds, beds = [31, 32, 33], list(synthetic.initial_beds(prob, 3))
    opt = dict(burn_in=20, thin=10, ess=dict(max_lag=3))
    driver.largeScaleChain_mp(3, 2, ch, rf, beds, seeds, [120] * 3, output_path=str(tmp_path), mode="philox", n_gpus=1, posterior=opt)
    got = posterior.PosteriorSummary.load(tmp_path / "LargeScaleChain" / "posterior_0k.npz")
    _, exp = MCMC_gpu.run_many(ch, rf, np.stack(beds), seeds, 120, batch=8, posterior=opt)
    assert got.lag_sqdiff.shape == (3, 64, 64) and np.array_equal(got.lag_sqdiff, exp.lag_sqdiff, equal_nan=True)
    assert np.array_equal(got.ess()[0], exp.ess()[0], equal_nan=True) and np.array_equal(got.mcse(), exp.mcse(), equal_nan=True)


def test_c_entry_refusals():
    import torch
    from mcmc_gpu_amd.engine import GsmEngine, _ptr
    H = W = 16
    eng = GsmEngine(H, W, 2)
    try:
        K = 3
        b = torch.ones((2, H, W), dtype=torch.float64, device=eng.dev)
        ring = torch.full((K + 1, 2, H * W), 5.0, dtype=torch.float64, device=eng.dev)
        out = torch.full((K, H, W), 7.0, dtype=torch.float64, device=eng.dev)
        null, st = C.c_void_p(0), eng._stream()
        lib, E_ARG = eng.lib, -1
        off8 = lambda t: C.c_void_p(t.data_ptr() + 8)
        refused = [((null, _ptr(ring), K, 0, 0, _ptr(out)), b"NULL"), ((_ptr(b), null, K, 0, 0, _ptr(out)), b"NULL"),
                   ((_ptr(b), _ptr(ring), K, 0, 0, null), b"NULL"),
                   ((_ptr(b), _ptr(ring), 0, 0, 0, _ptr(out)), b"n_lags"), ((_ptr(b), _ptr(ring), 16, 0, 0, _ptr(out)), b"n_lags"),
                   ((_ptr(b), _ptr(ring), K, -1, 0, _ptr(out)), b"head"), ((_ptr(b), _ptr(ring), K, K, 0, _ptr(out)), b"head"),
                   ((_ptr(b), _ptr(ring), K, 0, -1, _ptr(out)), b"n_valid"), ((_ptr(b), _ptr(ring), K, 0, K + 1, _ptr(out)), b"n_valid"),
                   ((off8(b), _ptr(ring), K, 0, 0, _ptr(out)), b"aligned"), ((_ptr(b), off8(ring), K, 0, 0, _ptr(out)), b"aligned")]
        for args, word in refused:
            assert lib.gsm_posterior_lagged(eng.h, *args, st) == E_ARG, args
            assert word in lib.gsm_last_error(eng.h), (word, lib.gsm_last_error(eng.h))
        torch.cuda.synchronize()
        assert (out == 7.0).all() and (ring == 5.0).all()        # nothing was written
        assert lib.gsm_posterior_lagged(eng.h, _ptr(b), _ptr(ring), K, 0, 0, _ptr(out), st) == 0     # starts a sequence: stores only
        torch.cuda.synchronize()
        assert (out == 7.0).all() and (ring[0] == 1.0).all() and (ring[1:] == 5.0).all()
        assert lib.gsm_posterior_lagged(eng.h, _ptr(b), _ptr(ring), K, 1, 1, _ptr(out), st) == 0     # lag 1 against equal beds: adds 0
        torch.cuda.synchronize()
        assert (out == 7.0).all() and (ring[:2] == 1.0).all() and (ring[2:] == 5.0).all()
        eng.beds = b
        with pytest.raises(ValueError, match="ring"):                # the engine method checks the ring's dtype and size first
            eng.posterior_lagged(ring[:K].to(torch.float32), K, 0, 0, out)
        with pytest.raises(ValueError, match="ring"):
            eng.posterior_lagged(ring, K, 0, 0, out)
    finally:
        eng.close()
