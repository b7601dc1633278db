"""GPU suite of the posterior accumulator (mcmc_gpu_amd/posterior.py, csrc/posterior_kernel.hip): the kernels against NumPy,
their conditioning, the run_many / largeScaleChain_mp paths against the code without `posterior=`, and the error paths.
Definitions and tolerances: tests/posterior_common.py."""
import ctypes as C
import json

import numpy as np
import pytest

import posterior_common as pc
from mcmc_gpu_amd import MCMC_gpu, driver, posterior, synthetic

pytestmark = pytest.mark.gpu


def _feed(x, g, state_dtype, split, rhat, cells=None):
    """x [C, T, H, W] fed snapshot by snapshot through the engine methods (no chain is run: the engine's beds are set)."""
    import torch
    from mcmc_gpu_amd.engine import GsmEngine
    Cn, T, H, W = x.shape
    eng = GsmEngine(H, W, Cn, state_dtype=state_dtype)
    try:
        acc = posterior.PosteriorAccumulator(eng, T, 0, 1, split=split, rhat=rhat, common_ref=g, sample_cells=cells)
        eng.beds = torch.empty((Cn, H, W), dtype=eng.state_dtype, device=eng.dev)
        for t in range(T):
            eng.beds.copy_(torch.as_tensor(x[:, t]))
            acc.add()
        with pytest.raises(RuntimeError):
            acc.add()
        return acc.finalize()
    finally:
        eng.close()


@pytest.mark.parametrize("state_dtype", ["f64", "f32"])
@pytest.mark.parametrize("T", [9, 10])
@pytest.mark.parametrize("shape", [(37, 41), (64, 64)])
def test_kernels_against_numpy(shape, T, state_dtype):
    H, W = shape
    Cn = 5
    rng = np.random.default_rng(H * 100 + T)
    x = -300.0 + 100.0 * rng.normal(size=(Cn, T, H, W))
    x[:, :, 10:14, 10:20] = x[:, :1, 10:14, 10:20]           # constant within every chain
    half = T - T // 2                                        # constant within each half of every chain, a step between the halves
    x[:, :half, 20:22, 5:9] = x[:, :1, 20:22, 5:9]
    x[:, half:, 20:22, 5:9] = x[:, half:half + 1, 20:22, 5:9]
    x[2, T - 2, 5, 7] = np.nan
    g = -300.0 + 10.0 * rng.normal(size=(H, W))
    if state_dtype == "f32":
        x = x.astype(np.float32).astype(np.float64)          # the reference sees the same f32 values, cast to f64
    cells = np.array([0, 5 * W + 7, 12 * W + 15, H * W - 1])
    for split in (True, False):
        ref = pc.posterior_reference(x, split)
        for rhat in (True, False):
            s = _feed(x, g, state_dtype, split, rhat, cells)
            pc.check_maps(s, ref, rhat=rhat, label=f"{shape} T={T} {state_dtype} split={split} rhat={rhat}")
            assert np.isnan(s.mean[5, 7]) and np.isnan(s.sd[5, 7]) and np.isnan(s.mean).sum() == 1
            assert np.array_equal(s.sample_values, x.reshape(Cn, T, H * W)[:, :, cells].transpose(0, 2, 1), equal_nan=True)
            assert (s.n_chains, s.n_sequences, s.n_per_sequence) == (Cn, ref["M"], ref["N"])
            if rhat:
                const = np.zeros((H, W), dtype=bool)
                const[10:14, 10:20] = True
                const[20:22, 5:9] = split                    # W == 0 there only when the halves are the sequences
                assert (s.within_var[const] == 0).all() and np.isnan(s.rhat[const]).all()
                assert np.isfinite(s.rhat[~const]).sum() == H * W - const.sum() - 1
            else:
                assert s.rhat is None


@pytest.mark.parametrize("state_dtype", ["f64", "f32"])
@pytest.mark.parametrize("rhat, split, hist, ess, points", [
    (True, True, None, None, False),
    (True, False, dict(bins=64, half_width=50.0, levels=(-300.0, -250.0)), dict(max_lag=3), True),
    (False, False, dict(bins=2, half_width=50.0), None, True)])
def test_memory_budget_is_what_is_allocated(rhat, split, hist, ess, points, state_dtype):
    """The bytes the accumulator holds against the free device memory are those of the tensors it then owns, exactly."""
    import torch
    from mcmc_gpu_amd.engine import GsmEngine
    H, W, Cn, T = 37, 41, 5, 10
    eng = GsmEngine(H, W, Cn, state_dtype=state_dtype)
    try:
        acc = posterior.PosteriorAccumulator(eng, T, 0, 1, split=split, rhat=rhat, hist=hist, ess=ess,
                                             sample_cells=np.array([0, 5 * W + 7, H * W - 1]) if points else None)
        held = {k: v for k, v in vars(acc).items() if isinstance(v, torch.Tensor)}
        print(f"budget {acc.device_bytes} B; held {({k: v.nbytes for k, v in held.items()})}")
        assert acc.device_bytes == sum(v.nbytes for v in held.values())
        assert len({v.data_ptr() for v in held.values()}) == len(held)      # no tensor counted twice under two names
    finally:
        eng.close()


@pytest.mark.parametrize("T", [9, 10])
def test_conditioning_large_offset(T):
    """Beds 1e6 + N(0, 1): an unshifted sum of squares loses about u * 1e12 = 1e-4 of a variance of 1.  Expected maps from
    posterior_reference(x - 1e6) (exact subtraction) with 1e6 added to the mean: NumPy's own mean and between-sequence variance
    of values near 1e6 are off by up to 1e-9."""
    Cn, H, W = 5, 64, 64
    z = np.random.default_rng(T).normal(size=(Cn, T, H, W))
    x = 1e6 + z
    g = np.full((H, W), 1e6)
    for split in (True, False):
        ref = pc.posterior_reference(x - 1e6, split)
        ref["mean"] = ref["mean"] + 1e6
        for rhat in (True, False):
            s = _feed(x, g, "f64", split, rhat)
            pc.check_maps(s, ref, mean_atol=1e-8, rhat=rhat, label=f"conditioning T={T} split={split} rhat={rhat}")


def _template_with_points():
    prob, ch, rf = synthetic.template(64)
    ij = np.array([[30, 30], [2, 3], [16, 40]])              # inside the update region, outside it, on a data row
    assert prob["region_mask"][30, 30] == 1 and prob["region_mask"][2, 3] == 0 and prob["data_mask"][16, 40]
    ch.set_sample_points_locations(np.array([[prob["xx"][i, j], prob["yy"][i, j]] for i, j in ij]))
    assert np.array_equal(ch._sample_indices(), ij)
    return prob, ch, rf, ij


def _stretched_snapshots(ch, rf, beds, seeds, its):
    """The beds at the snapshot iterations from run_many WITHOUT posterior, called stretch by stretch with step0."""
    cur, done, snaps = np.asarray(beds, dtype=np.float64), 0, []
    for k in [int(v) for v in its]:
        if k > done:
            r = MCMC_gpu.run_many(ch, rf, cur, seeds, k - done + 1, batch=8, step0=done)
            cur, done = np.stack([t[0] for t in r]), k
        snaps.append(cur)
    return np.stack(snaps, axis=1)                           # [C, T, H, W]


@pytest.mark.parametrize("burn_in,thin,T", [(11, 5, 10), (0, 7, 9)])
def test_run_many_posterior_end_to_end(burn_in, thin, T):
    prob, ch, rf, ij = _template_with_points()
    beds, seeds, n_iter = synthetic.initial_beds(prob, 4), [5, 6, 7, 8], 61
    its = posterior.snapshot_iterations(n_iter, burn_in, thin)
    assert its.size == T
    x = _stretched_snapshots(ch, rf, beds, seeds, its)
    plain = MCMC_gpu.run_many(ch, rf, beds, seeds, n_iter, batch=8)
    for split in (True, False):
        ref = pc.posterior_reference(x, split)
        for rhat in (True, False):
            res, s = MCMC_gpu.run_many(ch, rf, beds, seeds, n_iter, batch=8, posterior=dict(burn_in=burn_in, thin=thin, split=split, rhat=rhat))
            assert len(res) == len(plain)
            for ra, rb in zip(res, plain):
                assert len(ra) == len(rb) and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(ra, rb))
            pc.check_maps(s, ref, rhat=rhat, label=f"end to end burn_in={burn_in} thin={thin} split={split} rhat={rhat}")
            assert np.array_equal(s.snapshot_iterations, its) and (s.burn_in, s.thin, s.split) == (burn_in, thin, split)
            assert np.array_equal(s.sample_values, x[:, :, ij[:, 0], ij[:, 1]].transpose(0, 2, 1))
            assert np.array_equal(s.sample_loc, ch.sample_loc)
            if rhat:
                # W == 0, hence rhat NaN, exactly where no SEQUENCE's snapshots differ (with split=False: no chain's used
                # snapshots).  A cell that is constant within both halves of every chain but stepped between them has W == 0 too:
                # rhat = sqrt(B / 0) has no finite value there, so the halves, not the chains, define the NaN set.
                seq = pc.sequences(x, split)
                still = (seq == seq[:, :1]).all(axis=(0, 1))
                assert still[2, 3] and not still[30, 30]
                assert np.isnan(s.rhat[still]).all() and np.isfinite(s.rhat[~still]).all()
                assert (s.within_var[still] == 0).all()


def test_rhat_measures_disagreement():
    prob, ch, rf = synthetic.template(64)
    seeds = list(range(40, 48))
    opt = dict(burn_in=1, thin=10)
    med = []
    for shift in (0.0, 200.0):
        beds = synthetic.initial_beds(prob, 8)
        beds[4:] += shift * (prob["region_mask"] == 1)           # thickness stays positive: it is about 1000 m
        _, s = MCMC_gpu.run_many(ch, rf, beds, seeds, 201, batch=8, posterior=opt)
        med.append(float(np.median(s.rhat[np.isfinite(s.rhat)])))
    print(f"median rhat: chains from one start {med[0]:.4f}, chains 4-7 started 200 m higher {med[1]:.4f}")
    assert med[1] > med[0], f"median rhat {med[1]} (chains 4-7 started 200 m higher) is not above {med[0]} (all from one start)"


def _folder_arrays(folder, k):
    out = {"bed": np.load(folder / f"bed_{k}.npy"), "iter": np.loadtxt(folder / "current_iter.txt"),
           "philox": json.load(open(folder / "RNGState_philox.txt"))}
    with np.load(folder / f"results_{k}.npz") as r:
        out.update({key: r[key] for key in r.files})
    return out


def test_driver_writes_the_summary_and_leaves_the_checkpoints_alone(tmp_path):
    prob, ch, rf, ij = _template_with_points()
    ch.set_rng_mode("philox")
    seeds = [111111, 222222, 333333]
    beds = list(synthetic.initial_beds(prob, 3))
    opt = dict(burn_in=100, thin=100)
    a = driver.largeScaleChain_mp(3, 7, ch, rf, beds, seeds, [1000] * 3, output_path=str(tmp_path / "with"), posterior=opt, n_gpus=1)
    b = driver.largeScaleChain_mp(3, 7, ch, rf, beds, seeds, [1000] * 3, output_path=str(tmp_path / "without"), n_gpus=1)
    assert len(a) == 3 and len(a[0]) == 7
    for ra, rb in zip(a, b):
        assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(ra, rb))
    for s in seeds:
        fa = _folder_arrays(tmp_path / "with" / "LargeScaleChain" / str(s)[:6], "1k")
        fb = _folder_arrays(tmp_path / "without" / "LargeScaleChain" / str(s)[:6], "1k")
        assert fa.keys() == fb.keys() and fa["philox"] == fb["philox"] == {"key": s, "step": 999}
        for key in fa:
            if key != "philox":
                assert np.array_equal(fa[key], fb[key], equal_nan=True), key
    assert not (tmp_path / "without" / "LargeScaleChain" / "posterior_1k.npz").exists()
    got = posterior.PosteriorSummary.load(tmp_path / "with" / "LargeScaleChain" / "posterior_1k.npz")
    _, exp = MCMC_gpu.run_many(ch, rf, np.stack(beds), seeds, 1000, batch=8, posterior=opt)
    for name in ("mean", "sd", "rhat", "within_var", "between_var_over_n", "sample_values", "snapshot_iterations", "sample_loc"):
        assert np.array_equal(getattr(got, name), getattr(exp, name), equal_nan=True), name
    assert (got.n_chains, got.n_sequences, got.n_per_sequence) == (3, 6, 4) and got.sample_values.shape == (3, 3, 9)


def test_driver_two_ranks_merge(tmp_path, monkeypatch):
    """n_gpus=2 without a launcher (two self-started ranks on the box's one GPU, gloo): ragged shards of 3 and 2 chains, partials
    summed over the ranks, traces gathered."""
    monkeypatch.setenv("GSM_DIST_BACKEND", "gloo")
    prob, ch, rf, ij = _template_with_points()
    seeds = [31, 32, 33, 34, 35]
    beds = list(synthetic.initial_beds(prob, 5))
    opt = dict(burn_in=20, thin=10)
    out = {}
    for n in (1, 2):
        res = driver.largeScaleChain_mp(5, 2, ch, rf, beds, seeds, [120] * 5, output_path=str(tmp_path / f"r{n}"), mode="philox", n_gpus=n,
                                        posterior=opt)
        out[n] = (res, posterior.PosteriorSummary.load(tmp_path / f"r{n}" / "LargeScaleChain" / "posterior_0k.npz"))
    for ra, rb in zip(out[1][0], out[2][0]):
        assert all(np.array_equal(np.asarray(x, dtype=float), np.asarray(y, dtype=float), equal_nan=True) for x, y in zip(ra, rb))
    one, two = out[1][1], out[2][1]
    assert (two.n_chains, two.n_sequences, two.n_per_sequence) == (5, 10, 5) == (one.n_chains, one.n_sequences, one.n_per_sequence)
    assert np.array_equal(two.sample_values, one.sample_values) and two.sample_values.shape == (5, 3, 10)
    ref = dict(mean=one.mean, sd=one.sd, within_var=one.within_var, between_var_over_n=one.between_var_over_n, rhat=one.rhat)
    pc.check_maps(two, ref, label="two ranks against one")


def test_error_paths(tmp_path, monkeypatch):
    import torch
    from mcmc_gpu_amd.engine import GsmEngine, _ptr
    prob, ch, rf = synthetic.template(64)
    beds, seeds = list(synthetic.initial_beds(prob, 2)), [1, 2]
    with pytest.raises(ValueError, match="philox"):
        driver.largeScaleChain_mp(2, 1, ch, rf, beds, seeds, [100] * 2, output_path=str(tmp_path), mode="replay", n_gpus=1,
                                  posterior=dict(burn_in=0, thin=10))
    with pytest.raises(ValueError, match="same n_iter"):
        driver.largeScaleChain_mp(2, 1, ch, rf, beds, seeds, [100, 90], output_path=str(tmp_path), mode="philox", n_gpus=1,
                                  posterior=dict(burn_in=0, thin=10))
    with pytest.raises(ValueError, match="snapshots"):
        driver.largeScaleChain_mp(2, 1, ch, rf, beds, seeds, [100] * 2, output_path=str(tmp_path), mode="philox", n_gpus=1,
                                  posterior=dict(burn_in=80, thin=10))
    assert not (tmp_path / "LargeScaleChain").exists()               # refused before anything ran
    with pytest.raises(ValueError, match="snapshots"):
        MCMC_gpu.run_many(ch, rf, np.stack(beds), seeds, 100, posterior=dict(burn_in=0, thin=40))           # T = 3 < 4 with split
    MCMC_gpu.run_many(ch, rf, np.stack(beds), seeds, 100, posterior=dict(burn_in=0, thin=40, split=False))  # T = 3 is enough unsplit
    with monkeypatch.context() as m:
        m.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (1 << 17, 1 << 40))
        with pytest.raises(MemoryError, match="rhat=False"):
            MCMC_gpu.run_many(ch, rf, np.stack(beds), seeds, 100, posterior=dict(burn_in=0, thin=10))
        MCMC_gpu.run_many(ch, rf, np.stack(beds), seeds, 100, posterior=dict(burn_in=0, thin=10, rhat=False))   # two [H, W] arrays fit
    eng = GsmEngine(16, 16, 2)
    try:
        z = lambda *s: torch.zeros(s, dtype=torch.float64, device=eng.dev)
        b, ref, s1, s2, g, out = z(2, 16, 16), z(2, 16, 16), z(2, 2 * 256), z(2, 2 * 256), z(16, 16), z(3, 16, 16)
        null, st = C.c_void_p(0), eng._stream()
        lib, E_ARG = eng.lib, -1
        assert lib.gsm_posterior_accumulate(eng.h, _ptr(b), null, _ptr(s1), _ptr(s2), 1, null, 0, null, st) == E_ARG
        assert b"NULL" in lib.gsm_last_error(eng.h)
        assert lib.gsm_posterior_accumulate(eng.h, _ptr(b), _ptr(ref), C.c_void_p(s1.data_ptr() + 8), _ptr(s2), 1, null, 0, null, st) == E_ARG
        assert b"aligned" in lib.gsm_last_error(eng.h)
        assert lib.gsm_posterior_accumulate(eng.h, _ptr(b), _ptr(ref), _ptr(s1), _ptr(s2), 1, null, 0, _ptr(out), st) == E_ARG
        assert lib.gsm_posterior_accumulate_pooled(eng.h, _ptr(b), null, _ptr(s1), _ptr(s2), null, 0, null, st) == E_ARG
        assert lib.gsm_posterior_sample(eng.h, _ptr(b), null, 0, null, st) == E_ARG
        assert lib.gsm_posterior_close(eng.h, _ptr(ref), null, _ptr(s1), _ptr(s2), 5, st) == E_ARG
        assert lib.gsm_posterior_close(eng.h, _ptr(ref), _ptr(g), _ptr(s1), _ptr(s2), 1, st) == E_ARG
        assert b"n_per_seq" in lib.gsm_last_error(eng.h)
        assert lib.gsm_posterior_partials(eng.h, _ptr(ref), _ptr(g), _ptr(s1), _ptr(s2), 2, 512, 1, 5, null, st) == E_ARG
        assert lib.gsm_posterior_partials(eng.h, _ptr(ref), _ptr(g), _ptr(s1), _ptr(s2), 2, 512, 1, 1, _ptr(out), st) == E_ARG
        assert b"n_per_seq" in lib.gsm_last_error(eng.h)
        assert lib.gsm_posterior_partials(eng.h, _ptr(ref), _ptr(g), _ptr(s1), _ptr(s2), 3, 512, 1, 5, _ptr(out), st) == E_ARG
        assert b"n_seq_per_chain" in lib.gsm_last_error(eng.h)
        assert lib.gsm_posterior_partials(eng.h, _ptr(ref), _ptr(g), _ptr(s1), _ptr(s2), 2, 512, 3, 5, _ptr(out), st) == E_ARG
        assert b"n_closed" in lib.gsm_last_error(eng.h)
        assert lib.gsm_posterior_partials(eng.h, _ptr(ref), _ptr(g), _ptr(s1), _ptr(s2), 2, 100, 1, 5, _ptr(out), st) == E_ARG
        assert lib.gsm_posterior_close(eng.h, _ptr(ref), _ptr(g), _ptr(s1), _ptr(s2), 5, st) == 0
        assert lib.gsm_posterior_partials(eng.h, _ptr(ref), _ptr(g), _ptr(s1), _ptr(s2), 2, 512, 1, 5, _ptr(out), st) == 0
        torch.cuda.synchronize()
        assert (out == 0).all()
    finally:
        eng.close()
