"""-m gpu: posterior summaries of the large-scale chain in 'pcg64' mode (MCMC_gpu.run_many_pcg64(posterior=) and
driver.largeScaleChain_mp(mode='pcg64', posterior=)).

Reference.  The snapshots are the beds of run_many_pcg64 WITHOUT posterior, run stretch by stretch from the generator states each
stretch returns (iteration k is the bed after k proposals, iteration 0 the initial bed), as test_gpu_posterior's
_stretched_snapshots does for Philox mode; the maps are asserted against posterior_common.posterior_reference of them at that
module's tolerances (T <= 10 snapshots of beds of order 1e3 m: inside the bounds derived there)."""
import functools
import json

import numpy as np
import pytest

import posterior_common as pc
from mcmc_gpu_amd import MCMC_gpu, driver, posterior, synthetic

pytestmark = pytest.mark.gpu

N, N_ITER = 4, 61
IJ = np.array([[30, 30], [2, 3], [16, 40]])                  # inside the update region, outside it, on a data row


def _template_with_points():
    prob, ch, rf = synthetic.template(64)
    ch.set_sample_points_locations(np.array([[prob["xx"][i, j], prob["yy"][i, j]] for i, j in IJ]))
    assert np.array_equal(ch._sample_indices(), IJ)
    return prob, ch, rf


def _states(n=N):
    return [np.random.default_rng(seed=700 + i).bit_generator.state for i in range(n)]


@functools.lru_cache(maxsize=None)
def _stretched_snapshots(burn_in, thin):
    """x [N, T, H, W]: the beds at the snapshot iterations from run_many_pcg64 without posterior, stretch by stretch"""
    prob, ch, rf = _template_with_points()
    cur, rf_st, ch_st, done, snaps = synthetic.initial_beds(prob, N), _states(), _states(), 0, []
    for k in [int(v) for v in posterior.snapshot_iterations(N_ITER, burn_in, thin)]:
        if k > done:
            r, rf_st, ch_st = MCMC_gpu.run_many_pcg64(ch, rf, cur, rf_st, ch_st, k - done + 1)
            cur, done = np.stack([t[0] for t in r]), k
        snaps.append(np.array(cur))
    x = np.stack(snaps, axis=1)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _plain(fused):
    prob, ch, rf = _template_with_points()
    return MCMC_gpu.run_many_pcg64(ch, rf, synthetic.initial_beds(prob, N), _states(), _states(), N_ITER, fused=fused)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("burn_in,thin,T,batch", [(11, 5, 10, None), (0, 7, 9, None), (11, 5, 10, 32), (0, 7, 9, 4)])
def test_run_many_pcg64_posterior(burn_in, thin, T, batch, fused):
    prob, ch, rf = _template_with_points()
    its = posterior.snapshot_iterations(N_ITER, burn_in, thin)
    assert its.size == T
    x = _stretched_snapshots(burn_in, thin)
    plain, rf_p, ch_p = _plain(fused)
    assert 0.2 < np.mean([r[4][1:].mean() for r in plain]) < 0.95
    for split in (True, False):
        ref = pc.posterior_reference(x, split)
        for rhat in (True, False):
            timing = {}
            res, rf_s, ch_s, s = MCMC_gpu.run_many_pcg64(ch, rf, synthetic.initial_beds(prob, N), _states(), _states(), N_ITER, batch=batch,
                                                         fused=fused, timing=timing,
                                                         posterior=dict(burn_in=burn_in, thin=thin, split=split, rhat=rhat))
            assert timing["fused"] == fused
            assert rf_s == rf_p and ch_s == ch_p and len(res) == N
            for ra, rb in zip(res, plain):                   # the chains are those of the run without posterior, bit for bit
                assert len(ra) == len(rb) == 7 and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(ra, rb))
            pc.check_maps(s, ref, rhat=rhat, label=f"pcg64 fused={fused} batch={batch} burn_in={burn_in} thin={thin} split={split} rhat={rhat}")
            assert np.array_equal(s.snapshot_iterations, its) and (s.burn_in, s.thin, s.split) == (burn_in, thin, split)
            assert np.array_equal(s.sample_values, x[:, :, IJ[:, 0], IJ[:, 1]].transpose(0, 2, 1))
            assert np.array_equal(s.sample_loc, ch.sample_loc)
    # the last stretch ends where the whole run ends when the last iteration is a snapshot
    if its[-1] == N_ITER - 1:
        assert np.array_equal(x[:, -1], np.stack([r[0] for r in plain]))


def test_accumulator_is_readable_after_the_call():
    prob, ch, rf = _template_with_points()
    opt = dict(burn_in=11, thin=5, hist=dict(bins=32, half_width=100.0), local=True, residual=True)
    *_, accum = MCMC_gpu.run_many_pcg64(ch, rf, synthetic.initial_beds(prob, N), _states(), _states(), N_ITER, posterior=opt,
                                        return_accumulator=True)
    assert accum.eng.h is None                               # the run's handle is closed
    sums = accum.local_sums()
    assert set(sums) == {"partials_sum", "M", "hist_counts", "residual_sums", "local_cross"} and int(sums["M"]) == 2 * N
    *_, s = MCMC_gpu.run_many_pcg64(ch, rf, synthetic.initial_beds(prob, N), _states(), _states(), N_ITER, posterior=opt)
    got = accum.finalize()
    for name in ("mean", "sd", "rhat", "hist_counts", "residual_sums", "local_cross", "sample_values"):
        assert np.array_equal(getattr(got, name), getattr(s, name), equal_nan=True), name
    assert got.hist_counts.sum() == 2 * N * 5 * 64 * 64


def _folder_arrays(folder, k):
    out = {"bed": np.load(folder / f"bed_{k}.npy"), "iter": np.loadtxt(folder / "current_iter.txt")}
    for name in ("RNGState_RandField.txt", "RNGState_chain.txt", "RNGState_philox.txt"):
        out[name] = json.load(open(folder / name))
    with np.load(folder / f"results_{k}.npz") as r:
        out.update({key: r[key] for key in r.files})
    return out


def test_driver_pcg64_mode(tmp_path, monkeypatch):
    """largeScaleChain_mp(mode='pcg64', posterior=): one rank and two self-started ranks (gloo, 2 + 1 chains) against the run
    without posterior and against the library call."""
    monkeypatch.setenv("GSM_DIST_BACKEND", "gloo")
    prob, ch, rf = _template_with_points()
    seeds = [111111, 222222, 333333]
    beds = list(synthetic.initial_beds(prob, 3))
    opt = dict(burn_in=11, thin=5)
    res = {}
    for tag, n_gpus, post in (("one", 1, opt), ("two", 2, opt), ("none", 1, None)):
        res[tag] = driver.largeScaleChain_mp(3, 1, ch, rf, beds, seeds, [N_ITER] * 3, output_path=str(tmp_path / tag), mode="pcg64",
                                             n_gpus=n_gpus, posterior=post)
    assert not (tmp_path / "none" / "LargeScaleChain" / "posterior_0k.npz").exists()
    for tag in ("one", "two"):
        for ra, rb in zip(res[tag], res["none"]):
            assert all(np.array_equal(np.asarray(x, dtype=float), np.asarray(y, dtype=float), equal_nan=True) for x, y in zip(ra, rb))
        for sd in seeds:
            fa = _folder_arrays(tmp_path / tag / "LargeScaleChain" / str(sd)[:6], "0k")
            fb = _folder_arrays(tmp_path / "none" / "LargeScaleChain" / str(sd)[:6], "0k")
            assert fa.keys() == fb.keys()
            for key in fa:
                assert fa[key] == fb[key] if isinstance(fa[key], dict) else np.array_equal(fa[key], fb[key], equal_nan=True), key
    one = posterior.PosteriorSummary.load(tmp_path / "one" / "LargeScaleChain" / "posterior_0k.npz")
    two = posterior.PosteriorSummary.load(tmp_path / "two" / "LargeScaleChain" / "posterior_0k.npz")
    st = [np.random.default_rng(seed=s).bit_generator.state for s in seeds]
    *_, exp = MCMC_gpu.run_many_pcg64(ch, rf, np.stack(beds), st, st, N_ITER, posterior=opt)
    for name in ("mean", "sd", "rhat", "within_var", "between_var_over_n", "sample_values", "snapshot_iterations", "sample_loc"):
        assert np.array_equal(getattr(one, name), getattr(exp, name), equal_nan=True), name
    assert (two.n_chains, two.n_sequences, two.n_per_sequence) == (3, 6, 5) == (one.n_chains, one.n_sequences, one.n_per_sequence)
    assert np.array_equal(two.sample_values, one.sample_values) and two.sample_values.shape == (3, 3, 10)
    pc.check_maps(two, dict(mean=one.mean, sd=one.sd, within_var=one.within_var, between_var_over_n=one.between_var_over_n, rhat=one.rhat),
                  label="pcg64 driver: two ranks against one")


def test_refusals(tmp_path):
    prob, ch, rf = _template_with_points()
    beds, seeds = list(synthetic.initial_beds(prob, 2)), [1, 2]
    with pytest.raises(ValueError, match="philox"):          # replay mode stays refused, and the text still names philox
        driver.largeScaleChain_mp(2, 1, ch, rf, beds, seeds, [100] * 2, output_path=str(tmp_path), mode="replay", n_gpus=1,
                                  posterior=dict(burn_in=0, thin=10))
    with pytest.raises(ValueError, match="same n_iter"):
        driver.largeScaleChain_mp(2, 1, ch, rf, beds, seeds, [100, 90], output_path=str(tmp_path), mode="pcg64", n_gpus=1,
                                  posterior=dict(burn_in=0, thin=10))
    with pytest.raises(ValueError, match="snapshots"):
        driver.largeScaleChain_mp(2, 1, ch, rf, beds, seeds, [100] * 2, output_path=str(tmp_path), mode="pcg64", n_gpus=1,
                                  posterior=dict(burn_in=80, thin=10))
    assert not (tmp_path / "LargeScaleChain").exists()       # refused before anything ran
    with pytest.raises(ValueError, match="snapshots"):
        MCMC_gpu.run_many_pcg64(ch, rf, np.stack(beds), _states(2), _states(2), 100, posterior=dict(burn_in=0, thin=40))
