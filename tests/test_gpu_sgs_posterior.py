"""-m gpu: posterior summaries of the small-scale chain (sgs.run_many_sgs(posterior=), driver.smallScaleChain_mp(posterior=)).

Reference.  x = bed_cache[:, its] of the only_save_last_bed=False run on the same seeds: the beds after the snapshot iterations'
decisions, in bed units, as the host keeps them.  The run with `posterior` folds cur + trend (one fp64 add on the device, NumPy's
bits) into the accumulators, so the maps are asserted against posterior_common.posterior_reference(x) at the tolerances derived in
posterior_common (beds of order 1e3 m, T <= 61 snapshots: inside their T <= 20 bound for thin >= 5; for thin = 1 the recursive-sum
bound T u D = 61 * 1.1e-16 * 1e3 = 7e-12 m stays two orders under MEAN_ATOL), and every additive quantity bit for bit against an
accumulator on a fresh engine fed x snapshot by snapshot.

The reference's within-sequence variance.  With the normal-score transformer a cell of an accepted block that holds a datum comes
back from the inverse transform a few ulp (1.1e-13 m at 1e3 m) from where it was: such a cell is not constant within a sequence, its
W is 1e-28 .. 1e-26 m^2 (measured), and rhat = sqrt(((N - 1) / N W + B) / W) there is of order 1e13.  posterior_reference takes
np.var of the values themselves: the mean of N values near 1e3 m is rounded to 1.1e-13 m, the size of the deviations, so its W for such a cell has
no correct digit (it guards only sequences that are exactly constant), and RHAT_RTOL cannot be asked of a ratio with that W.  Its
own bound says so: a variance known to 1e-10 m^2 gives rhat to 1e-7 only where W >= 1e-3 m^2.  _reference therefore keeps
posterior_reference's mean, sd and B_over_N and takes W from the same definition with every sequence shifted by its first value
first (an exact subtraction, the values of a sequence being within a factor 2 of each other): np.var of the shifted values is good
to a few u relative whatever their size.  It asserts that this W agrees with posterior_reference's within VAR_RTOL / VAR_ATOL, the
reference's own accuracy, and that it is 0 on exactly the same cells; rhat follows from it.  Every cell is then asserted at
MEAN_ATOL, VAR_RTOL / VAR_ATOL and RHAT_RTOL as everywhere else."""
import functools

import numpy as np
import pytest

import posterior_common as pc
import posterior_hist_common as hc
from mcmc_gpu_amd import driver, posterior, sgs, synthetic

pytestmark = pytest.mark.gpu

H, N, N_ITER = 32, 4, 61
SOURCES = ("replay", "pcg64", "philox")
POINTS = np.array([[5, 7], [20, 11], [16, 16]])


class _Wrapped:
    """scikit-learn's transformer behind another class: run_many_sgs then calls it on the host and keeps the chains' state there"""

    def __init__(self, inner):
        self.inner = inner

    def transform(self, x):
        return self.inner.transform(x)

    def inverse_transform(self, x):
        return self.inner.inverse_transform(x)


def _template(cfg, points=False):
    """cfg 'qt': the template as it is (device transformer, trend); 'plain': no transformer, no trend; 'trend': no transformer, a
    trend; 'host': the transformer behind another class, trend."""
    prob, ch = synthetic.sgs_template(H, transform=cfg in ("qt", "host"), light=True)
    if cfg == "trend":
        ch.set_trend(prob["surf"] - 1000.0, detrend_map=True)
    if cfg == "host":
        ch.set_normal_transformation(_Wrapped(ch.nst_trans), do_transform=True)
    if points:
        ch.set_sample_points_locations(np.array([[prob["xx"][i, j], prob["yy"][i, j]] for i, j in POINTS]))
    return prob, ch


def _run(cfg, source, points=False, keep_all=False, **kw):
    """(result tuples, the generators' final states, the summary or accumulator or None) of the N chains on fixed seeds"""
    prob, ch = _template(cfg, points)
    beds = [prob["bed"] + np.random.default_rng(40 + i).normal(0, 3, prob["bed"].shape) for i in range(N)]
    rngs = [np.random.default_rng(900 + i) for i in range(N)]
    out = sgs.run_many_sgs(ch, beds, rngs, N_ITER, only_save_last_bed=not keep_all, pcg64=source == "pcg64",
                           philox_seeds=[300 + i for i in range(N)] if source == "philox" else None, **kw)
    assert len(out) == (2 if kw.get("posterior") is None else 3) and out[1] is rngs
    return out[0], [r.bit_generator.state for r in rngs], out[2] if len(out) == 3 else None


@functools.lru_cache(maxsize=None)
def _bed_cache(cfg, source, points=False):
    """x [N, N_ITER, H, W]: every iteration's beds as the host records them; computed once per case, no test writes into it"""
    x = np.stack([r[0] for r in _run(cfg, source, points, keep_all=True)[0]])
    assert x.shape == (N, N_ITER, H, H)
    x.setflags(write=False)
    return x


def _reference(x, split):
    """posterior_reference(x, split) with W, and the rhat that follows from it, computed from sequences shifted by their first
    value (module docstring)"""
    ref = pc.posterior_reference(x, split)
    seq = pc.sequences(x, split)
    d = seq - seq[:, :1]
    assert np.array_equal(d + seq[:, :1], seq)                # the shift is exact
    Nn = seq.shape[1]
    W = np.var(d, axis=1, ddof=1).mean(axis=0)
    assert np.array_equal(W == 0, ref["within_var"] == 0)
    assert (np.abs(W - ref["within_var"]) <= pc.VAR_RTOL * W + pc.VAR_ATOL).all()
    with np.errstate(invalid="ignore", divide="ignore"):
        rhat = np.where(W == 0, np.nan, np.sqrt(((Nn - 1) / Nn * W + ref["between_var_over_n"]) / W))
        off = np.abs(rhat - ref["rhat"]) > pc.RHAT_RTOL * rhat
    print(f"reference: {int(off.sum())} cells where posterior_reference's rhat is off by more than RHAT_RTOL from the shifted form; "
          f"smallest W > 0: {W[W > 0].min():.3e} m^2, largest W among those cells: {W[off].max() if off.any() else 0.0:.3e} m^2")
    ref.update(within_var=W, rhat=rhat)
    return ref


def _same_chains(a, b, source):
    """beds, accept masks, counts, blocks and generator states bit for bit; losses bit for bit with device draws, to 1e-12 with
    host draws (the bar of test_batched_iterations_equal_one_by_one)"""
    (ra, sa), (rb, sb) = a[:2], b[:2]
    assert sa == sb and len(ra) == len(rb) == N
    for x, y in zip(ra, rb):
        assert len(x) == len(y)
        for k in (0, 4, 5, 6) + ((7,) if len(x) == 8 else ()):
            assert np.array_equal(x[k], y[k], equal_nan=True), k
        if source == "replay":
            np.testing.assert_allclose(x[3], y[3], rtol=1e-12)
        else:
            assert np.array_equal(x[3], y[3])


@pytest.mark.parametrize("burn_in,thin", [(11, 5), (0, 7), (0, 1)])
def test_schedules(burn_in, thin):
    source = "pcg64"
    its = posterior.snapshot_iterations(N_ITER, burn_in, thin)
    x = _bed_cache("qt", source)[:, its]
    plain = _run("qt", source)
    assert 0.05 < np.mean([r[4].mean() for r in plain[0]]) < 0.95
    for split in (True, False):
        ref = _reference(x, split)
        for rhat in (True, False):
            out = _run("qt", source, posterior=dict(burn_in=burn_in, thin=thin, split=split, rhat=rhat))
            s = out[2]
            pc.check_maps(s, ref, rhat=rhat, label=f"sgs burn_in={burn_in} thin={thin} split={split} rhat={rhat}")
            assert np.array_equal(s.snapshot_iterations, its) and (s.burn_in, s.thin, s.split) == (burn_in, thin, split)
            assert (s.n_chains, s.n_sequences, s.n_per_sequence) == (N, ref["M"], ref["N"]) and s.sample_values is None
            _same_chains(out, plain, source)


_SWITCHES = (("GSM_SGS_DRAW_AHEAD", "0"), ("GSM_SGS_BATCH", "1"), ("GSM_SGS_BATCH", "4"), ("GSM_SGS_BATCH", "32"))
_CASES = [(c, None) for c in ("qt", "plain", "trend", "host")] + [(c, e) for c in ("qt", "trend") for e in _SWITCHES]


@pytest.mark.parametrize("cfg,env", _CASES, ids=[c if e is None else f"{c}-{e[0][8:]}={e[1]}" for c, e in _CASES])
@pytest.mark.parametrize("source", SOURCES)
def test_draw_sources_and_iteration_ends(monkeypatch, source, cfg, env):
    burn_in, thin, split = 11, 5, True
    its = posterior.snapshot_iterations(N_ITER, burn_in, thin)
    x = _bed_cache(cfg, source)[:, its]                      # one iteration per batch whatever the switches say
    if env is not None:
        monkeypatch.setenv(*env)
    plain = _run(cfg, source)
    out = _run(cfg, source, posterior=dict(burn_in=burn_in, thin=thin))
    pc.check_maps(out[2], _reference(x, split), label=f"sgs {source} {cfg} {env}")
    _same_chains(out, plain, source)


def _fed(ch, x, its, opt, cells):
    """local_sums(), traces and projections of an accumulator on a fresh engine with the run's static fields, fed x through set_state"""
    from mcmc_gpu_amd.engine import GsmEngine
    eng = GsmEngine(H, H, N)
    try:
        eng.set_static(ch.surf, ch.velx, ch.vely, ch.dhdt, ch.smb, None, ch.grounded_ice_mask, ch.mc_region_mask, ch.resolution, ch.sigma_mc)
        acc = posterior.PosteriorAccumulator(eng, N_ITER, opt["burn_in"], opt["thin"], common_ref=posterior.default_common_ref(ch.initial_bed),
                                             sample_cells=cells, hist=opt["hist"], ess=opt["ess"], cov=opt["cov"], residual=opt["residual"],
                                             local=opt["local"])
        for t in range(its.size):
            eng.set_state(np.ascontiguousarray(x[:, t]))
            acc.add()
        return {k: v.cpu().numpy() for k, v in acc.local_sums().items()}, acc.sample_values(), acc.projections()
    finally:
        eng.close()


@pytest.mark.parametrize("source", SOURCES)
def test_every_option_in_one_run(source):
    cells = POINTS[:, 0] * H + POINTS[:, 1]
    prob, ch = _template("qt", points=True)
    g = posterior.default_common_ref(ch.initial_bed)
    opt = dict(burn_in=11, thin=5, hist=dict(bins=64, half_width=40.0, levels=(float(g[16, 16]), float(g[5, 7]) - 5.0)), ess=dict(max_lag=3),
               cov=dict(probes=posterior.point_probes(H, H, cells[:2]), names=("a", "b")), residual=dict(levels=(0.0, 50.0)),
               local=dict(reach=2))
    its = posterior.snapshot_iterations(N_ITER, 11, 5)
    x = _bed_cache("qt", source, True)[:, its]
    out = _run("qt", source, points=True, posterior=opt, return_accumulator=True)
    accum = out[2]                                           # read after the run's engine was closed
    assert accum.eng.h is None
    got = {k: v.cpu().numpy() for k, v in accum.local_sums().items()}
    exp, exp_sv, exp_proj = _fed(ch, x, its, posterior.check_options(opt, N_ITER, N), cells)
    assert set(got) == set(exp) == {"partials_sum", "M", "hist_counts", "lag_sqdiff", "probe_cross", "residual_sums", "local_cross"}
    for k in exp:
        assert np.array_equal(got[k], exp[k], equal_nan=True), k
    assert np.array_equal(accum.projections(), exp_proj) and np.array_equal(accum.sample_values(), exp_sv)
    s = accum.finalize()
    used = hc.used_values(x, True)
    counts = hc.hist_counts(used, g, 64, 40.0, opt["hist"]["levels"])
    assert np.array_equal(s.hist_counts, counts[:67]) and np.array_equal(s.level_counts, counts[67:])
    assert np.array_equal(s.sample_values, x[:, :, POINTS[:, 0], POINTS[:, 1]].transpose(0, 2, 1))   # bed units, trend included
    assert np.array_equal(s.sample_loc, ch.sample_loc)
    pc.check_maps(s, _reference(x, True), label=f"sgs every option {source}")
    assert np.isfinite(s.expected_loss()) and s.local_covariance().shape[0] == 12 and s.covariance().shape == (2, H, H)
    # the run's own per-iteration traces stay detrended, and the chains are those of the run without posterior
    plain = _run("qt", source, points=True)
    _same_chains(out, plain, source)
    full = _bed_cache("qt", source, True)
    np.testing.assert_allclose(out[0][0][7][0, 1:], full[0, 1:, 5, 7] - ch.trend[5, 7], rtol=0, atol=1e-9)


def _files(folder):
    return {str(p.relative_to(folder)): p.read_bytes() for p in sorted(folder.rglob("*")) if p.is_file() and p.suffix != ".npz"}


def test_driver(tmp_path, monkeypatch):
    """smallScaleChain_mp: one rank and two self-started ranks (gloo, 3 + 2 chains), with and without posterior"""
    monkeypatch.setenv("GSM_DIST_BACKEND", "gloo")
    prob, ch = _template("qt", points=True)
    beds = [prob["bed"] + np.random.default_rng(40 + i).normal(0, 3, prob["bed"].shape) for i in range(5)]
    seeds = [911, 922, 933, 944, 955]
    opt = dict(burn_in=11, thin=5, hist=dict(bins=32, half_width=40.0))
    res, summ = {}, {}
    for tag, n_gpus, post in (("one", 1, opt), ("two", 2, opt), ("none", 1, None)):
        res[tag] = driver.smallScaleChain_mp(5, 1, ch, beds, seeds, 5, [N_ITER] * 5, output_path=str(tmp_path / tag), mode="pcg64",
                                             n_gpus=n_gpus, posterior=post)
        base = tmp_path / tag / "LargeScaleChain" / "5" / "SmallScaleChain"
        if post is None:
            assert not list(base.glob("posterior_*"))
        else:
            summ[tag] = posterior.PosteriorSummary.load(base / "posterior_0k.npz")
    for tag in ("one", "two"):
        assert len(res[tag]) == 5
        for a, b in zip(res[tag], res["none"]):
            assert all(np.array_equal(np.asarray(x, dtype=float), np.asarray(y, dtype=float), equal_nan=True) for x, y in zip(a, b))
        fa, fb = _files(tmp_path / tag), _files(tmp_path / "none")
        assert fa.keys() == fb.keys() and len(fa) == 5 * 7 and all(fa[k] == fb[k] for k in fa)        # byte for byte
    one, two = summ["one"], summ["two"]
    assert (two.n_chains, two.n_sequences, two.n_per_sequence) == (5, 10, 5) == (one.n_chains, one.n_sequences, one.n_per_sequence)
    assert np.array_equal(two.sample_values, one.sample_values) and two.sample_values.shape == (5, 3, 10)
    assert np.array_equal(two.hist_counts, one.hist_counts) and one.hist_counts.sum() == 5 * 10 * H * H
    pc.check_maps(two, dict(mean=one.mean, sd=one.sd, within_var=one.within_var, between_var_over_n=one.between_var_over_n, rhat=one.rhat),
                  label="sgs driver: two ranks against one")
    # the one-rank summary is the library call's
    out = sgs.run_many_sgs(ch, beds, [np.random.default_rng(seed=s) for s in seeds], N_ITER, pcg64=True, posterior=opt)
    for name in ("mean", "sd", "rhat", "hist_counts", "sample_values"):
        assert np.array_equal(getattr(one, name), getattr(out[2], name), equal_nan=True), name


def test_refusals(tmp_path):
    prob, ch = _template("plain")
    beds = [prob["bed"]] * 2
    call = lambda n_iters, post, **kw: driver.smallScaleChain_mp(2, 1, ch, beds, [1, 2], 5, n_iters, output_path=str(tmp_path), n_gpus=1,
                                                                 posterior=post, **kw)
    with pytest.raises(ValueError, match="same n_iter"):
        call([61, 60], dict(burn_in=0, thin=5))
    with pytest.raises(ValueError, match="snapshots"):
        call([61, 61], dict(burn_in=50, thin=5))
    with pytest.raises(ValueError, match="unknown posterior option"):
        call([61, 61], dict(burn_in=0, thin=5, every=3), mode="philox")
    with pytest.raises(TypeError):
        call([61, 61], True)
    assert not (tmp_path / "LargeScaleChain").exists()       # refused before anything ran or was written
    rngs = [np.random.default_rng(i) for i in range(2)]
    states = [r.bit_generator.state for r in rngs]
    with pytest.raises(ValueError, match="snapshots"):
        sgs.run_many_sgs(ch, beds, rngs, 61, posterior=dict(burn_in=0, thin=40))          # T = 2 < 4 with split
    with pytest.raises(ValueError, match="max_lag"):
        sgs.run_many_sgs(ch, beds, rngs, 61, posterior=dict(burn_in=11, thin=5, ess=True))  # 5 snapshots per sequence, max_lag 7
    assert [r.bit_generator.state for r in rngs] == states   # before a draw was made
