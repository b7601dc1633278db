"""GPU suite of the posterior covariance with linear functionals (csrc/posterior_cov_kernel.hip, gsm_posterior_project,
gsm_posterior_cross, mcmc_gpu_amd/posterior.py `cov`): both kernels against the extended-precision restatement within the a-priori
bounds, the zero-weight skip and the NaN rules, the instantiations by probe count, the vector widths and the split of the chain
axis, the C entries, the run_many and largeScaleChain_mp paths and two handles.  Definitions and bounds:
tests/posterior_cov_common.py.  The projection bound is asserted on the device's own projections p^ (the accumulator's d_proj);
the summary's probe_values must then be exactly the one host addition Omega_k . g + p^ that defines them."""
import ctypes as C

import numpy as np
import pytest

import posterior_common as pc
import posterior_cov_common as cc
from mcmc_gpu_amd import MCMC_gpu, driver, posterior, synthetic
from test_gpu_posterior import _template_with_points

pytestmark = pytest.mark.gpu

NAN_CELL = (5, 7)


def _n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _feed(x, g, state_dtype, split, probes, rhat=True):
    """x [C, T, H, W] fed snapshot by snapshot through PosteriorAccumulator.add() (no chain is run: the engine's beds are set);
    returns (the summary, the device's projections p^ [C, K, T])."""
    import torch
    from mcmc_gpu_amd.engine import GsmEngine
    Cn, T, H, W = x.shape
    K = probes.shape[0]
    eng = GsmEngine(H, W, Cn, state_dtype=state_dtype)
    try:
        acc = posterior.PosteriorAccumulator(eng, T, 0, 1, split=split, rhat=rhat, common_ref=g, cov=dict(probes=probes))
        assert acc.d_probes.shape == (K, H, W) and acc.d_proj.shape == (T, Cn, K) and acc.probe_cross.shape == (K, H, W)
        assert all(t.dtype == torch.float64 for t in (acc.d_probes, acc.d_proj, acc.probe_cross))
        held = {k: v for k, v in vars(acc).items() if isinstance(v, torch.Tensor)}
        assert acc.device_bytes == sum(v.nbytes for v in held.values())       # the three tensors are in the memory budget
        eng.beds = torch.empty((Cn, H, W), dtype=eng.state_dtype, device=eng.dev)
        for t in range(T):
            eng.beds.copy_(torch.as_tensor(x[:, t]))
            acc.add()
        with pytest.raises(RuntimeError):
            acc.add()
        return acc.finalize(), acc.projections()
    finally:
        eng.close()


def _offsets(probes, g):
    """Omega_k . g over the support, in float64 as the host sums it."""
    return np.array([(w[w != 0] * g[w != 0]).sum() for w in probes])


def _small_data(H, W, Cn, T, f32):
    """The draws of test_gpu_posterior_ess._small_data: a block constant within every chain, a block constant within each half of
    every chain, one NaN at a single (chain, snapshot, cell)."""
    rng = np.random.default_rng(H * 100 + T)
    x = -300.0 + 100.0 * rng.normal(size=(Cn, T, H, W))
    x[:, :, 10:14, 10:20] = x[:, :1, 10:14, 10:20]
    half = T - T // 2
    x[:, :half, 20:22, 5:9] = x[:, :1, 20:22, 5:9]
    x[:, half:, 20:22, 5:9] = x[:, half:half + 1, 20:22, 5:9]
    x[2, T - 2, NAN_CELL[0], NAN_CELL[1]] = np.nan
    g = -300.0 + 10.0 * rng.normal(size=(H, W))
    if f32:
        x = x.astype(np.float32).astype(np.float64)              # the reference sees the same f32 values, cast to f64
    return x, g


def _gaussian_probes(K, H, W, seed, holes=True):
    """K dense Gaussian fields; with holes, a tenth of the weights are set to 0, among them the weight at NAN_CELL."""
    rng = np.random.default_rng(seed)
    P = rng.normal(size=(K, H, W))
    if holes:
        P *= rng.uniform(size=P.shape) > 0.1
        P[:, NAN_CELL[0], NAN_CELL[1]] = 0.0
    return P


def _check_both(s, p_hat, x, g, probes, split, label):
    """The two bounds on one fed summary; returns the end-to-end bound [K, H, W]."""
    Cn, T = x.shape[:2]
    lo = cc.first_used(T, split)
    p, A, m = cc.projection_reference(x, g, probes)
    cc.check_projection(p_hat, p, A, m, label)
    assert np.array_equal(s.probe_values, _offsets(probes, g)[None, :, None] + p_hat, equal_nan=True)
    n = Cn * (T - lo)
    assert n == s.n_sequences * s.n_per_sequence
    return cc.check_cross_both(s.probe_cross, x, g, (p, A, m), p_hat, lo, n, label)


@pytest.mark.parametrize("state_dtype", ["f64", "f32"])
@pytest.mark.parametrize("split,T", [(True, 8), (True, 9), (False, 9)])
def test_small_odd_plane_against_the_restatement(split, T, state_dtype):
    """37 x 41: an odd plane (one cell per lane, a tail workgroup, several plane parts per chain in the project kernel).  Five probes:
    a point on an ordinary cell, a point on the NaN cell, a region mean that excludes the NaN cell, one that includes it, and a dense
    Gaussian field with weight 0 at the NaN cell alone."""
    H, W, Cn = 37, 41, 5
    x, g = _small_data(H, W, Cn, T, state_dtype == "f32")
    nan_flat = NAN_CELL[0] * W + NAN_CELL[1]
    m_out, m_in = np.zeros((H, W), dtype=bool), np.zeros((H, W), dtype=bool)
    m_out[24:30, 11:19] = True
    m_in[3:8, 5:10] = True
    assert not m_out[NAN_CELL] and m_in[NAN_CELL]
    gauss = np.random.default_rng(7).normal(size=(1, H, W))
    gauss[0][NAN_CELL] = 0.0
    probes = np.concatenate([posterior.point_probes(H, W, [15 * W + 20, nan_flat]), posterior.region_mean_probes(np.stack([m_out, m_in])), gauss])
    assert (probes[4] != 0).sum() == H * W - 1
    label = f"{H}x{W} C={Cn} T={T} split={split} {state_dtype}"
    s, p_hat = _feed(x, g, state_dtype, split, probes)
    _check_both(s, p_hat, x, g, probes, split, label)
    # the zero-weight skip: the NaN reaches exactly the two probes whose support holds it, at exactly its chain and snapshot
    hit = np.zeros((Cn, 5, T), dtype=bool)
    hit[2, [1, 3], T - 2] = True
    assert np.array_equal(np.isnan(s.probe_values), hit) and np.array_equal(np.isnan(p_hat), hit)
    # cross: NaN at the NaN cell for every probe; everywhere for the probes with a NaN projection at a snapshot of a sequence
    lo = cc.first_used(T, split)
    whole = hit[:, :, lo:].any(axis=(0, 2))
    assert whole.tolist() == [False, True, False, True, False]
    exp_nan = np.zeros((5, H, W), dtype=bool)
    exp_nan[:, NAN_CELL[0], NAN_CELL[1]] = True
    exp_nan[whole] = True
    assert np.array_equal(np.isnan(s.probe_cross), exp_nan)
    cov = s.covariance()
    assert np.array_equal(np.isnan(cov), exp_nan)
    np.testing.assert_allclose(cov, cc.covariance_formula(s), rtol=1e-13, atol=0)
    with np.errstate(invalid="ignore"):
        rho = s.correlation()
    assert (np.abs(rho[~np.isnan(rho)]) <= 1 + 1e-9).all() and abs(rho[0, 15, 20] - 1.0) <= 1e-9
    # fixed trees, chains in index order, parts in part order: a second feed gives the same bits
    s2, p2 = _feed(x, g, state_dtype, split, probes)
    assert np.array_equal(p2, p_hat, equal_nan=True) and np.array_equal(s2.probe_cross, s.probe_cross, equal_nan=True)
    pc.check_maps(s, pc.posterior_reference(x, split), label=label)


def test_dropped_snapshot_does_not_count():
    """split, T = 9: a NaN in the dropped first snapshot makes its projections NaN there (all T are kept) and touches no cross sum."""
    H, W, Cn, T = 37, 41, 5, 9
    x, g = _small_data(H, W, Cn, T, False)
    x[2, T - 2, NAN_CELL[0], NAN_CELL[1]] = x[2, T - 3, NAN_CELL[0], NAN_CELL[1]]
    x[1, 0, NAN_CELL[0], NAN_CELL[1]] = np.nan
    probes = np.concatenate([posterior.point_probes(H, W, [NAN_CELL[0] * W + NAN_CELL[1]]), _gaussian_probes(1, H, W, 3, holes=False)])
    s, p_hat = _feed(x, g, "f64", True, probes)
    hit = np.zeros((Cn, 2, T), dtype=bool)
    hit[1, :, 0] = True
    assert np.array_equal(np.isnan(s.probe_values), hit)
    assert not np.isnan(s.probe_cross).any() and not np.isnan(s.covariance()).any()
    _check_both(s, p_hat, x, g, probes, True, "dropped snapshot")


@pytest.mark.parametrize("state_dtype", ["f64", "f32"])
@pytest.mark.parametrize("K", [1, 3, 4, 7, 8, 15])
def test_instantiations_and_widths(K, state_dtype):
    """64 x 64 at 16 bytes of bed per lane with either state type; K on both sides of every instantiation's ceiling (3, 7, 15)."""
    H, W, Cn, T = 64, 64, 6, 6
    plan = cc.cross_split_plan(H, W, Cn, state_dtype == "f32", _n_cu())
    assert plan["vec"] * (4 if state_dtype == "f32" else 8) == 16, plan
    x, g = _small_data(H, W, Cn, T, state_dtype == "f32")
    probes = _gaussian_probes(K, H, W, K)
    if K >= 3:
        probes[K - 1][NAN_CELL] = 1.5                                            # the last probe alone has a weight at the NaN cell
    s, p_hat = _feed(x, g, state_dtype, False, probes, rhat=(K % 2 == 1))          # with the per-chain and with the pooled moments
    assert (s.rhat is None) == (K % 2 == 0)
    _check_both(s, p_hat, x, g, probes, False, f"{H}x{W} C={Cn} T={T} K={K} {state_dtype}")
    whole = np.isnan(s.probe_cross).all(axis=(1, 2))
    assert whole.tolist() == [K >= 3 and k == K - 1 for k in range(K)]
    assert np.isnan(s.probe_cross).sum() == whole.sum() * H * W + (K - whole.sum())


@pytest.mark.parametrize("H,W,Cn,state_dtype", list(cc.MANY_PLAN))
def test_many_chains_per_part(H, W, Cn, state_dtype):
    """Many chains per workgroup of the cross pass: multi-trip chain loops, a ragged last part and empty parts, at every vector width."""
    T, K = 4, 3
    plan = cc.cross_split_plan(H, W, Cn, state_dtype == "f32", _n_cu())
    print(f"cross split plan {H}x{W} x {Cn} chains {state_dtype} on {_n_cu()} CUs: {plan}")
    assert (plan["vec"], plan["parts"], plan["cpp"]) == cc.MANY_PLAN[(H, W, Cn, state_dtype)], \
        f"{H}x{W} x {Cn} chains ({state_dtype}) on {_n_cu()} compute units gives {plan}, not the regime this case is here for"
    assert plan["cpp"] >= 5 and plan["last"] < plan["cpp"] and plan["empty"] >= 1, plan
    x, g = pc.many_chain_data(Cn, T, H, W, H * 100 + T, f32=True)
    region = np.zeros((H, W), dtype=bool)
    region[40:60, 30:90] = True
    gauss = np.random.default_rng(5).normal(size=(1, H, W))
    gauss[0][NAN_CELL] = 0.0
    probes = np.concatenate([posterior.point_probes(H, W, [70 * W + 11]), posterior.region_mean_probes(region), gauss])
    s, p_hat = _feed(x, g, state_dtype, False, probes, rhat=False)
    assert not np.isnan(p_hat).any()
    _check_both(s, p_hat, x, g, probes, False, f"{H}x{W} C={Cn} T={T} K={K} {state_dtype}")
    assert np.isnan(s.probe_cross).sum() == K and np.isnan(s.probe_cross[:, NAN_CELL[0], NAN_CELL[1]]).all()


def test_c_entry_points():
    import torch
    from mcmc_gpu_amd.engine import GsmEngine, _ptr
    H, W, Cn, K = 37, 41, 5, 3
    x, g = _small_data(H, W, Cn, 4, False)
    x0 = x[:, 0]
    probes = _gaussian_probes(K, H, W, 9, holes=False)
    eng = GsmEngine(H, W, Cn)
    try:
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(eng.dev)
        b, dg, dp = dev(x0), dev(g), dev(probes)
        proj = torch.full((Cn, K), 7.0, dtype=torch.float64, device=eng.dev)
        cross = torch.full((K, H, W), 7.0, dtype=torch.float64, device=eng.dev)
        null, st = C.c_void_p(0), eng._stream()
        lib, E_ARG = eng.lib, -1
        off8 = C.c_void_p(b.data_ptr() + 8)
        refused_project = [((null, _ptr(dg), _ptr(dp), K, _ptr(proj)), b"NULL"), ((_ptr(b), null, _ptr(dp), K, _ptr(proj)), b"NULL"),
                           ((_ptr(b), _ptr(dg), null, K, _ptr(proj)), b"NULL"), ((_ptr(b), _ptr(dg), _ptr(dp), K, null), b"NULL"),
                           ((_ptr(b), _ptr(dg), _ptr(dp), 0, _ptr(proj)), b"n_probes"), ((_ptr(b), _ptr(dg), _ptr(dp), 16, _ptr(proj)), b"n_probes"),
                           ((off8, _ptr(dg), _ptr(dp), K, _ptr(proj)), b"aligned")]
        for args, word in refused_project:
            assert lib.gsm_posterior_project(eng.h, *args, st) == E_ARG, args
            assert word in lib.gsm_last_error(eng.h), (word, lib.gsm_last_error(eng.h))
        refused_cross = [((null, _ptr(dg), _ptr(proj), K, _ptr(cross)), b"NULL"), ((_ptr(b), null, _ptr(proj), K, _ptr(cross)), b"NULL"),
                         ((_ptr(b), _ptr(dg), null, K, _ptr(cross)), b"NULL"), ((_ptr(b), _ptr(dg), _ptr(proj), K, null), b"NULL"),
                         ((_ptr(b), _ptr(dg), _ptr(proj), 0, _ptr(cross)), b"n_probes"), ((_ptr(b), _ptr(dg), _ptr(proj), 16, _ptr(cross)), b"n_probes"),
                         ((off8, _ptr(dg), _ptr(proj), K, _ptr(cross)), b"aligned")]
        for args, word in refused_cross:
            assert lib.gsm_posterior_cross(eng.h, *args, st) == E_ARG, args
            assert word in lib.gsm_last_error(eng.h), (word, lib.gsm_last_error(eng.h))
        torch.cuda.synchronize()
        assert (proj == 7.0).all() and (cross == 7.0).all()          # nothing was written
        assert lib.gsm_posterior_project(eng.h, _ptr(b), _ptr(dg), _ptr(dp), K, _ptr(proj), st) == 0
        p_hat = proj.cpu().numpy()[:, :, None]                       # [C, K, 1]: the device's own bits
        p, A, m = cc.projection_reference(x0[:, None], g, probes)
        cc.check_projection(p_hat, p, A, m, "C entry")
        cross.zero_()
        assert lib.gsm_posterior_cross(eng.h, _ptr(b), _ptr(dg), _ptr(proj), K, _ptr(cross), st) == 0
        once = cross.cpu().numpy()
        cc.check_cross_given(once, x0[:, None], g, p_hat, 0, Cn, "C entry, one call")
        assert lib.gsm_posterior_cross(eng.h, _ptr(b), _ptr(dg), _ptr(proj), K, _ptr(cross), st) == 0     # ADDED to
        twice = cross.cpu().numpy()
        ref, mag = cc.cross_sums(x0[:, None], g, p_hat, p_hat)
        cc.check_cross(twice, 2 * ref, (2 * Cn + 4) * cc.U * 2 * mag, "C entry, two calls")
        assert np.array_equal(twice, 2 * once)                       # the same sum added to itself: a doubling is exact
        eng.beds = b
        with pytest.raises(ValueError, match="probes"):              # the engine methods check shapes and dtypes first
            eng.posterior_project(dg, dp[:, :, :-1].contiguous(), proj)
        with pytest.raises(ValueError, match="n_probes"):
            eng.posterior_cross(dg, proj, 16, cross)
        with pytest.raises(ValueError, match="proj"):
            eng.posterior_cross(dg, proj[:, :2].contiguous(), K, cross)
    finally:
        eng.close()


def test_run_many_end_to_end():
    prob, ch, rf, ij = _template_with_points()
    beds, seeds, n_iter = synthetic.initial_beds(prob, 8), list(range(11, 19)), 400
    H, W = beds.shape[1:]
    probes = np.concatenate([posterior.point_probes(H, W, [ij[0, 0] * W + ij[0, 1]]), posterior.region_mean_probes(prob["region_mask"] == 1)])
    opt = dict(burn_in=0, thin=50)
    plain, without = MCMC_gpu.run_many(ch, rf, beds, seeds, n_iter, batch=8, posterior=opt)
    res, s = MCMC_gpu.run_many(ch, rf, beds, seeds, n_iter, batch=8, posterior=dict(opt, cov=dict(probes=probes, names=["point", "region"])))
    assert len(res) == len(plain) == 8
    for ra, rb in zip(res, plain):
        assert len(ra) == len(rb) and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(ra, rb))
    assert without.probes is None and without.probe_values is None and without.probe_cross is None and without.probe_names is None
    for name in ("mean", "sd", "rhat", "within_var", "between_var_over_n", "sample_values", "snapshot_iterations", "sample_loc"):
        assert np.array_equal(getattr(s, name), getattr(without, name), equal_nan=True), name
    assert s.probe_names == ("point", "region") and s.probe_values.shape == (8, 2, 8) and s.probe_cross.shape == (2, H, W)
    assert (s.n_sequences, s.n_per_sequence) == (16, 4)
    # a point probe is the sample trace of its cell: one product by 1.0 plus the offset
    assert np.array_equal(s.probe_values[:, 0], s.sample_values[:, 0])
    cov = s.covariance()
    np.testing.assert_allclose(cov, cc.covariance_formula(s), rtol=1e-13, atol=0)
    i, j = ij[0]
    assert abs(cov[0, i, j] - s.sd[i, j] ** 2) <= 1e-9 * s.sd[i, j] ** 2 + 1e-9          # the tolerances of the variances (posterior_common)
    st = s.probe_stats()
    assert abs(st["sd"][0] - s.sd[i, j]) <= 1e-9 * s.sd[i, j] + 1e-9 and st["cov"].shape == (2, 2) and np.isfinite(st["rhat"]).all()
    with pytest.raises(ValueError, match="cov"):
        MCMC_gpu.run_many(ch, rf, beds, seeds, n_iter, batch=8, posterior=dict(opt, cov=dict(probes=probes[:, :-1])))
    with pytest.raises(ValueError, match="cov"):
        MCMC_gpu.run_many(ch, rf, beds, seeds, n_iter, batch=8, posterior=dict(opt, cov=dict(probes=np.zeros((1, H, W)))))


def test_driver_writes_the_fields(tmp_path):
    prob, ch, rf, ij = _template_with_points()
    ch.set_rng_mode("philox")
    seeds, beds = [31, 32, 33], list(synthetic.initial_beds(prob, 3))
    H, W = beds[0].shape
    probes = np.concatenate([posterior.point_probes(H, W, [30 * W + 30]), _gaussian_probes(1, H, W, 2, holes=False)])
    opt = dict(burn_in=20, thin=10, cov=dict(probes=probes, names=("point", "gauss")))
    driver.largeScaleChain_mp(3, 2, ch, rf, beds, seeds, [120] * 3, output_path=str(tmp_path), mode="philox", n_gpus=1, posterior=opt)
    got = posterior.PosteriorSummary.load(tmp_path / "LargeScaleChain" / "posterior_0k.npz")
    _, exp = MCMC_gpu.run_many(ch, rf, np.stack(beds), seeds, 120, batch=8, posterior=opt)
    assert got.probe_names == ("point", "gauss") and got.probe_values.shape == (3, 2, 10) and got.probe_cross.shape == (2, H, W)
    for name in ("probes", "probe_values", "probe_cross", "probe_centre"):
        assert np.array_equal(getattr(got, name), getattr(exp, name), equal_nan=True), name
    assert np.array_equal(got.covariance(), exp.covariance(), equal_nan=True)


def test_two_handles_add():
    """Chains [0:a] and [a:] in two handles: their cross sums add to the one-handle result within the two bounds (another cut of
    the chain axis: the bits may differ), their projections gathered are the one-handle projections exactly."""
    H, W, Cn, T, a = 37, 41, 5, 9, 2
    x, g = _small_data(H, W, Cn, T, False)
    x[2, T - 2, NAN_CELL[0], NAN_CELL[1]] = -123.0
    probes = np.concatenate([posterior.point_probes(H, W, [15 * W + 20]), _gaussian_probes(2, H, W, 4, holes=False)])
    one, p_one = _feed(x, g, "f64", True, probes)
    lo, hi = _feed(x[:a], g, "f64", True, probes), _feed(x[a:], g, "f64", True, probes)
    assert np.array_equal(np.concatenate([lo[0].probe_values, hi[0].probe_values]), one.probe_values)
    assert np.array_equal(np.concatenate([lo[1], hi[1]]), p_one)
    b_lo = _check_both(lo[0], lo[1], x[:a], g, probes, True, "chains [0:2]")
    b_hi = _check_both(hi[0], hi[1], x[a:], g, probes, True, "chains [2:5]")
    _check_both(one, p_one, x, g, probes, True, "one handle")
    p, _, _ = cc.projection_reference(x, g, probes)
    ref, _ = cc.cross_sums(x, g, p, p, cc.first_used(T, True))
    cc.check_cross(lo[0].probe_cross + hi[0].probe_cross, ref, b_lo + b_hi, "two handles")
