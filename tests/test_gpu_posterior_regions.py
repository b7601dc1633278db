"""GPU suite of the posterior region functionals (csrc/posterior_regions_kernel.hip, gsm_posterior_regions, mcmc_gpu_amd/posterior.py
`regions`): the pass on beds set with set_state against the NumPy restatement of tests/posterior_regions_common.py -- counts, min,
max and every hypsometry counter equal, the three sums within (m + 3) u sum |t| of the long-double sum of the bit-equal terms --,
reproducibility, the hypsometry's accumulation, every refusal of the C entry, and the run_many and run_many_sgs paths with and
without the option.

The handle refuses a grid with a side below 3 cells (gsm_set_static, which the pass needs for the surface), so the thinnest grid
here has 3 rows, not 1; that a one-row handle is refused is asserted in test_refusals.

Largest share of the bound a sum took on an MI355X: 0.20 in test_pass_against_restatement and through the accumulator (the two-cell
region, one rounding against (2 + 3) u; 0.19 on 37 x 53); the end-to-end volumes 1.9e-03 (run_many) and 4.8e-03 (run_many_sgs)."""
import ctypes as C
import functools

import numpy as np
import pytest

import posterior_regions_common as rg
from mcmc_gpu_amd import MCMC_gpu, posterior, sgs, synthetic

pytestmark = pytest.mark.gpu

GSM_E_ARG, GSM_E_STATE = -1, -2


def _engine(f, H, W, n_chains, state_dtype="f64", static=True):
    from mcmc_gpu_amd.engine import GsmEngine
    eng = GsmEngine(H, W, n_chains, state_dtype=state_dtype)
    if static:
        eng.set_static(f["surf"], f["velx"], f["vely"], f["dhdt"], f["smb"], None, np.ones((H, W), dtype=np.uint8), f["mc_mask"], f["resolution"],
                       f["sigma_mc"])
    return eng


@functools.lru_cache(maxsize=None)
def _reference(H, W, Cn, f32):
    """(func, A) of the case over all 8 regions, computed once and shared; region k's slots do not depend on the other regions."""
    x, f, m = rg.case(H, W, Cn, f32)
    return rg.reference(x, f["surf"], m)


def _call(eng, bits, K, bins, hyps=None, func=None):
    import torch
    func = torch.full((eng.n_chains, K, 8), 7.0, dtype=torch.float64, device=eng.dev) if func is None else func
    if bins:
        hyps = torch.zeros((eng.n_chains, K, bins + 2), dtype=torch.int32, device=eng.dev) if hyps is None else hyps
        eng.posterior_regions(bits, K, rg.SEA, rg.RATIO, func, rg.HYPS_LO, bins / (rg.HYPS_HI - rg.HYPS_LO), bins, hyps)
    else:
        eng.posterior_regions(bits, K, rg.SEA, rg.RATIO, func)
    return func, hyps


@pytest.mark.parametrize("state_dtype", ["f64", "f32"])
@pytest.mark.parametrize("Cn", rg.CHAINS)
@pytest.mark.parametrize("H,W", rg.GRIDS)
def test_pass_against_restatement(H, W, Cn, state_dtype):
    """K = 1, 3, 8 x 0, 2, 16, 64 bins on one handle.  The bit plane always carries all 8 masks: with K < 8 the higher bits are
    ignored.  Region 0 is the whole domain (NaN and infinite beds and the NaN of surf inside it), 1 and 2 overlap, 3 is empty, 4 one
    cell, 5 all-NaN for two chains, 6 holds the NaN of surf; beds at sea level, one step below it, at bin edges and in both overflow
    slots (posterior_regions_common.case)."""
    import torch
    f32 = state_dtype == "f32"
    x, f, m = rg.case(H, W, Cn, f32)
    ref, A = _reference(H, W, Cn, f32)
    t = rg.terms(x, f["surf"])
    assert t["marine"].any() and (t["below"] & ~t["marine"] & t["valid"]).any() and (~t["below"] & (t["t_haf"] > 0)).any()   # every branch
    assert ((t["t_thick"] == 0) & t["valid"]).any() and (x == rg.SEA).any()
    assert ref[1, 5, 0] == 0 and ref[0, 5, 0] == 2 and ref[0, 3, 0] == 0 and ref[0, 4, 0] == 1 and ref[0, 6, 0] == m[6].sum() - 1
    eng = _engine(f, H, W, Cn, state_dtype)
    try:
        eng.set_state(x)
        assert np.array_equal(eng.beds.cpu().numpy().astype(np.float64), x, equal_nan=True)      # the state type holds the case's values
        bits = torch.as_tensor(posterior.region_bits(m)).to(eng.dev)
        worst = 0.0
        for K in (1, 3, 8):
            for bins in rg.BINS:
                label = f"{H}x{W} C={Cn} {state_dtype} K={K} bins={bins}"
                func, hyps = _call(eng, bits, K, bins)
                got = func.cpu().numpy()
                worst = max(worst, rg.check_func(got, ref[:, :K], A[:, :K], label))
                func2, hyps2 = _call(eng, bits, K, bins, hyps=hyps)
                assert np.array_equal(func2.cpu().numpy(), got), f"{label}: two calls differ"            # bit-identical
                if bins:
                    exp = rg.hyps_reference(x, f["surf"], m[:K], rg.HYPS_LO, bins / (rg.HYPS_HI - rg.HYPS_LO), bins)
                    assert exp[:, 0, 0].min() > 0 and exp[:, 0, bins + 1].min() > 0                      # both overflow slots are used
                    assert np.array_equal(exp.sum(axis=2), ref[:, :K, 0].astype(np.int64))
                    assert np.array_equal(hyps2.cpu().numpy(), 2 * exp), f"{label}: hypsometry"          # added to: the second call doubles
        print(f"{H}x{W} C={Cn} {state_dtype}: worst share of the bound {worst:.3e}")
    finally:
        eng.close()


def test_min_max_of_an_empty_region_and_infinities():
    """A region without a valid cell: count 0, sums 0, min +inf, max -inf -- for the empty region, and for region 5 of the chains
    whose beds are NaN there."""
    import torch
    (H, W), Cn = rg.GRIDS[0], 5
    x, f, m = rg.case(H, W, Cn, False)
    eng = _engine(f, H, W, Cn)
    try:
        eng.set_state(x)
        got = _call(eng, torch.as_tensor(posterior.region_bits(m)).to(eng.dev), 8, 0)[0].cpu().numpy()
    finally:
        eng.close()
    for c, k in [(0, 3), (4, 3)] + [(c, 5) for c in rg.NAN_CHAINS]:
        assert np.array_equal(got[c, k], [0, 0, 0, 0, 0, 0, np.inf, -np.inf]), (c, k, got[c, k])
    assert got[0, 5, 0] == 2 and np.isfinite(got[0, 5]).all()


def test_refusals():
    """Every refusal returns its code and writes nothing: func and hyps keep their fill."""
    import torch
    from mcmc_gpu_amd import _lib
    H, W, Cn = 37, 53, 5
    x, f, m = rg.case(H, W, Cn, False)
    lib = _lib.load()
    eng, bare = _engine(f, H, W, Cn), _engine(f, H, W, Cn, static=False)
    try:
        for e in (eng, bare):
            e.beds = torch.as_tensor(x).to(e.dev)
        bits = torch.as_tensor(posterior.region_bits(m)).to(eng.dev)
        func = torch.full((Cn, 8, 8), 7.0, dtype=torch.float64, device=eng.dev)
        hyps = torch.full((Cn, 8, 66), 5, dtype=torch.int32, device=eng.dev)
        p = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)

        def call(h=eng, beds=eng.beds, bits=bits, K=3, sea=0.0, ratio=rg.RATIO, func=func, lo=-100.0, inv_w=0.1, bins=16, hyps=hyps, off=0):
            rc = lib.gsm_posterior_regions(h.h, C.c_void_p(beds.data_ptr() + off) if beds is not None else None, p(bits), K, sea, ratio, p(func),
                                           lo, inv_w, bins, p(hyps), None)
            torch.cuda.synchronize()
            return rc

        inf, nan = float("inf"), float("nan")
        cases = [("NULL beds", dict(beds=None)), ("NULL region_bits", dict(bits=None)), ("NULL func", dict(func=None)),
                 ("n_regions 0", dict(K=0)), ("n_regions 9", dict(K=9)), ("n_regions -1", dict(K=-1)),
                 ("odd bins", dict(bins=7)), ("bins 1", dict(bins=1)), ("bins 66", dict(bins=66)), ("bins -2", dict(bins=-2)),
                 ("NULL hyps with bins", dict(hyps=None)),
                 ("sea_level inf", dict(sea=inf)), ("sea_level nan", dict(sea=nan)),
                 ("ratio 0", dict(ratio=0.0)), ("ratio < 0", dict(ratio=-1.0)), ("ratio inf", dict(ratio=inf)), ("ratio nan", dict(ratio=nan)),
                 ("inv_width 0", dict(inv_w=0.0)), ("inv_width < 0", dict(inv_w=-0.1)), ("inv_width inf", dict(inv_w=inf)),
                 ("inv_width nan", dict(inv_w=nan)), ("beds off by 8 bytes", dict(off=8))]
        for label, kw in cases:
            assert call(**kw) == GSM_E_ARG, label
            assert "gsm_posterior_regions" in lib.gsm_last_error(eng.h).decode(), label
        assert call(h=bare, beds=bare.beds) == GSM_E_STATE                                     # before gsm_set_static
        assert "gsm_set_static" in lib.gsm_last_error(bare.h).decode()
        assert (func == 7.0).all().item() and (hyps == 5).all().item()                         # nothing was written
        # a non-finite inv_width or a NULL hyps is no error without hypsometry, and the call then writes func only
        assert call(bins=0, hyps=None, inv_w=nan, lo=nan) == 0
        flat, n = func.view(-1), Cn * 3 * 8                                                     # [n_chains, 3, 8] at the head of the buffer
        assert np.array_equal(flat[:n].view(Cn, 3, 8)[..., 0].cpu().numpy(), rg.reference(x, f["surf"], m[:3], 0.0)[0][..., 0].astype(np.float64))
        assert (flat[n:] == 7.0).all().item() and (hyps == 5).all().item()
        # the engine's own checks
        with pytest.raises(ValueError, match="n_regions"):
            eng.posterior_regions(bits, 9, 0.0, 1.1, func)
        with pytest.raises(ValueError, match="n_bins"):
            eng.posterior_regions(bits, 8, 0.0, 1.1, func, 0.0, 1.0, 3, hyps)
        with pytest.raises(ValueError, match="hyps"):
            eng.posterior_regions(bits, 8, 0.0, 1.1, func, 0.0, 1.0, 16, hyps)                # 66 slots given, 18 needed
        with pytest.raises(ValueError, match="region_bits"):
            eng.posterior_regions(bits.to(torch.int32), 8, 0.0, 1.1, func)
        with pytest.raises(ValueError, match="func"):
            eng.posterior_regions(bits, 3, 0.0, 1.1, func)
        with pytest.raises(RuntimeError, match="set_static"):
            bare.posterior_regions(bits, 8, 0.0, 1.1, func)
    finally:
        eng.close()
        bare.close()
    # a grid with a side below 3 cells: the handle exists for gsm_gaussian_filter alone, every other entry refuses it
    from mcmc_gpu_amd.engine import GsmEngine
    row = GsmEngine(1, 64, 2)
    try:
        fr = torch.full((2, 1, 8), 7.0, dtype=torch.float64, device=row.dev)
        beds = torch.zeros((2, 1, 64), dtype=torch.float64, device=row.dev)
        rc = lib.gsm_posterior_regions(row.h, p(beds), p(torch.ones(64, dtype=torch.uint8, device=row.dev)), 1, 0.0, 1.1, p(fr), 0.0, 0.0, 0, None, None)
        torch.cuda.synchronize()
        assert rc == GSM_E_ARG and (fr == 7.0).all().item()
    finally:
        row.close()


def test_accumulator_feeds_every_snapshot_and_counts_the_used_ones():
    """PosteriorAccumulator.add(): the slots of ALL T snapshots, the hypsometry of those that belong to a sequence (split, T = 9:
    the first is dropped); the tensors are in the memory budget; rhat on and off."""
    import torch
    H, W, Cn, T = 37, 53, 5, 9
    x0, f, m = rg.case(H, W, Cn, False)
    x = np.stack([np.roll(x0, t, axis=2) for t in range(T)], axis=1)              # [C, T, H, W]: another bed per snapshot
    opt = dict(masks=m, sea_level=rg.SEA, rho_ice=rg.RHO_ICE, rho_water=rg.RHO_WATER, hyps=dict(lo=rg.HYPS_LO, hi=rg.HYPS_HI, bins=16))
    for rhat in (True, False):
        eng = _engine(f, H, W, Cn)
        try:
            acc = posterior.PosteriorAccumulator(eng, T, 0, 1, split=True, rhat=rhat, regions=opt, local=True)
            assert acc.d_region_bits.shape == (H, W) and acc.d_func.shape == (T, Cn, 8, 8) and acc.region_hyps.shape == (Cn, 8, 18)
            assert acc.region_hyps.dtype == torch.int32 and acc.d_region_bits.dtype == torch.uint8
            held = {k: v for k, v in vars(acc).items() if isinstance(v, torch.Tensor)}
            assert acc.device_bytes == sum(v.nbytes for v in held.values())
            eng.beds = torch.empty((Cn, H, W), dtype=eng.state_dtype, device=eng.dev)
            for t in range(T):
                eng.beds.copy_(torch.as_tensor(x[:, t]))
                acc.add()
            assert not any(k.startswith("region") for k in acc.local_sums())       # per chain: gathered, never summed over ranks
            s = acc.finalize()
        finally:
            eng.close()
        assert s.region_func.shape == (Cn, 8, T, 8) and s.region_names[0] == "region0" and s.region_resolution == f["resolution"]
        for t in range(T):
            ref, A = rg.reference(x[:, t], f["surf"], m)
            rg.check_func(s.region_func[:, :, t], ref, A, f"accumulator rhat={rhat} snapshot {t}")
        exp = sum(rg.hyps_reference(x[:, t], f["surf"], m, rg.HYPS_LO, 16 / 1024.0, 16) for t in range(1, T))
        assert np.array_equal(s.region_hyps, exp)
        assert s.region_values("volume").shape == (Cn, 8, T) and s.hypsometry()["area"].shape == (Cn, 8, 18)
        assert np.isfinite(s.region_stats()["volume_above_flotation"]["q50"][:3]).all()
    eng = _engine(f, H, W, Cn, static=False)
    try:
        with pytest.raises(ValueError, match="set_static"):
            posterior.PosteriorAccumulator(eng, T, 0, 1, regions=opt)
    finally:
        eng.close()


def _volume_check(s, beds, surf, masks, sea, ratio, label):
    """region_values('volume') of the last snapshot against the restatement on the returned beds, at the bar"""
    ref, A = rg.reference(beds, surf, masks, sea, ratio)
    a = float(s.region_resolution) ** 2
    got = s.region_values("volume")[:, :, -1]
    err = np.abs(got.astype(np.longdouble) - ref[..., 2] * np.longdouble(a))
    bound = (ref[..., 0] + 3 + 1) * rg.U * A[..., 2] * a             # one more rounding than the sum's: region_values' product with resolution^2
    print(f"{label}: worst share of the bound {float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0))):.3e}")
    assert (err <= bound).all(), f"{label}: volume of the last snapshot beyond the bound"
    assert np.array_equal(s.region_values("count")[:, :, -1], ref[..., 0].astype(np.float64))
    assert np.array_equal(s.region_values("area_below_sea_level")[:, :, -1], ref[..., 4].astype(np.float64) * a)


def _region_masks(H, W):
    m = np.zeros((3, H, W), dtype=bool)
    m[0] = True
    m[1, H // 4: 3 * H // 4, H // 8: W // 2] = True
    m[2, H // 2:, W // 3:] = True
    return m


def test_run_many_with_and_without_regions():
    """Philox run_many, 64 x 64, 6 chains, 281 iterations, thin 40: T = 8 and the last snapshot is the last iteration."""
    prob, ch, rf = synthetic.template(64)
    beds, seeds, n_iter = synthetic.initial_beds(prob, 6), [5, 6, 7, 8, 9, 10], 281
    m = _region_masks(64, 64)
    sea = float(np.median(prob["bed"]))                              # the beds straddle it
    base = dict(burn_in=0, thin=40, hist=dict(bins=32, half_width=60.0), cov=dict(probes=posterior.region_mean_probes(m[1:])), local=True)
    plain, s0 = MCMC_gpu.run_many(ch, rf, beds, seeds, n_iter, batch=8, posterior=base)
    res, s = MCMC_gpu.run_many(ch, rf, beds, seeds, n_iter, batch=8,
                               posterior=dict(base, regions=dict(masks=m, names=("all", "a", "b"), sea_level=sea, hyps=dict(lo=sea - 400, hi=sea + 400, bins=16))))
    none = MCMC_gpu.run_many(ch, rf, beds, seeds, n_iter, batch=8)
    for other in (plain, none):
        assert len(res) == len(other) == 6
        for ra, rb in zip(res, other):
            assert len(ra) == len(rb) and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(ra, rb))
    for name in ("mean", "sd", "rhat", "within_var", "between_var_over_n", "hist_counts", "probe_values", "probe_cross", "local_cross"):
        assert np.array_equal(getattr(s, name), getattr(s0, name), equal_nan=True), name
    assert s0.region_func is None and s.region_func.shape == (6, 3, 8, 8) and s.region_names == ("all", "a", "b")
    assert s.snapshot_iterations[-1] == n_iter - 1
    out = np.stack([r[0] for r in res])
    below = s.region_values("area_below_sea_level")[:, 0, -1]
    assert (below > 0).all() and (below < 64 * 64 * float(ch.resolution) ** 2).all()
    _volume_check(s, out, ch.surf, m, sea, 1028.0 / 917.0, "run_many")
    hy = s.hypsometry()
    n_valid = s.region_values("count")[:, :, s.region_func.shape[2] - 2 * s.n_per_sequence:].sum(axis=2)
    assert np.array_equal(s.region_hyps.sum(axis=2), n_valid.astype(np.int64)) and hy["mean"].shape == (3, 18)
    st = s.region_stats()
    assert np.isfinite(st["volume"]["rhat"][0]) and (st["volume"]["q025"] <= st["volume"]["q50"]).all()


def test_run_many_sgs_with_and_without_regions():
    """The small template of tests/test_gpu_sgs_posterior.py: 32 x 32, 4 chains, 61 iterations; burn_in 10, thin 5: T = 11 and the last
    snapshot is the last iteration."""
    Hs, N, n_iter = 32, 4, 61

    def run(post):
        prob, ch = synthetic.sgs_template(Hs, transform=True, light=True)         # a fresh chain per run, as the other suites do
        beds = [prob["bed"] + np.random.default_rng(40 + i).normal(0, 3, prob["bed"].shape) for i in range(N)]
        rngs = [np.random.default_rng(900 + i) for i in range(N)]
        out = sgs.run_many_sgs(ch, beds, rngs, n_iter, only_save_last_bed=True, pcg64=True, **({} if post is None else dict(posterior=post)))
        return out, [r.bit_generator.state for r in rngs]

    m = _region_masks(Hs, Hs)
    prob, ch = synthetic.sgs_template(Hs, transform=True, light=True)
    sea = float(np.median(prob["bed"]))
    base = dict(burn_in=10, thin=5, hist=dict(bins=32, half_width=40.0), residual=True)
    none, st_none = run(None)
    plain, st_plain = run(base)
    with_r, st_r = run(dict(base, regions=dict(masks=m, sea_level=sea, hyps=dict(lo=sea - 200, hi=sea + 200, bins=8))))
    assert st_none == st_plain == st_r
    for other in (none, plain):
        for ra, rb in zip(with_r[0], other[0]):
            assert len(ra) == len(rb) and all(np.array_equal(np.asarray(a, dtype=float), np.asarray(b, dtype=float), equal_nan=True) for a, b in zip(ra, rb))
    s, s0 = with_r[2], plain[2]
    for name in ("mean", "sd", "rhat", "within_var", "between_var_over_n", "hist_counts", "residual_sums"):
        assert np.array_equal(getattr(s, name), getattr(s0, name), equal_nan=True), name
    assert s0.region_func is None and s.region_func.shape == (N, 3, 11, 8) and s.snapshot_iterations[-1] == n_iter - 1
    out = np.stack([np.asarray(r[0], dtype=np.float64) for r in with_r[0]])
    assert out.shape == (N, Hs, Hs)
    _volume_check(s, out, ch.surf, m, sea, 1028.0 / 917.0, "run_many_sgs")
    assert s.hypsometry()["edges"].shape == (9,) and s.region_hyps.sum() == int(s.region_values("count")[:, :, 1:].sum())
