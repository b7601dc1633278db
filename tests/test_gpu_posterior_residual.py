"""GPU suite of the posterior residual maps (csrc/posterior_residual_kernel.hip, gsm_posterior_residual, mcmc_gpu_amd/posterior.py
`residual`): the fused pass against gsm_residual's own output summed in extended precision, within the a-priori bounds and with
exact counts; the NaN rules, the borders, the vector widths, the cut of the chain axis, two handles, the C entry, and the run_many
and largeScaleChain_mp paths.  Definitions, cases and bounds: tests/posterior_residual_common.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import posterior_residual_common as rc
from mcmc_gpu_amd import MCMC_gpu, driver, posterior, synthetic
from test_gpu_posterior import _template_with_points

pytestmark = pytest.mark.gpu


def _n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _engine(f, H, W, n_chains, state_dtype="f64"):
    from mcmc_gpu_amd.engine import GsmEngine
    eng = GsmEngine(H, W, n_chains, state_dtype=state_dtype)
    eng.set_static(f["surf"], f["velx"], f["vely"], f["dhdt"], f["smb"], None, np.ones((H, W), dtype=np.uint8), f["mc_mask"], f["resolution"],
                   f["sigma_mc"])
    return eng


def _device_residuals(x, f):
    """r [C, T, H, W]: gsm_residual's output for every fed bed (fp64 handle; x holds the values the state type can represent)."""
    Cn, T, H, W = x.shape
    eng = _engine(f, H, W, Cn)
    try:
        return np.stack([eng.residual(x[:, t]).cpu().numpy() for t in range(T)], axis=1)
    finally:
        eng.close()


@functools.lru_cache(maxsize=None)
def _case(H, W, Cn, T):
    """(x, g, fields, r) of one case, computed once and shared: no test writes into it."""
    x, g, f = rc.case_data(H, W, Cn, T)
    return x, g, f, _device_residuals(x, f)


def _feed(x, g, f, state_dtype, split, levels=rc.LEVELS, rhat=True, extra=None):
    """x [C, T, H, W] fed snapshot by snapshot through PosteriorAccumulator.add() (no chain is run: the engine's beds are set);
    returns the summary."""
    import torch
    Cn, T, H, W = x.shape
    eng = _engine(f, H, W, Cn, state_dtype)
    try:
        acc = posterior.PosteriorAccumulator(eng, T, 0, 1, split=split, rhat=rhat, common_ref=g, residual=dict(levels=levels), **(extra or {}))
        assert acc.d_rg.shape == (H, W) and acc.residual_sums.shape == (3 + len(levels), H, W)
        assert acc.d_rg.dtype == torch.float64 and acc.residual_sums.dtype == torch.float64
        held = {k: v for k, v in vars(acc).items() if isinstance(v, torch.Tensor)}
        assert acc.device_bytes == sum(v.nbytes for v in held.values())       # both tensors are in the memory budget
        assert np.allclose(acc.residual_ref, rc.shift(g, f), rtol=1e-13, atol=1e-9)   # rg is the residual of the common field
        eng.beds = torch.empty((Cn, H, W), dtype=eng.state_dtype, device=eng.dev)
        for t in range(T):
            eng.beds.copy_(torch.as_tensor(x[:, t]))
            acc.add()
        assert "residual_sums" in acc.local_sums()
        return acc.finalize()
    finally:
        eng.close()


def _check(s, r, split, label):
    """Counts, sums and summary methods of a fed summary against the reference on the device's own residuals."""
    T = r.shape[1]
    lo = rc.first_used(T, split)
    ref = rc.reference_sums(r, s.residual_ref, [float(v) for v in s.residual_levels], lo)
    rc.check_sums(s.residual_sums, ref, label)
    rc.check_summary(s, ref, label)
    return ref


@pytest.mark.parametrize("state_dtype", ["f64", "f32"])
@pytest.mark.parametrize("split,T", [(True, 8), (True, 9), (False, 9)])
def test_small_odd_plane(split, T, state_dtype):
    """37 x 41: an odd plane (one cell per lane, two tiles across, a tail tile below).  One NaN bed in the interior and one in the first
    row, one NaN in velx, a loss mask over part of the grid, two levels; with split and T = 9 also a NaN bed in the dropped first
    snapshot."""
    H, W, Cn = 37, 41, 5
    x, g, f, r = _case(H, W, Cn, T)
    dropped = split and T % 2 == 1
    if dropped:                                             # a NaN in the snapshot that belongs to no sequence: it counts nowhere
        x = x.copy()
        x[1, 0, 30, 10] = np.nan
    label = f"{H}x{W} C={Cn} T={T} split={split} {state_dtype}"
    plan = rc.split_plan(H, W, Cn, state_dtype == "f32", _n_cu())
    assert plan["vec"] == 1 and plan["tiles_x"] == 2 and plan["tiles_y"] * plan["ly"] > H, plan
    s = _feed(x, g, f, state_dtype, split)
    ref = _check(s, r, split, label)
    n = Cn * (T - rc.first_used(T, split))
    assert n == s.n_sequences * s.n_per_sequence
    # An interior NaN bed: exactly its four neighbours lose one count -- the cell itself keeps its own, because np.gradient's centred
    # differences do not read the cell they are taken at.  A NaN bed in the first row: that cell (its one-sided difference along the
    # rows reads it), its left and right neighbours and the cell below lose one.  The NaN velocity: exactly its left and right
    # neighbours have no count; its own cell and its other neighbours keep theirs.
    exp = np.full((H, W), n, dtype=np.int64)
    i, j = rc.NAN_BED
    for di, dj in ((0, 1), (0, -1), (1, 0), (-1, 0)):
        exp[i + di, j + dj] -= 1
    i, j = rc.NAN_BED_BORDER
    for di, dj in ((0, 0), (0, 1), (0, -1), (1, 0)):
        exp[i + di, j + dj] -= 1
    i, j = rc.NAN_VELX
    exp[i, j - 1] = exp[i, j + 1] = 0
    assert np.array_equal(s.residual_count(), exp) and exp[i, j] == n and exp[i - 1, j] == n
    assert np.isnan(s.residual_mean()[i, j - 1]) and np.isnan(s.loss_density()[i, j + 1]) and np.isfinite(s.expected_loss())
    # the loss of the states themselves: the mean of nansum(r^2 over the mask) / (2 sigma^2)
    exp_loss, b_loss = rc.summary_reference(ref, s.residual_ref, rc.LEVELS, f["mc_mask"], f["sigma_mc"], n)["expected_loss"]
    direct = rc.direct_loss(r, f["mc_mask"], f["sigma_mc"], rc.first_used(T, split))
    b_shift = rc.shift_rounding_bound(ref, s.residual_ref, f["mc_mask"], f["sigma_mc"], n)
    print(f"expected_loss {label}: {s.expected_loss()!r} against the direct {float(direct)!r}, bounds {float(b_loss):.3e} + {float(b_shift):.3e}")
    assert abs(direct - exp_loss) <= b_shift + 1e-17 * direct and abs(s.expected_loss() - direct) <= b_loss + b_shift + 1e-17 * direct
    assert 0 < f["mc_mask"].sum() < H * W and (s.loss_density()[f["mc_mask"] == 0][exp[f["mc_mask"] == 0] > 0] == 0).all()
    for l in range(len(rc.LEVELS)):                          # both levels cut the ensemble: neither counts nothing nor everything
        assert 0 < s.residual_sums[3 + l].sum() < s.residual_sums[0].sum()
    # a fixed order: a second feed gives the same bits
    again = _feed(x, g, f, state_dtype, split)
    assert np.array_equal(again.residual_sums, s.residual_sums)


@pytest.mark.parametrize("state_dtype", ["f64", "f32"])
@pytest.mark.parametrize("H,W", [(3, 130), (70, 3)])
def test_grids_thinner_than_a_tile(H, W, state_dtype):
    """Every cell touches a border: the one-sided differences of both axes and all four corners."""
    Cn, T = 3, 4
    x, g, f, r = _case(H, W, Cn, T)
    s = _feed(x, g, f, state_dtype, False)
    _check(s, r, False, f"{H}x{W} C={Cn} T={T} {state_dtype}")
    assert (s.residual_count() == Cn * T).all()


@pytest.mark.parametrize("state_dtype", ["f64", "f32"])
def test_sixteen_bytes_per_lane(state_dtype):
    H, W, Cn, T = 64, 64, 6, 6
    plan = rc.split_plan(H, W, Cn, state_dtype == "f32", _n_cu())
    assert plan["vec"] * (4 if state_dtype == "f32" else 8) == 16, plan
    x, g, f, r = _case(H, W, Cn, T)
    s = _feed(x, g, f, state_dtype, False, rhat=(state_dtype == "f64"))                  # with the per-chain and with the pooled moments
    assert (s.rhat is None) == (state_dtype == "f32")
    _check(s, r, False, f"{H}x{W} C={Cn} T={T} {state_dtype}")
    i, j = rc.NAN_VELX
    assert s.residual_count()[i, j - 1] == 0 and s.residual_count()[i, j + 1] == 0 and s.residual_count()[i, j] == Cn * T


@pytest.mark.parametrize("state_dtype", ["f64", "f32"])
@pytest.mark.parametrize("Cn", [130, 390])
def test_many_chains_per_part(Cn, state_dtype):
    """16 x 24, one tile: several chains to a part -- multi-trip chain loops, a ragged last part, empty parts."""
    H, W, T = 16, 24, 2
    plan = rc.split_plan(H, W, Cn, state_dtype == "f32", _n_cu())
    print(f"residual split plan {H}x{W} x {Cn} chains {state_dtype} on {_n_cu()} CUs: {plan}")
    assert plan["tiles_x"] * plan["tiles_y"] == 1 and plan["cpp"] >= 5 and plan["last"] < plan["cpp"] and plan["empty"] >= 1, plan
    x, g, f, r = _case(H, W, Cn, T)
    s = _feed(x, g, f, state_dtype, False, rhat=False)
    _check(s, r, False, f"{H}x{W} C={Cn} T={T} {state_dtype}")


def test_bit_equality_with_gsm_residual():
    """One chain, one counted snapshot, rg = 0: S1 is gsm_residual's output bit for bit where that is finite, cnt is 1 there and 0
    elsewhere.  (The accumulator's shift is zeroed on the device for this: any finite field is a legal shift.)"""
    import torch
    H, W = 37, 41
    x, g, f, r = _case(H, W, 5, 8)
    eng = _engine(f, H, W, 1)
    try:
        acc = posterior.PosteriorAccumulator(eng, 2, 0, 1, split=False, rhat=False, common_ref=g, residual=True)
        acc.d_rg.zero_()
        eng.beds = torch.as_tensor(x[2:3, 6].copy()).to(eng.dev)                          # the chain and snapshot with the NaN bed
        acc.add()
        planes = acc.residual_sums.cpu().numpy()
    finally:
        eng.close()
    r0 = r[2, 6]
    fin = np.isfinite(r0)
    assert planes.shape == (3, H, W) and 0 < (~fin).sum() < 10
    assert np.array_equal(planes[0], fin.astype(np.float64))
    assert np.array_equal(planes[1][fin].view(np.int64), r0[fin].view(np.int64)) and (planes[1][~fin] == 0).all()
    assert np.array_equal(planes[2][fin], r0[fin] * r0[fin]) and (planes[2][~fin] == 0).all()


def test_two_handles_add():
    """Chains [0:2] and [2:5] in two handles: their planes add to the one-handle result, counts exactly, sums within the two bounds."""
    H, W, Cn, T, a = 37, 41, 5, 9, 2
    x, g, f, r = _case(H, W, Cn, T)
    one = _feed(x, g, f, "f64", True)
    lo, hi = _feed(x[:a], g, f, "f64", True), _feed(x[a:], g, f, "f64", True)
    _check(lo, r[:a], True, "chains [0:2]")
    _check(hi, r[a:], True, "chains [2:5]")
    ref = _check(one, r, True, "one handle")
    both = lo.residual_sums + hi.residual_sums
    assert np.array_equal(both[0], one.residual_sums[0]) and np.array_equal(both[3:], one.residual_sums[3:])
    rc.check_sums(both, ref, "two handles")


def test_c_entry_point():
    import torch
    from mcmc_gpu_amd.engine import GsmEngine, _ptr
    H, W, Cn = 37, 41, 5
    x, g, f, r = _case(H, W, Cn, 8)
    eng = _engine(f, H, W, Cn)
    bare = GsmEngine(H, W, Cn)                                                           # static fields never set
    try:
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(eng.dev)
        b, drg = dev(x[:, 0]), dev(rc.shift(g, f))
        sums = torch.full((5, H, W), 7.0, dtype=torch.float64, device=eng.dev)
        null, st = C.c_void_p(0), eng._stream()
        lib, E_ARG, E_STATE = eng.lib, -1, -2
        lv = lambda *v: (C.c_double * len(v))(*v)
        two = lv(*rc.LEVELS)
        refused = [((null, _ptr(drg), two, 2, _ptr(sums)), b"NULL"), ((_ptr(b), null, two, 2, _ptr(sums)), b"NULL"),
                   ((_ptr(b), _ptr(drg), two, 2, null), b"NULL"), ((_ptr(b), _ptr(drg), null, 2, _ptr(sums)), b"NULL"),
                   ((_ptr(b), _ptr(drg), two, -1, _ptr(sums)), b"n_levels"), ((_ptr(b), _ptr(drg), lv(1, 2, 3, 4, 5), 5, _ptr(sums)), b"n_levels"),
                   ((_ptr(b), _ptr(drg), lv(1.0, -2.0), 2, _ptr(sums)), b"levels"), ((_ptr(b), _ptr(drg), lv(float("nan"), 2.0), 2, _ptr(sums)), b"levels"),
                   ((_ptr(b), _ptr(drg), lv(1.0, float("inf")), 2, _ptr(sums)), b"levels"),
                   ((C.c_void_p(b.data_ptr() + 8), _ptr(drg), two, 2, _ptr(sums)), b"aligned")]
        for args, word in refused:
            assert lib.gsm_posterior_residual(eng.h, *args, st) == E_ARG, args
            assert word in lib.gsm_last_error(eng.h), (word, lib.gsm_last_error(eng.h))
        assert lib.gsm_posterior_residual(bare.h, _ptr(b), _ptr(drg), two, 2, _ptr(sums), st) == E_STATE
        assert b"gsm_set_static" in lib.gsm_last_error(bare.h)
        torch.cuda.synchronize()
        assert (sums == 7.0).all()                                                       # nothing was written
        sums.zero_()
        assert lib.gsm_posterior_residual(eng.h, _ptr(b), _ptr(drg), two, 2, _ptr(sums), st) == 0
        once = sums.cpu().numpy()
        ref = rc.reference_sums(r[:, :1], rc.shift(g, f), rc.LEVELS)
        rc.check_sums(once, ref, "C entry, one call")
        assert lib.gsm_posterior_residual(eng.h, _ptr(b), _ptr(drg), two, 2, _ptr(sums), st) == 0       # ADDED to
        assert np.array_equal(sums.cpu().numpy(), 2 * once)                               # the same sums added to themselves: a doubling is exact
        none = torch.zeros((3, H, W), dtype=torch.float64, device=eng.dev)
        assert lib.gsm_posterior_residual(eng.h, _ptr(b), _ptr(drg), null, 0, _ptr(none), st) == 0      # no levels: three planes
        assert np.array_equal(none.cpu().numpy(), once[:3])
        eng.beds = b
        with pytest.raises(ValueError, match="levels"):                                   # the engine method checks its arguments first
            eng.posterior_residual(drg, (1.0, -1.0), sums)
        with pytest.raises(ValueError, match="sums"):
            eng.posterior_residual(drg, rc.LEVELS, none)
        bare.beds = b
        with pytest.raises(RuntimeError, match="set_static"):
            bare.posterior_residual(drg, (), none)
    finally:
        eng.close()
        bare.close()


def test_run_many_end_to_end():
    prob, ch, rf, ij = _template_with_points()
    beds, seeds, n_iter = synthetic.initial_beds(prob, 8), list(range(11, 19)), 400
    H, W = beds.shape[1:]
    opt = dict(burn_in=0, thin=50, hist=dict(half_width=400.0), ess=dict(max_lag=3), cov=dict(probes=posterior.point_probes(H, W, [30 * W + 30])))
    plain, without = MCMC_gpu.run_many(ch, rf, beds, seeds, n_iter, batch=8, posterior=opt)
    res, s = MCMC_gpu.run_many(ch, rf, beds, seeds, n_iter, batch=8, posterior=dict(opt, residual=dict(levels=(2.0, 10.0))))
    assert len(res) == len(plain) == 8
    for ra, rb in zip(res, plain):
        assert len(ra) == len(rb) and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(ra, rb))
    assert all(getattr(without, name) is None for name in ("residual_sums", "residual_ref", "residual_levels", "residual_sigma_mc", "residual_mc_mask"))
    for name in ("mean", "sd", "rhat", "within_var", "between_var_over_n", "sample_values", "snapshot_iterations", "sample_loc", "hist_counts",
                 "level_counts", "lag_sqdiff", "probe_values", "probe_cross"):
        assert np.array_equal(getattr(s, name), getattr(without, name), equal_nan=True), name
    assert s.residual_sums.shape == (5, H, W) and (s.n_sequences, s.n_per_sequence) == (16, 4) and s.residual_sigma_mc == ch.sigma_mc
    assert np.array_equal(s.residual_mc_mask, np.asarray(ch.mc_region_mask) == 1)
    n = s.n_sequences * s.n_per_sequence
    assert s.residual_count().max() == n and (s.residual_count() <= n).all()
    # the mean of the chains' own loss records at the counted snapshot iterations: the project's loss bar (1e-10 relative, README parity
    # row) plus the derived bound of the sums relative to the value (sum |d| <= sqrt(cnt S2) for the S1 bound)
    its = s.snapshot_iterations[len(s.snapshot_iterations) - 2 * s.n_per_sequence:]
    assert len(its) == 8
    recorded = np.mean([res[c][3][its] for c in range(8)])
    P = s.residual_sums.astype(np.longdouble)
    ref = dict(cnt=s.residual_count(), s1=P[1], s2=P[2], abs1=np.sqrt(P[0] * P[2]), above=s.residual_sums[3:].astype(np.int64))
    _, b_loss = rc.summary_reference(ref, s.residual_ref, (2.0, 10.0), s.residual_mc_mask, s.residual_sigma_mc, n)["expected_loss"]
    print(f"expected_loss {s.expected_loss()!r}, mean of the recorded losses {recorded!r}, relative difference "
          f"{abs(s.expected_loss() - recorded) / recorded:.3e}, derived bound {float(b_loss) / recorded:.3e} relative")
    assert abs(s.expected_loss() - recorded) <= 1e-10 * recorded + float(b_loss)
    with pytest.raises(ValueError, match="residual"):
        MCMC_gpu.run_many(ch, rf, beds, seeds, n_iter, batch=8, posterior=dict(burn_in=0, thin=50, residual=dict(levels=(-1.0,))))


def test_driver_writes_the_fields(tmp_path):
    prob, ch, rf, ij = _template_with_points()
    ch.set_rng_mode("philox")
    seeds, beds = [31, 32, 33], list(synthetic.initial_beds(prob, 3))
    H, W = beds[0].shape
    opt = dict(burn_in=20, thin=10, residual=dict(levels=(5.0,)))
    driver.largeScaleChain_mp(3, 2, ch, rf, beds, seeds, [120] * 3, output_path=str(tmp_path), mode="philox", n_gpus=1, posterior=opt)
    got = posterior.PosteriorSummary.load(tmp_path / "LargeScaleChain" / "posterior_0k.npz")
    _, exp = MCMC_gpu.run_many(ch, rf, np.stack(beds), seeds, 120, batch=8, posterior=opt)
    assert got.residual_sums.shape == (4, H, W) and got.residual_levels.tolist() == [5.0] and got.residual_sigma_mc == ch.sigma_mc
    for name in ("residual_sums", "residual_ref", "residual_levels", "residual_mc_mask"):
        assert np.array_equal(getattr(got, name), getattr(exp, name), equal_nan=True), name
    for name in ("residual_mean", "residual_sd", "residual_rms", "residual_count", "loss_density"):
        assert np.array_equal(getattr(got, name)(), getattr(exp, name)(), equal_nan=True), name
    assert got.expected_loss() == exp.expected_loss() and got.expected_loss() > 0
    assert np.array_equal(got.prob_residual_above(5.0), exp.prob_residual_above(5.0), equal_nan=True)
    with pytest.raises(KeyError):
        got.prob_residual_above(6.0)
