"""GPU suite of the posterior histogram (csrc/posterior_hist_kernel.hip, gsm_posterior_histogram, posterior.py's `hist`): the
device counts, bins and levels alike, EQUAL the NumPy restatement's (tests/posterior_hist_common.py) -- integers, no tolerance.

The snapshots are fed as tests/test_gpu_posterior_many_chains.py feeds them (the engine's beds are set, no chain runs).  The
shapes are the smallest that reach each loop shape of the kernel on a device of 256 compute units; hp.hist_plan restates the
split rule and every case asserts its regime BEFORE it feeds anything, so on another device the test fails with the plan in its
message instead of quietly running one chain per part.  Values are rounded to float so that both state types see the same numbers."""
import ctypes as C

import numpy as np
import pytest

import posterior_common as pc
import posterior_hist_common as hp
from mcmc_gpu_amd import MCMC_gpu, driver, posterior, synthetic
from test_gpu_posterior import _stretched_snapshots, _template_with_points

pytestmark = pytest.mark.gpu

HALF = 400.0
# (H, W, chains) -> (parts, cpp, trips of the 8-chain loop, remainder, chains of the last filled part, empty parts, dead lanes)
REGIME = {
    (16, 16, 3): (3, 1, 0, 1, 1, 0, 0),             # parts = chains, one chain per part
    (127, 129, 101): (16, 7, 0, 7, 3, 1, 1),        # remainder loop only, ragged last part, an empty part, a dead lane
    (128, 128, 390): (16, 25, 3, 1, 15, 0, 0),      # three trips with 8 loads in flight, then the remainder; last part 1 trip + 7
}


def _n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _assert_regime(H, W, Cn):
    plan = hp.hist_plan(H, W, Cn, _n_cu())
    print(f"histogram plan {H}x{W} x {Cn} chains on {_n_cu()} CUs: {plan}")
    got = tuple(plan[k] for k in ("parts", "cpp", "trips", "rem", "last", "empty", "dead"))
    assert got == REGIME[(H, W, Cn)], f"{H}x{W} x {Cn} chains on {_n_cu()} compute units gives {plan}, not the regime this case is here for"


_DATA = {}


def _data(H, W, Cn, T):
    """Snapshots x [C, T, H, W] (float values), the common field g, the planted level and the expected counts by (split, B, levels):
    built once per (grid, chains, T) and kept until the next one is asked for.  Planted at chain 0's last snapshot, row 0: d == 0
    exactly (bin B / 2), +inf, -inf, a finite value beyond each end of the range; the NaN is many_chain_data's own, at cell (5, 7)
    of the last chain; `present` is a value of the data, used as a level."""
    key = (H, W, Cn, T)
    if _DATA.get("key") != key:
        _DATA.clear()
        x, g = pc.many_chain_data(Cn, T, H, W, H * 100 + T, f32=True)
        unplanted = hp.hist_counts(hp.used_values(x, True), g, 64, HALF)
        n = unplanted[:67, 0, 0].sum()
        share = unplanted[[0, 65]].sum() / (n * H * W)
        filled = int((unplanted[1:65].sum(axis=(1, 2)) > 0).sum())
        print(f"unplanted data {key}: underflow + overflow share {share:.2e}, {filled} of 64 bins non-empty somewhere")
        assert share <= 0.01 and filled >= 32
        g[0, 1] = np.float64(np.float32(g[0, 1]))
        x[0, T - 1, 0, 1] = g[0, 1]
        x[0, T - 1, 0, 2], x[0, T - 1, 0, 3] = np.inf, -np.inf
        x[0, T - 1, 0, 4] = np.float64(np.float32(g[0, 4] + 1000.0))
        x[0, T - 1, 0, 5] = np.float64(np.float32(g[0, 5] - 1000.0))
        assert np.isnan(x[Cn - 1, T - 2, 5, 7]) and np.isnan(x).sum() == 1
        assert np.array_equal(x, x.astype(np.float32).astype(np.float64), equal_nan=True)
        _DATA.update(key=key, x=x, g=g, present=float(x[min(1, Cn - 1), T - 1, 3, 3]), exp={}, dev={})
    return _DATA


def _levels(d, L):
    """L levels: first a value present in the data (`<` is strict), then heights spread over the range and beyond it."""
    return tuple([d["present"], -300.0, -250.5, -1e4, 1e4, -700.0, 0.0, -299.0][:L])


def _expected(d, split, B, levels):
    k = (split, B, levels)
    if k not in d["exp"]:
        d["exp"][k] = hp.hist_counts(hp.used_values(d["x"], split), d["g"], B, HALF, levels)
    return d["exp"][k]


def _device(d, state):
    import torch
    if state not in d["dev"]:
        d["dev"].clear()
        d["dev"][state] = torch.as_tensor(d["x"]).to(device="cuda:0", dtype=torch.float64 if state == "f64" else torch.float32)
    return d["dev"][state]


def _feed(dx, g, state_dtype, split, rhat, hist):
    """The snapshots dx [C, T, H, W] (on the device, state dtype) through PosteriorAccumulator.add(); returns the summary and the raw
    int32 counts."""
    import torch
    from mcmc_gpu_amd.engine import GsmEngine
    Cn, T, H, W = dx.shape
    eng = GsmEngine(H, W, Cn, state_dtype=state_dtype)
    try:
        acc = posterior.PosteriorAccumulator(eng, T, 0, 1, split=split, rhat=rhat, common_ref=g, hist=hist)
        assert acc.hist_counts.dtype == torch.int32 and tuple(acc.hist_counts.shape) == (hist.get("bins", 64) + 3 + len(hist.get("levels", ())), H, W)
        eng.beds = torch.empty((Cn, H, W), dtype=eng.state_dtype, device=eng.dev)
        for t in range(T):
            eng.beds.copy_(dx[:, t])
            acc.add()
        return acc.finalize(), acc.hist_counts.cpu().numpy()
    finally:
        eng.close()


def _check(d, summary, raw, split, B, levels, Cn, T):
    H, W = d["g"].shape
    exp = _expected(d, split, B, levels)
    n = Cn * (2 * (T // 2) if split else T)
    assert raw.shape == exp.shape == (B + 3 + len(levels), H, W)
    assert (exp[:B + 3].sum(axis=0) == n).all()
    bad = np.argwhere(raw != exp)
    assert np.array_equal(raw, exp), f"{len(bad)} counts differ, first at (slot, i, j) = {bad[:5].tolist()}"
    assert summary.hist_counts.dtype == np.int64 and np.array_equal(summary.hist_counts, exp[:B + 3])
    assert np.array_equal(summary.level_counts, exp[B + 3:]) and np.array_equal(summary.level_values, np.asarray(levels, dtype=np.float64))
    assert summary.hist_half_width == HALF and np.array_equal(summary.hist_centre, d["g"])
    assert summary.n_sequences * summary.n_per_sequence == n
    # the planted values sit where the slot rule puts them
    assert raw[B // 2 + 1, 0, 1] >= 1 and hp.slots(d["x"][0, T - 1, 0, 1], d["g"][0, 1], B, HALF) == B // 2 + 1
    base = hp.hist_counts(hp.used_values(d["x"][1:], split), d["g"], B, HALF) if Cn <= 3 else None
    if base is not None:                             # few chains: the planted chain's share, cell by cell
        assert raw[B + 1, 0, 2] - base[B + 1, 0, 2] >= 1 and raw[0, 0, 3] - base[0, 0, 3] >= 1
        assert raw[B + 1, 0, 4] - base[B + 1, 0, 4] >= 1 and raw[0, 0, 5] - base[0, 0, 5] >= 1
    assert raw[B + 2, 5, 7] == 1 and raw[B + 2].sum() == 1
    if levels:
        v = hp.used_values(d["x"], split)[:, 3, 3]
        assert (v == levels[0]).sum() >= 1 and raw[B + 3, 3, 3] == (v < levels[0]).sum() < (v <= levels[0]).sum()


@pytest.mark.parametrize("L", [0, 1, 8])
@pytest.mark.parametrize("B", [2, 64, 128])
@pytest.mark.parametrize("state", ["f64", "f32"])
def test_one_chain_per_part_every_bin_and_level_count(state, B, L):
    H, W, Cn, T = 16, 16, 3, 4
    _assert_regime(H, W, Cn)
    d = _data(H, W, Cn, T)
    levels = _levels(d, L)
    s, raw = _feed(_device(d, state), d["g"], state, True, True, dict(bins=B, half_width=HALF, levels=levels))
    _check(d, s, raw, True, B, levels, Cn, T)


@pytest.mark.parametrize("rhat", [True, False])
@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("state", ["f64", "f32"])
@pytest.mark.parametrize("T", [4, 5])
def test_ragged_parts_and_dead_lanes(T, state, split, rhat):
    """Odd T with split drops the first snapshot: the counts sum to M N, not to C T."""
    H, W, Cn = 127, 129, 101
    _assert_regime(H, W, Cn)
    d = _data(H, W, Cn, T)
    levels = _levels(d, 2)
    s, raw = _feed(_device(d, state), d["g"], state, split, rhat, dict(bins=64, half_width=HALF, levels=levels))
    _check(d, s, raw, split, 64, levels, Cn, T)
    if split and T == 5:
        assert (raw[:67].sum(axis=0) == Cn * 4).all()
    assert (s.rhat is not None) == rhat
    q, ex = s.quantile(0.5), hp.numpy_quantile(hp.used_values(d["x"], split), 0.5)
    ok = np.isfinite(ex)
    assert np.array_equal(np.isfinite(q), ok) and (np.abs(q - ex)[ok] < 2 * HALF / 64).all()


def test_many_chains_per_part():
    H, W, Cn, T = 128, 128, 390, 2
    _assert_regime(H, W, Cn)
    d = _data(H, W, Cn, T)
    levels = _levels(d, 3)                           # more than two levels: the kernel's eight-counter form (the other cases: the two-counter one)
    s, raw = _feed(_device(d, "f32"), d["g"], "f32", False, False, dict(bins=64, half_width=HALF, levels=levels))
    _check(d, s, raw, False, 64, levels, Cn, T)


def test_the_call_adds_to_the_counts():
    """Two calls on the same snapshot give twice the counts of one."""
    import torch
    from mcmc_gpu_amd.engine import GsmEngine
    H, W, Cn, T = 16, 16, 3, 4
    d = _data(H, W, Cn, T)
    levels = _levels(d, 2)
    one = hp.hist_counts(d["x"][:, T - 1], d["g"], 64, HALF, levels)
    eng = GsmEngine(H, W, Cn, state_dtype="f64")
    try:
        acc = posterior.PosteriorAccumulator(eng, 2, 0, 1, split=False, rhat=False, common_ref=d["g"], hist=dict(half_width=HALF, levels=levels))
        eng.beds = torch.as_tensor(d["x"][:, T - 1]).to(eng.dev)
        acc.add()
        assert np.array_equal(acc.hist_counts.cpu().numpy(), one)
        acc.add()
        assert np.array_equal(acc.hist_counts.cpu().numpy(), 2 * one)
        assert np.array_equal(acc.finalize().hist_counts, 2 * one[:67])
    finally:
        eng.close()


def test_run_many_with_histogram_end_to_end():
    prob, ch, rf, ij = _template_with_points()
    beds, seeds, n_iter, burn_in, thin, B = synthetic.initial_beds(prob, 4), [5, 6, 7, 8], 61, 1, 10, 32
    its = posterior.snapshot_iterations(n_iter, burn_in, thin)
    assert its.size == 6
    x = _stretched_snapshots(ch, rf, beds, seeds, its)
    g = posterior.default_common_ref(ch.initial_bed)
    v = hp.used_values(x, True)
    assert v.shape[0] == 24
    half = float(np.ceil(np.nanquantile(np.abs(v - g), 0.995)))         # from the snapshots' spread about g
    assert half > 0
    levels = (float(x[0, -1, 30, 30]), float(np.nanmedian(x)))
    exp = hp.hist_counts(v, g, B, half, levels)
    share = exp[[0, B + 1]].sum() / exp[:B + 3].sum()
    print(f"end to end: half_width {half} m, underflow + overflow share {share:.2e}, NaN count {exp[B + 2].sum()}")
    assert share <= 0.01
    opt = dict(burn_in=burn_in, thin=thin)
    for rhat in (True, False):
        plain, sp = MCMC_gpu.run_many(ch, rf, beds, seeds, n_iter, batch=8, posterior=dict(opt, rhat=rhat))
        res, s = MCMC_gpu.run_many(ch, rf, beds, seeds, n_iter, batch=8,
                                   posterior=dict(opt, rhat=rhat, hist=dict(bins=B, half_width=half, levels=list(levels))))
        assert sp.hist_counts is None and sp.level_counts is None
        assert len(res) == len(plain) == 4
        for ra, rb in zip(res, plain):
            assert len(ra) == len(rb) == 7 and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(ra, rb))
        for name in ("mean", "sd", "rhat", "within_var", "between_var_over_n", "sample_values"):
            a, b = getattr(s, name), getattr(sp, name)
            assert (a is None and b is None) or np.array_equal(a, b, equal_nan=True), name
        assert np.array_equal(s.hist_counts, exp[:B + 3]) and np.array_equal(s.level_counts, exp[B + 3:])
        assert (s.hist_counts.sum(axis=0) == 24).all() and s.hist_half_width == half and np.array_equal(s.hist_centre, g)
        w = 2 * half / B
        for q in (0.05, 0.5, 0.95):
            got, ex = s.quantile(q), hp.numpy_quantile(v, q)
            slot = hp.slots(ex, g, B, half)
            ok = (slot >= 1) & (slot <= B)
            assert np.array_equal(np.isfinite(got), ok) and ok.sum() > 0.9 * ok.size
            # the order statistic lies in [lo, lo + w) of its bin and quantile() in (lo, lo + w]: within w, and AT w where a cell never
            # moved (d == 0 is a bin's lower edge) and the rank is the bin's last.  1e-9 m covers quantile()'s three roundings at |x| ~ 1e3 m.
            err = np.abs(got - ex)[ok]
            print(f"end to end rhat={rhat} q={q}: largest |quantile - inverted_cdf| = {err.max() / w:.4f} w")
            assert (err <= w + 1e-9).all(), q
        for l, lv in enumerate(levels):
            assert np.array_equal(s.prob_below(l), (v < lv).sum(axis=0) / 24)


def test_driver_two_ranks_add_their_histograms(tmp_path, monkeypatch):
    """n_gpus=2 without a launcher (two self-started ranks, gloo): ragged shards of 3 and 2 chains, counts summed over the ranks."""
    monkeypatch.setenv("GSM_DIST_BACKEND", "gloo")
    prob, ch, rf, ij = _template_with_points()
    seeds = [31, 32, 33, 34, 35]
    beds = list(synthetic.initial_beds(prob, 5))
    opt = dict(burn_in=20, thin=10, hist=dict(bins=32, half_width=150.0, levels=[-100.0, 0.0]))
    out = {}
    for n in (1, 2):
        driver.largeScaleChain_mp(5, 2, ch, rf, beds, seeds, [120] * 5, output_path=str(tmp_path / f"r{n}"), mode="philox", n_gpus=n, posterior=opt)
        out[n] = posterior.PosteriorSummary.load(tmp_path / f"r{n}" / "LargeScaleChain" / "posterior_0k.npz")
    one, two = out[1], out[2]
    assert (two.n_chains, two.n_sequences, two.n_per_sequence) == (5, 10, 5)
    assert two.hist_counts.shape == (35, 64, 64) and two.hist_counts.dtype == np.int64 and (two.hist_counts.sum(axis=0) == 50).all()
    assert (one.hist_counts[1:33].sum(axis=(1, 2)) > 0).any()
    for name in ("hist_counts", "level_counts", "level_values", "hist_centre"):
        assert np.array_equal(getattr(one, name), getattr(two, name)), name
    assert one.hist_half_width == two.hist_half_width == 150.0
    assert np.array_equal(one.quantile(0.5), two.quantile(0.5), equal_nan=True)


def test_error_paths():
    import torch
    from mcmc_gpu_amd.engine import GsmEngine, _ptr
    eng = GsmEngine(16, 16, 2)
    try:
        b, g = torch.zeros((2, 16, 16), dtype=torch.float64, device=eng.dev), torch.zeros((16, 16), dtype=torch.float64, device=eng.dev)
        cnt = torch.zeros((64 + 3 + 2, 16, 16), dtype=torch.int32, device=eng.dev)
        lv = (C.c_double * 2)(-1.0, 1.0)
        null, st = C.c_void_p(0), eng._stream()
        lib, E_ARG, D = eng.lib, -1, C.c_double
        call = lambda beds=_ptr(b), gg=_ptr(g), inv=0.08, B=64, levels=lv, L=2, counts=_ptr(cnt): \
            lib.gsm_posterior_histogram(eng.h, beds, gg, D(inv), B, levels, L, counts, st)
        assert call(beds=null) == E_ARG and b"NULL" in lib.gsm_last_error(eng.h)
        assert call(gg=null) == E_ARG and call(counts=null) == E_ARG
        for B in (63, 0, 1, -2, 130, 129):
            assert call(B=B) == E_ARG and b"n_bins" in lib.gsm_last_error(eng.h), B
        for L in (-1, 9):
            assert call(L=L) == E_ARG and b"n_levels" in lib.gsm_last_error(eng.h), L
        assert call(levels=null) == E_ARG and b"levels" in lib.gsm_last_error(eng.h)
        for inv in (0.0, -0.5, float("nan"), float("inf")):
            assert call(inv=inv) == E_ARG and b"inv_width" in lib.gsm_last_error(eng.h), inv
        torch.cuda.synchronize()
        assert (cnt == 0).all()                          # nothing ran
        assert call() == 0 and call(levels=null, L=0) == 0
        torch.cuda.synchronize()
        c = cnt.cpu().numpy().reshape(69, 256)
        assert c[33].tolist() == [2 * 2] * 256 and c[68].tolist() == [2] * 256      # d == 0 is bin 32, twice; 0 < 1.0 in the call with levels
        assert c.sum() == 6 * 256                        # and nothing else: 0 < -1.0 never
        eng.beds = b
        with pytest.raises(ValueError, match="counts"):
            eng.posterior_histogram(g, 0.08, 64, (0.0,), cnt)
        with pytest.raises(ValueError, match="hist"):
            posterior.PosteriorAccumulator(eng, 10, 0, 1, hist=dict(half_width=-1.0))
    finally:
        eng.close()
