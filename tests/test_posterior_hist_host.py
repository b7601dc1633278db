"""CPU suite of the posterior histogram: quantile / interval / prob_below of a PosteriorSummary built from the NumPy restatement of
the counts (tests/posterior_hist_common.py), the `hist` option's errors and the count limit, the summary file with and without
the new fields, the cross-rank sum of counts over gloo, the split rule by hand, and the new symbol of the library."""
import os
import socket
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import posterior_common as pc
import posterior_hist_common as hp
from mcmc_gpu_amd import _lib, posterior

ROOT = Path(__file__).resolve().parent.parent

C, T, H, W, B, HALF = 101, 4, 8, 9, 64, 400.0
WIDTH = 2 * HALF / B
UNDER, CONST, NAN = (1, 1), (2, 2), (5, 7)


def _planted():
    """(x [C, T, H, W], g) of pc.many_chain_data with three planted cells: UNDER has a tenth of its values far below the range
    (its 5 % quantile is in the underflow slot, its median is not), CONST holds one value, NAN is the data's own NaN cell."""
    x, g = pc.many_chain_data(C, T, H, W, 0)
    assert np.isnan(x[C - 1, T - 2][NAN]) and np.isnan(x).sum() == 1
    x[:10, :, UNDER[0], UNDER[1]] = g[UNDER] - 2 * HALF
    x[:, :, CONST[0], CONST[1]] = np.float64(np.float32(-287.3))
    return x, g


def _summary(x, g, split=True, levels=(), bins=B, half=HALF):
    v = hp.used_values(x, split)
    cnt = hp.hist_counts(v, g, bins, half, levels)
    n_seq = 2 if split else 1
    N = x.shape[1] // 2 if split else x.shape[1]
    s = posterior.finalize(pc.numpy_pooled_partials(x, split, g), x.shape[0] * n_seq, N, g, rhat=False, n_chains=x.shape[0],
                           snapshot_iterations=np.arange(x.shape[1]), burn_in=0, thin=1, split=split,
                           hist_counts=cnt[:bins + 3], hist_half_width=half, hist_centre=g,
                           level_values=np.asarray(levels, dtype=np.float64), level_counts=cnt[bins + 3:])
    return s, v, cnt


def test_quantiles_within_one_bin_width_of_numpy():
    x, g = _planted()
    s, v, cnt = _summary(x, g)
    n = v.shape[0]
    assert n == C * T == s.n_sequences * s.n_per_sequence and (cnt[:B + 3].sum(axis=0) == n).all()
    plain = pc.many_chain_data(C, T, H, W, 0)
    share = hp.hist_counts(hp.used_values(plain[0], True), plain[1], B, HALF)[[0, B + 1]].sum() / (n * H * W)
    print(f"underflow + overflow share of the unplanted data: {share:.2e}")
    assert share <= 0.01
    worst = 0.0
    for q in (0.05, 0.5, 0.95):
        got, exp = s.quantile(q), hp.numpy_quantile(v, q)
        exp_slot = hp.slots(exp, g, B, HALF)
        in_range = (exp_slot >= 1) & (exp_slot <= B)                 # NaN cells have slot B + 2
        assert np.array_equal(np.isfinite(got), in_range), q
        assert in_range.sum() >= H * W - 2
        err = np.abs(got - exp)[in_range].max() / WIDTH
        worst = max(worst, err)
        print(f"q={q}: largest |quantile - inverted_cdf| = {err:.3f} w over {in_range.sum()} cells")
        assert (np.abs(got - exp)[in_range] < WIDTH).all(), q
    assert worst < 1.0
    # planted cells
    assert np.isnan(s.quantile(0.05)[UNDER]) and np.isfinite(s.quantile(0.5)[UNDER]) and cnt[0][UNDER] == 10 * T
    assert all(np.isnan(s.quantile(q)[NAN]) for q in (0.05, 0.5, 0.95)) and cnt[B + 2][NAN] == 1 and cnt[B + 2].sum() == 1
    k = int(hp.slots(x[0, 0][CONST], g[CONST], B, HALF))
    assert cnt[k][CONST] == n and 1 <= k <= B
    lo = g[CONST] + (k - 1 - B // 2) * WIDTH
    for q in (0.05, 0.5, 1.0):
        assert lo < s.quantile(q)[CONST] <= lo + WIDTH and abs(s.quantile(q)[CONST] - (lo + q * WIDTH)) < 1e-9
    lo5, hi5 = s.interval(0.9)
    assert np.array_equal(lo5, s.quantile((1 - 0.9) / 2), equal_nan=True) and np.array_equal(hi5, s.quantile((1 + 0.9) / 2), equal_nan=True)
    assert np.allclose(lo5, s.quantile(0.05), rtol=0, atol=1e-9, equal_nan=True)
    ok = np.isfinite(lo5) & np.isfinite(hi5)
    assert (lo5[ok] <= s.quantile(0.5)[ok]).all() and (s.quantile(0.5)[ok] <= hi5[ok]).all()
    for bad in (0.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            s.quantile(bad)
    with pytest.raises(ValueError):
        s.interval(1.0)


@pytest.mark.parametrize("split", [True, False])
def test_prob_below_is_exact(split):
    x, g = _planted()
    present = float(x[3, T - 1, 4, 4])                               # a level equal to a value of the data: `<` is strict
    levels = (-300.0, present, -1e9, 1e9)
    s, v, cnt = _summary(x, g, split=split, levels=levels)
    n = v.shape[0]
    for l, lv in enumerate(levels):
        with np.errstate(invalid="ignore"):
            exp = (v < lv).sum(axis=0) / n
        assert np.array_equal(s.prob_below(l), exp), lv
    assert (v[:, 4, 4] == present).sum() >= 1 and (v[:, 4, 4] <= present).sum() > (v[:, 4, 4] < present).sum() == cnt[B + 3 + 1][4, 4]
    assert (s.prob_below(2) == 0).all() and (np.delete(s.prob_below(3).ravel(), NAN[0] * W + NAN[1]) == 1).all()
    assert s.prob_below(3)[NAN] == (n - 1) / n                       # a NaN is below no level
    plain = posterior.finalize(pc.numpy_pooled_partials(x, split, g), 2, 2, g, rhat=False, n_chains=1, snapshot_iterations=np.arange(4),
                               burn_in=0, thin=1, split=split)
    for call in (lambda: plain.quantile(0.5), lambda: plain.prob_below(0), lambda: plain.interval(0.9)):
        with pytest.raises(ValueError, match="histogram"):
            call()


def test_small_bin_counts():
    """B = 2 and B = 128 through the same quantile rule."""
    x, g = pc.many_chain_data(C, T, H, W, 1)
    for bins in (2, 128):
        s, v, cnt = _summary(x, g, bins=bins)
        w = 2 * HALF / bins
        got, exp = s.quantile(0.5), hp.numpy_quantile(v, 0.5)
        ok = np.isfinite(exp)
        assert np.array_equal(np.isfinite(got), ok) and (np.abs(got - exp)[ok] < w).all()


def test_hist_option_errors():
    ok = dict(burn_in=0, thin=1)
    opt = posterior.check_options(dict(ok, hist=dict(half_width=250)), 10)
    assert opt["hist"] == dict(bins=64, half_width=250.0, levels=())
    assert posterior.check_options(ok, 10)["hist"] is None and posterior.check_options(dict(ok, hist=None), 10)["hist"] is None
    opt = posterior.check_options(dict(ok, hist=dict(bins=128, half_width=1.5, levels=[0.0, -50])), 10)
    assert opt["hist"] == dict(bins=128, half_width=1.5, levels=(0.0, -50.0))
    assert posterior.check_options(dict(ok, hist=dict(bins=2, half_width=1, levels=np.arange(8.0))), 10)["hist"]["levels"] == tuple(range(8))
    bad = [dict(half_width=100, width=3),                            # unknown sub-key
           dict(bins=64),                                            # half_width is required
           dict(half_width=100, bins=63), dict(half_width=100, bins=0), dict(half_width=100, bins=130), dict(half_width=100, bins=64.0),
           dict(half_width=100, bins=True), dict(half_width=100, bins=-2),
           dict(half_width=0), dict(half_width=-5.0), dict(half_width=float("nan")), dict(half_width=float("inf")), dict(half_width="wide"),
           dict(half_width=100, levels=list(range(9))),              # more than 8 levels
           dict(half_width=100, levels=[0.0, float("nan")]), dict(half_width=100, levels=[float("-inf")]), dict(half_width=100, levels=["sea"]),
           "hist", 64]
    for h in bad:
        with pytest.raises(ValueError):
            posterior.check_options(dict(ok, hist=h), 10)
    with pytest.raises(ValueError, match="snapshots"):               # refused like any other schedule
        posterior.check_options(dict(burn_in=8, thin=1, hist=dict(half_width=100)), 10)


def test_count_overflow_is_refused():
    h = dict(half_width=100)
    # split, T = 10: 10 used snapshots per chain
    posterior.check_options(dict(burn_in=0, thin=1, hist=h), 10, n_chains=(2 ** 31 - 1) // 10)
    with pytest.raises(ValueError, match="int32"):
        posterior.check_options(dict(burn_in=0, thin=1, hist=h), 10, n_chains=(2 ** 31 - 1) // 10 + 1)
    # odd T with split drops a snapshot: 8 of 9 count
    posterior.check_options(dict(burn_in=1, thin=1, hist=h), 10, n_chains=(2 ** 31 - 1) // 8)
    with pytest.raises(ValueError, match="int32"):
        posterior.check_options(dict(burn_in=1, thin=1, hist=h), 10, n_chains=(2 ** 31 - 1) // 8 + 1)
    posterior.check_options(dict(burn_in=1, thin=1, split=False, hist=h), 10, n_chains=(2 ** 31 - 1) // 9)
    with pytest.raises(ValueError, match="int32"):
        posterior.check_options(dict(burn_in=1, thin=1, split=False, hist=h), 10, n_chains=(2 ** 31 - 1) // 9 + 1)
    posterior.check_options(dict(burn_in=0, thin=1), 10, n_chains=2 ** 40)           # no histogram, no limit
    with pytest.raises(ValueError, match="int32"):
        posterior.check_hist_count(2 ** 28, 10, 0, 1, True)


def test_summary_file_with_and_without_the_histogram(tmp_path):
    x, g = _planted()
    s, v, cnt = _summary(x, g, levels=(-300.0, -250.0))
    s.save(tmp_path / "with.npz")
    t = posterior.PosteriorSummary.load(tmp_path / "with.npz")
    for name in ("hist_counts", "hist_centre", "level_values", "level_counts", "mean", "sd"):
        assert np.array_equal(getattr(s, name), getattr(t, name), equal_nan=True), name
    assert t.hist_counts.dtype == np.int64 and t.level_counts.dtype == np.int64 and t.hist_counts.shape == (B + 3, H, W)
    assert t.hist_half_width == HALF and isinstance(t.hist_half_width, float)
    assert np.array_equal(t.quantile(0.5), s.quantile(0.5), equal_nan=True) and np.array_equal(t.prob_below(1), s.prob_below(1))
    # a summary saved without the new fields (what the code wrote before it had them) still loads
    old = posterior.finalize(pc.numpy_pooled_partials(x, True, g), 2 * C, T // 2, g, rhat=False, n_chains=C, snapshot_iterations=np.arange(T),
                             burn_in=0, thin=1, split=True)
    old.save(tmp_path / "without.npz")
    with np.load(tmp_path / "without.npz") as z:
        assert not any(k.startswith("hist_") or k.startswith("level_") for k in z.files)
    u = posterior.PosteriorSummary.load(tmp_path / "without.npz")
    assert u.hist_counts is None and u.hist_half_width is None and u.hist_centre is None and u.level_values is None and u.level_counts is None
    assert np.array_equal(u.mean, old.mean, equal_nan=True)


def test_hist_plan_hand_computed_cases():
    """The split rule on 256 compute units, worked by hand from the comments of posterior_hist_kernel.hip."""
    assert hp.hist_plan(16, 16, 3, 256) == dict(cell_blocks=1, dead=0, parts=3, cpp=1, trips=0, rem=1, last=1, last_trips=0, last_rem=1, empty=0)
    # 16383 cells: 64 workgroups, one dead lane; 1024 / 64 = 16 parts of ceil(101 / 16) = 7 chains, 15 of them hold chains
    assert hp.hist_plan(127, 129, 101, 256) == dict(cell_blocks=64, dead=1, parts=16, cpp=7, trips=0, rem=7, last=3, last_trips=0, last_rem=3,
                                                     empty=1)
    assert hp.hist_plan(128, 128, 390, 256) == dict(cell_blocks=64, dead=0, parts=16, cpp=25, trips=3, rem=1, last=15, last_trips=1, last_rem=7,
                                                     empty=0)
    pl = hp.hist_plan(256, 256, 1024, 256)                           # production: 256 workgroups x 4 parts of 256 chains
    assert (pl["parts"], pl["cpp"], pl["trips"], pl["rem"]) == (4, 256, 32, 0)
    pl = hp.hist_plan(1024, 1024, 200000, 256)                       # one part by the fill rule: raised so that 16 bits hold a part
    assert pl["parts"] == 4 and pl["cpp"] == 50000 <= hp.HIST_MAX_CPP


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


LEVELS2 = (-300.0, -200.0)


def _worker(rank, world, port, n_chains, q):
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import posterior_common as pc_
    import posterior_hist_common as hp_
    from mcmc_gpu_amd import parallel
    parallel.init_distributed("gloo")
    lo, hi = parallel.shard_bounds(n_chains, world, rank)
    x, g = pc_.many_chain_data(n_chains, 4, 8, 9, 5)
    local = hp_.hist_counts(hp_.used_values(x[lo:hi], True), g, 64, 400.0, LEVELS2).astype(np.int32)
    tot = parallel.all_reduce_counts(torch.as_tensor(local))
    parallel.barrier()
    q.put((rank, tot.numpy(), str(tot.dtype)))
    torch.distributed.destroy_process_group()


def test_all_reduce_counts_world2_ragged():
    n_chains, world = 7, 2
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n_chains, q)) for r in range(world)]
    for p in procs:
        p.start()
    outs = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    x, g = pc.many_chain_data(n_chains, 4, 8, 9, 5)
    exp = hp.hist_counts(hp.used_values(x, True), g, 64, 400.0, LEVELS2)
    assert (exp[:67].sum(axis=0) == 28).all()
    for rank, tot, dtype in outs:
        assert dtype == "torch.int64" and np.array_equal(tot, exp), rank
    # one process, no group: the counts come back as int64, unchanged
    from mcmc_gpu_amd import parallel
    alone = parallel.all_reduce_counts(torch.as_tensor(exp.astype(np.int32)))
    assert alone.dtype == torch.int64 and np.array_equal(alone.numpy(), exp)


def test_library_exports_the_histogram_entry_point():
    assert "gsm_posterior_histogram" in _lib.declared_symbols()
    assert "posterior_hist_kernel.hip" in _lib.SOURCES
    assert hasattr(_lib.load(), "gsm_posterior_histogram")
