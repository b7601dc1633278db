"""CPU suite of the posterior's effective sample size (mcmc_gpu_amd/posterior.py, `ess`): the option checks, the host arithmetic
of PosteriorSummary.autocorrelation / ess / mcse against the cell-by-cell restatement of tests/posterior_ess_common.py, the
estimator against AR(1) sequences of known autocorrelation time, the summary file, the exported entry point and the rank sum."""
import os
import socket
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import posterior_common as pc
import posterior_ess_common as ec
from mcmc_gpu_amd import _lib, posterior

ROOT = Path(__file__).resolve().parent.parent


def test_ess_option_checks():
    ok = dict(burn_in=0, thin=1, split=False)
    assert posterior.check_options(ok, 20)["ess"] is None and posterior.check_options(dict(ok, ess=None), 20)["ess"] is None
    assert posterior.check_options(dict(ok, ess=True), 20)["ess"] == dict(max_lag=7)
    assert posterior.check_options(dict(ok, ess={}), 20)["ess"] == dict(max_lag=7)
    assert posterior.check_options(dict(ok, ess=dict(max_lag=15)), 20)["ess"] == dict(max_lag=15)
    assert posterior.check_options(dict(ok, ess=dict(max_lag=np.int64(1))), 20)["ess"] == dict(max_lag=1)
    assert "ess" in posterior.POSTERIOR_KEYS
    for bad in (dict(max_lag=7, lag=3), dict(max_lag=6), dict(max_lag=0), dict(max_lag=-1), dict(max_lag=17), dict(max_lag=7.0),
                dict(max_lag=True), dict(max_lag="7"), 7, "yes"):
        with pytest.raises(ValueError, match="ess"):
            posterior.check_options(dict(ok, ess=bad), 20)
    # max_lag <= N - 1: lag t needs N - t >= 1 pairs per sequence.  T = 8: N = 8 unsplit, 4 split
    assert posterior.check_options(dict(burn_in=0, thin=1, split=False, ess=dict(max_lag=7)), 8)["ess"] == dict(max_lag=7)
    assert posterior.check_options(dict(burn_in=0, thin=1, split=True, ess=dict(max_lag=3)), 8)["ess"] == dict(max_lag=3)
    with pytest.raises(ValueError, match="max_lag"):
        posterior.check_options(dict(burn_in=0, thin=1, split=False, ess=dict(max_lag=9)), 8)
    with pytest.raises(ValueError, match="max_lag"):
        posterior.check_options(dict(burn_in=0, thin=1, split=True, ess=dict(max_lag=5)), 8)
    with pytest.raises(ValueError, match="max_lag"):
        posterior.check_options(dict(burn_in=0, thin=1, split=True, ess=True), 14)          # the default 7 > N - 1 = 6
    with pytest.raises(ValueError, match="rhat"):
        posterior.check_options(dict(ok, rhat=False, ess=True), 20)
    assert posterior.check_options(dict(ok, rhat=False, ess=None), 20)["ess"] is None
    with pytest.raises(ValueError, match="unknown posterior"):
        posterior.check_options(dict(ok, ESS=True), 20)


def _summary(S, W, B, mean, sd, M, N, split=False):
    return posterior.PosteriorSummary(mean=mean, sd=sd, rhat=np.sqrt(((N - 1) / N * W + B) / np.where(W == 0, np.nan, W)), within_var=W,
                                      between_var_over_n=B, n_chains=M // (2 if split else 1), n_sequences=M, n_per_sequence=N,
                                      snapshot_iterations=np.arange(N * (2 if split else 1)), burn_in=0, thin=1, split=split, lag_sqdiff=S)


def _planted_maps(K, M, N, seed):
    """Random W, B, S with rho_t mostly in (-0.5, 1), and the cells the definitions single out planted by their exact rho_t:
    S_t = 2 var+ M (N - t) (1 - rho_t) in numbers that are exact in binary."""
    rng = np.random.default_rng(seed)
    H, Wd = 12, 11
    W = rng.uniform(0.5, 2.0, size=(H, Wd))
    B = rng.uniform(0.0, 0.5, size=(H, Wd))
    rho = rng.uniform(-0.5, 1.0, size=(K, H, Wd)) * np.exp(-0.3 * np.arange(K))[:, None, None]
    W[0, :3] = 0.0                                                   # W == 0: NaN
    plant = {(2, 2): [-1.5] + [0.25] * (K - 1),                      # P_0 = -0.5 < 0: no pair is summed, tau = -1 before the floor
             (3, 3): [1.0, -0.5, -0.49] + [0.5] * (K - 3),           # pairs (2.0, -0.99): tau = 3, then cut
             (4, 4): [0.5] * K,                                      # no negative pair: truncated
             (5, 5): [-0.75] + [0.001] * (K - 1)}                    # P_0 = 0.25, then 0.002: tau near -0.5 before the floor, floor active
    for (i, j), r in plant.items():
        W[i, j], B[i, j] = 1.0, 0.25                                 # var+ = (N - 1)/N + 0.25
        rho[:, i, j] = r[:K]
    vp = (N - 1) / N * W + B
    S = np.stack([2.0 * vp * M * (N - t) * (1.0 - rho[t - 1]) for t in range(1, K + 1)])
    mean = rng.normal(size=(H, Wd))
    mean[7, 7] = np.nan                                              # the cell saw a NaN
    sd = rng.uniform(1.0, 2.0, size=(H, Wd))
    return S, W, B, mean, sd


@pytest.mark.parametrize("K,M,N", [(7, 8, 16), (3, 10, 4), (1, 4, 9), (15, 6, 40)])
def test_host_arithmetic_against_the_cell_loop(K, M, N):
    S, W, B, mean, sd = _planted_maps(K, M, N, K * 100 + N)
    s = _summary(S, W, B, mean, sd, M, N)
    rho_e, ess_e, trunc_e, mcse_e, tau_raw = ec.ess_loop(S, W, B, mean, sd, M, N)
    rho = s.autocorrelation()
    ess, trunc = s.ess()
    mcse = s.mcse()
    assert rho.shape == (K, 12, 11) and ess.shape == trunc.shape == mcse.shape == (12, 11) and trunc.dtype == bool
    for got, exp, name in ((rho, rho_e, "rho"), (ess, ess_e, "ess"), (mcse, mcse_e, "mcse")):
        assert np.array_equal(np.isnan(got), np.isnan(exp)), name
        np.testing.assert_allclose(got, exp, rtol=1e-13, atol=0, err_msg=name)
    assert np.array_equal(trunc, trunc_e)
    nan = np.zeros((12, 11), dtype=bool)
    nan[0, :3] = True
    nan[7, 7] = True
    assert np.array_equal(np.isnan(ess), nan) and np.isnan(rho[:, nan]).all() and np.isfinite(rho[:, ~nan]).all() and not trunc[nan].any()
    floor = 1.0 / np.log10(M * N)
    # the planted cells, by their exact values
    assert tau_raw[2, 2] == -1.0 and not trunc[2, 2] and ess[2, 2] == M * N / floor
    assert abs(rho[0, 2, 2] + 1.5) < 1e-12
    if K >= 3:
        assert abs(tau_raw[3, 3] - 3.0) < 1e-12 and not trunc[3, 3] and abs(ess[3, 3] - M * N / 3.0) < 1e-9
    else:
        assert trunc[3, 3]                                           # the negative pair lies beyond max_lag
    assert trunc[4, 4] and abs(tau_raw[4, 4] - (2.0 + (K - 1))) < 1e-12 and abs(ess[4, 4] - M * N / (K + 1.0)) < 1e-9
    assert abs(tau_raw[5, 5] - (-0.5 + 0.002 * (K - 1))) < 1e-12 and tau_raw[5, 5] < floor and ess[5, 5] == M * N / floor and trunc[5, 5]
    assert (ess[~nan] <= M * N / floor * (1 + 1e-15)).all() and (ess[~nan] > 0).all()
    assert np.array_equal(mcse[~nan], (sd / np.sqrt(ess))[~nan])


def _sequence_summary(x, K):
    """PosteriorSummary of the sequences x [M, N, cells] (cells a multiple of 20) with NumPy's W, B and the restated S_t."""
    M, N, cells = x.shape
    x4 = x.reshape(M, N, 20, cells // 20)
    ref = pc.posterior_reference(x4, False)
    S = ec.lag_sqdiff_reference(x4, False, K).astype(np.float64)
    return _summary(S, ref["within_var"], ref["between_var_over_n"], ref["mean"], ref["sd"], M, N), S, ref


def test_ar1_autocorrelation_time():
    """AR(1) with coefficient 0.5: tau = (1 + phi) / (1 - phi) = 3, ESS / (M N) = 1/3.  With a fresh default_rng(3) per case the
    definitions give, in vectorised NumPy and in the cell loop alike, a mean of 0.3288 over the 400 cells, 0.286 .. 0.371 cell by
    cell and 25 % truncated; white noise at N = 100, K = 7 gives 0.9775.  (The SECOND draw of one default_rng(3) gives
    0.3294, 0.281 .. 0.377 and 18 % for the same definitions at K = 15: other draws, not another estimator.)"""
    M, N = 64, 200
    x = ec.ar1_chains(0.5, M, N, 400, 200)
    s, S, ref = _sequence_summary(x, 15)
    ess, trunc = s.ess()
    share = ess / (M * N)
    _, ess_e, trunc_e, _, _ = ec.ess_loop(S, ref["within_var"], ref["between_var_over_n"], ref["mean"], ref["sd"], M, N)
    print(f"AR(1) phi=0.5 K=15: mean ESS/(MN) {share.mean():.4f}, min {share.min():.3f}, max {share.max():.3f}, truncated {trunc.mean():.0%}; "
          f"restatement mean {(ess_e / (M * N)).mean():.4f}")
    np.testing.assert_allclose(ess, ess_e, rtol=1e-13, atol=0)
    assert np.array_equal(trunc, trunc_e)
    assert abs(share.mean() - 1.0 / 3.0) <= 0.02
    assert (share >= 0.2).all() and (share <= 0.5).all()
    rho = s.autocorrelation()
    assert abs(rho[0].mean() - 0.5) < 0.01 and abs(rho[1].mean() - 0.25) < 0.01
    # white noise
    M, N = 64, 100
    xw = np.random.default_rng(3).normal(size=(M, N + 200, 400))[:, 200:]
    sw, _, _ = _sequence_summary(xw, 7)
    white = sw.ess()[0] / (M * N)
    print(f"white noise N=100 K=7: mean ESS/(MN) {white.mean():.4f}")
    assert 0.9 <= white.mean() <= 1.05
    mc = sw.mcse()
    assert np.allclose(mc, sw.sd / np.sqrt(sw.ess()[0]), rtol=1e-15)


def test_split_pairs_do_not_straddle_the_halves():
    """The restated S_t with split=True pairs only snapshots of the same half; an odd T drops the first snapshot."""
    rng = np.random.default_rng(5)
    x = rng.normal(size=(3, 9, 4, 5))
    S = ec.lag_sqdiff_reference(x, True, 3)
    exp = np.zeros((3, 4, 5))
    for c in range(3):
        for lo in (1, 5):
            for t in (1, 2, 3):
                for n in range(lo, lo + 4 - t):
                    exp[t - 1] += (x[c, n + t] - x[c, n]) ** 2
    np.testing.assert_allclose(S.astype(np.float64), exp, rtol=1e-14)


def test_summary_file_carries_lag_sqdiff(tmp_path):
    M, N, K = 6, 12, 5
    S, W, B, mean, sd = _planted_maps(K, M, N, 1)
    s = _summary(S, W, B, mean, sd, M, N)
    s.save(tmp_path / "with.npz")
    t = posterior.PosteriorSummary.load(tmp_path / "with.npz")
    assert t.lag_sqdiff.dtype == np.float64 and np.array_equal(t.lag_sqdiff, S)
    for a, b in zip(s.ess(), t.ess()):
        assert np.array_equal(a, b, equal_nan=True)
    assert np.array_equal(s.mcse(), t.mcse(), equal_nan=True) and np.array_equal(s.autocorrelation(), t.autocorrelation(), equal_nan=True)
    # a summary without the field still loads, and says what is missing
    s.lag_sqdiff = None
    s.save(tmp_path / "without.npz")
    old = posterior.PosteriorSummary.load(tmp_path / "without.npz")
    assert old.lag_sqdiff is None
    for fn in (old.ess, old.mcse, old.autocorrelation):
        with pytest.raises(ValueError, match="ess"):
            fn()


def test_library_exports_the_lagged_entry_point():
    assert "gsm_posterior_lagged" in _lib.declared_symbols()
    assert "posterior_lag_kernel.hip" in _lib.SOURCES
    assert hasattr(_lib.load(), "gsm_posterior_lagged")


def test_lag_split_plan_restates_the_part_rule():
    # 1024 chains of 256 x 256 on 256 compute units: 128 cell blocks of 2 fp64 cells per lane, 8 parts of 128 chains
    assert ec.lag_split_plan(256, 256, 1024, False, 256) == dict(vec=2, parts=8, cpp=128, last=128, empty=0)
    assert ec.lag_split_plan(256, 256, 1024, True, 256) == dict(vec=4, parts=16, cpp=64, last=64, empty=0)
    assert ec.lag_split_plan(127, 129, 101, True, 256) == dict(vec=1, parts=16, cpp=7, last=3, empty=1)
    assert ec.lag_split_plan(126, 129, 200, True, 256)["vec"] == 2


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, q):
    sys.path.insert(0, str(ROOT))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from mcmc_gpu_amd import parallel
    parallel.init_distributed("gloo")
    local = torch.as_tensor(np.random.default_rng(10 + rank).uniform(0.0, 1e6, size=(5, 6, 7)))
    local[2, 3, 4] = float("nan") if rank == 1 else 1.0
    keep = local.clone()
    total = parallel.all_reduce_sum(local)
    parallel.barrier()
    q.put((rank, total.numpy(), bool(np.array_equal(local.numpy(), keep.numpy(), equal_nan=True))))
    torch.distributed.destroy_process_group()


def test_lag_sums_add_over_two_ranks():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    outs = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    parts = [np.random.default_rng(10 + r).uniform(0.0, 1e6, size=(5, 6, 7)) for r in range(world)]
    parts[0][2, 3, 4], parts[1][2, 3, 4] = 1.0, np.nan
    exp = parts[0] + parts[1]
    for rank, total, untouched in outs:
        assert total.dtype == np.float64 and np.array_equal(total, exp, equal_nan=True) and np.isnan(total).sum() == 1
        assert untouched                                             # the rank's own sums are not overwritten
    # without a process group the sum of one rank is its own
    from mcmc_gpu_amd import parallel
    one = torch.as_tensor(parts[0])
    assert torch.equal(parallel.all_reduce_sum(one), one) and parallel.all_reduce_sum(one).data_ptr() != one.data_ptr()
