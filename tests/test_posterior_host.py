"""CPU suite of the posterior accumulator: the snapshot schedule, the finalisation of partials (one group of chains and ragged
groups whose partials add), the cross-rank merge over gloo, the new symbols of the library and the summary file, and the kernels'
summation order at the chain counts of tests/test_gpu_posterior_many_chains.py against the tolerances."""
import os
import socket
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import posterior_common as pc
from mcmc_gpu_amd import _lib, posterior

ROOT = Path(__file__).resolve().parent.parent


def test_snapshot_iterations_hand_written_cases():
    assert posterior.snapshot_iterations(10, 0, 3).tolist() == [0, 3, 6, 9]          # burn-in 0 includes the initial bed
    assert posterior.snapshot_iterations(10, 2, 3).tolist() == [2, 5, 8]             # thin does not divide n_iter
    assert posterior.snapshot_iterations(61, 11, 5).tolist() == list(range(11, 61, 5))
    assert posterior.snapshot_iterations(11, 10, 1).tolist() == [10]                 # n_iter - 1 is the last iteration
    assert posterior.snapshot_iterations(5, 7, 1).tolist() == []
    with pytest.raises(ValueError):
        posterior.snapshot_iterations(10, -1, 1)
    with pytest.raises(ValueError):
        posterior.snapshot_iterations(10, 0, 0)
    its, N, dropped = posterior.sequence_plan(61, 0, 7, split=True)                  # T = 9: odd, the first is dropped
    assert (its.size, N, dropped) == (9, 4, 1)
    its, N, dropped = posterior.sequence_plan(61, 11, 5, split=True)
    assert (its.size, N, dropped) == (10, 5, 0)
    assert posterior.sequence_plan(61, 0, 7, split=False)[1:] == (9, 0)
    posterior.sequence_plan(10, 0, 9, split=False)                                   # T = 2
    with pytest.raises(ValueError):
        posterior.sequence_plan(10, 0, 10, split=False)                              # T = 1 < 2
    with pytest.raises(ValueError):
        posterior.sequence_plan(10, 0, 4, split=True)                                # T = 3 < 4
    posterior.sequence_plan(10, 0, 3, split=True)                                    # T = 4
    with pytest.raises(ValueError):
        posterior.check_options(dict(burn_in=0, thin=1, bogus=1), 10)
    with pytest.raises(ValueError):
        posterior.check_options(dict(burn_in=8, thin=1), 10)


def _data(C, T, H, W, seed):
    g = np.random.default_rng(seed)
    x = -300.0 + 100.0 * g.normal(size=(C, T, H, W))
    x[:, :, 2:4, 1:5] = x[:, :1, 2:4, 1:5]            # constant within every chain: W == 0, rhat NaN
    x[1, T - 2, 0, 3] = np.nan
    return x, -300.0 + 10.0 * g.normal(size=(H, W))


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("T", [9, 10])
def test_finalize_of_numpy_partials_equals_the_reference(split, T):
    x, g = _data(5, T, 7, 6, 3)
    ref = pc.posterior_reference(x, split)
    s = posterior.finalize(pc.numpy_partials(x, split, g), ref["M"], ref["N"], g, rhat=True, n_chains=5,
                           snapshot_iterations=np.arange(T), burn_in=0, thin=1, split=split)
    pc.check_maps(s, ref, label=f"host split={split} T={T}")
    assert np.isnan(s.rhat[2:4, 1:5]).all() and (s.within_var[2:4, 1:5] == 0).all()
    assert np.isnan(s.mean[0, 3]) and np.isnan(s.sd[0, 3]) and np.isnan(s.rhat[0, 3])
    assert np.isfinite(s.rhat).sum() == 7 * 6 - 8 - 1
    p = posterior.finalize(pc.numpy_pooled_partials(x, split, g), ref["M"], ref["N"], g, rhat=False, n_chains=5,
                           snapshot_iterations=np.arange(T), burn_in=0, thin=1, split=split)
    assert p.rhat is None and p.within_var is None
    pc.check_maps(p, ref, rhat=False, label=f"host pooled split={split} T={T}")


@pytest.mark.parametrize("groups", [(4, 3), (1, 4, 2)])
def test_partials_of_ragged_groups_add(groups):
    C = sum(groups)
    x, g = _data(C, 10, 6, 5, 11)
    x[1, 8, 0, 3] = x[1, 7, 0, 3]                      # no NaN here: compare every cell
    kw = dict(n_chains=C, snapshot_iterations=np.arange(10), burn_in=0, thin=1, split=True)
    one = posterior.finalize(pc.numpy_partials(x, True, g), 2 * C, 5, g, **kw)
    lo, tot = 0, 0.0
    for n in groups:
        tot = tot + pc.numpy_partials(x[lo:lo + n], True, g)
        lo += n
    many = posterior.finalize(tot, 2 * C, 5, g, **kw)
    for name in ("mean", "sd", "within_var", "between_var_over_n", "rhat"):
        np.testing.assert_allclose(getattr(many, name), getattr(one, name), rtol=1e-12, atol=0, equal_nan=True, err_msg=name)


def test_split_plan_hand_computed_cases():
    """The split rule on 256 compute units, worked by hand from the comments of posterior_kernel.hip."""
    pl = pc.split_plan(128, 128, 390, True, 256)            # 4096 lanes of 4 cells = 16 cell blocks; 1024 / 16 = 64 parts
    assert pl["pooled"] == dict(vec=4, parts=64, cpp=7, last=5, empty=8)
    assert pl["partials"] == dict(vec=1, parts=16, cpp=25, last=15, empty=0)
    assert pl["accumulate"] == dict(V=4, grid=2048, trips=2, last_trip_blocks=1072, last_block_groups=512, tail=0)   # 3120 blocks wanted
    pl = pc.split_plan(127, 129, 101, False, 256)           # odd plane: one cell per lane in both forms
    assert pl["pooled"] == pl["partials"] == dict(vec=1, parts=16, cpp=7, last=3, empty=1)
    assert pl["accumulate"]["tail"] == 1 and pc.split_plan(127, 129, 101, True, 256)["accumulate"]["tail"] == 3
    pl = pc.split_plan(64, 64, 5, False, 256)               # what the few-chain tests run: one chain per part
    assert pl["pooled"] == dict(vec=2, parts=5, cpp=1, last=1, empty=0) and pl["accumulate"]["trips"] == 1
    pl = pc.split_plan(256, 256, 1024, False, 256)          # production
    assert (pl["pooled"]["parts"], pl["pooled"]["cpp"], pl["accumulate"]["trips"]) == (8, 128, 32)


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("T", [4, 5])
@pytest.mark.parametrize("C,grid", [(390, (128, 128)), (101, (127, 129))])
def test_kernel_summation_order_stays_within_the_tolerances(C, grid, T, split):
    """The kernels' order of summation (pc.emulate_partials) with the parts and chains per part that an MI355X gives C chains
    on `grid`, on 22 x 20 cells drawn as the GPU tests draw them: the reference and the order alone stay inside the tolerances."""
    H, W = 22, 20
    x, g = pc.many_chain_data(C, T, H, W, C + T)
    plan = pc.split_plan(*grid, C, True, 256)
    assert (plan["pooled"]["parts"], plan["pooled"]["cpp"]) == {390: (64, 7), 101: (16, 7)}[C]
    assert (plan["partials"]["parts"], plan["partials"]["cpp"]) == {390: (16, 25), 101: (16, 7)}[C]
    ref = pc.posterior_reference(x, split)
    const = pc.constant_cells(H, W, split)
    kw = dict(n_chains=C, snapshot_iterations=np.arange(T), burn_in=0, thin=1, split=split)
    for rhat in (True, False):
        form = plan["partials" if rhat else "pooled"]
        P = pc.emulate_partials(x, g, split, rhat, form["parts"], form["cpp"])
        s = posterior.finalize(P, ref["M"], ref["N"], g, rhat=rhat, **kw)
        pc.check_maps(s, ref, rhat=rhat, label=f"emulated C={C} T={T} split={split} rhat={rhat}")
        assert np.isnan(s.mean[5, 7]) and np.isnan(s.mean).sum() == 1
        if rhat:
            assert (s.within_var[const] == 0).all() and np.isnan(s.rhat[const]).all()
            assert np.isfinite(s.rhat[~const]).sum() == H * W - const.sum() - 1


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, n_chains, q):
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import posterior_common as pc_
    from mcmc_gpu_amd import parallel
    parallel.init_distributed("gloo")
    lo, hi = parallel.shard_bounds(n_chains, world, rank)
    x, g = _data(n_chains, 10, 6, 5, 11)
    tot, M = parallel.all_reduce_posterior(torch.as_tensor(pc_.numpy_partials(x[lo:hi], True, g)), 2 * (hi - lo))
    parallel.barrier()
    q.put((rank, tot.numpy(), M))
    torch.distributed.destroy_process_group()


def test_all_reduce_posterior_world2_ragged():
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
    x, g = _data(n_chains, 10, 6, 5, 11)
    exp = pc.numpy_partials(x[:4], True, g) + pc.numpy_partials(x[4:], True, g)
    ref = pc.posterior_reference(x, True)
    for rank, tot, M in outs:
        assert M == 14
        assert np.array_equal(tot, exp, equal_nan=True)
        s = posterior.finalize(tot, M, 5, g, n_chains=7, snapshot_iterations=np.arange(10), burn_in=0, thin=1, split=True)
        pc.check_maps(s, ref, label=f"gloo rank {rank}")


def test_library_exports_the_posterior_entry_points():
    names = {"gsm_posterior_accumulate", "gsm_posterior_accumulate_pooled", "gsm_posterior_sample", "gsm_posterior_close",
             "gsm_posterior_partials"}
    assert names <= set(_lib.declared_symbols())
    assert "posterior_kernel.hip" in _lib.SOURCES
    lib = _lib.load()
    for n in names:
        assert hasattr(lib, n), n


def test_summary_save_load_round_trip(tmp_path):
    x, g = _data(4, 9, 6, 5, 2)
    its = posterior.snapshot_iterations(61, 0, 7)
    for rhat in (True, False):
        part = pc.numpy_partials(x, True, g) if rhat else pc.numpy_pooled_partials(x, True, g)
        s = posterior.finalize(part, 8, 4, g, rhat=rhat, n_chains=4, snapshot_iterations=its, burn_in=0, thin=7, split=True,
                               sample_values=x[:, :, 1, :3].transpose(0, 2, 1).copy() if rhat else None,
                               sample_loc=np.arange(6.0).reshape(3, 2) if rhat else None)
        f = tmp_path / f"posterior_{int(rhat)}.npz"
        s.save(f)
        t = posterior.PosteriorSummary.load(f)
        for name in ("mean", "sd", "rhat", "within_var", "between_var_over_n", "snapshot_iterations", "sample_values", "sample_loc"):
            a, b = getattr(s, name), getattr(t, name)
            assert (a is None and b is None) or np.array_equal(a, b, equal_nan=True), name
        assert (t.n_chains, t.n_sequences, t.n_per_sequence, t.burn_in, t.thin, t.split) == (4, 8, 4, 0, 7, True)
