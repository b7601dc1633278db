"""GPU: the 'pcg64' mode of interpolate.sgs -- gsm_sgs_grid_draw_pcg64 (csrc/sgs_grid_draw_kernel.hip) makes the shuffle, the
path and the draws of every realisation on the device from the callers' own NumPy generators.  The mode has a parity contract,
so every check is an equality: the entry against interpolate._Plan.draws (NumPy) on the cases of
tests/interp_sgs_pcg64_common.py, and sgs / sgs_many / _run with mode='pcg64' against the same calls in the default mode."""
import warnings

import numpy as np
import pytest

import interp_sgs_common as ic
import interp_sgs_pcg64_common as pc
import nonstationary_common as nc

pytestmark = pytest.mark.gpu

SENTINEL = -7


def _entry(plan, gens, kind, path_len=None, H=pc.H, W=pc.W, null=(), n_cells=None):
    """One gsm_sgs_grid_draw_pcg64 call on buffers filled with SENTINEL.  Returns (return code, error text, path [R, path_len],
    draws [R, path_len], states [R, 6] uint64, work [R, n_cells]); `null`: names of pointers passed as NULL."""
    import torch
    from mcmc_gpu_amd.engine import GsmEngine, _ptr
    R = len(gens)
    flat = np.ascontiguousarray(plan.inds[:, 0] * plan.W + plan.inds[:, 1], dtype=np.int32)
    if path_len is None:
        path_len = int(np.count_nonzero(~plan.cond.ravel()[flat]))
    eng = GsmEngine(H, W, R)
    try:
        dev = eng.dev
        t = dict(states=torch.as_tensor(GsmEngine.pack_pcg64_states(gens).view(np.int64)).to(dev),
                 cells=torch.as_tensor(flat if flat.size else np.zeros(1, np.int32)).to(dev),
                 has_value=torch.as_tensor(plan.cond.astype(np.uint8).ravel()).to(dev),
                 lower=None, upper=None,
                 work=torch.full((R, max(1, flat.size)), SENTINEL, dtype=torch.int32, device=dev),
                 path=torch.full((R, max(1, abs(path_len))), SENTINEL, dtype=torch.int32, device=dev),
                 draws=torch.full((R, max(1, abs(path_len))), float(SENTINEL), dtype=torch.float64, device=dev))
        if plan.bounds is not None:
            t["lower"], t["upper"] = (torch.as_tensor(b).to(dev) for b in plan.bounds)
        p = {k: _ptr(None if k in null else v) for k, v in t.items()}
        with torch.cuda.device(dev):
            rc = eng.lib.gsm_sgs_grid_draw_pcg64(eng.h, p["states"], p["cells"], flat.size if n_cells is None else n_cells, p["has_value"],
                                                 p["lower"], p["upper"], kind, p["work"], p["path"], p["draws"], path_len, eng._stream())
            torch.cuda.synchronize(dev)
        text = eng.lib.gsm_last_error(eng.h).decode() if rc else ""
        return (rc, text, t["path"].cpu().numpy(), t["draws"].cpu().numpy(), t["states"].cpu().numpy().view(np.uint64),
                t["work"].cpu().numpy())
    finally:
        eng.close()


@pytest.mark.parametrize("cid", list(pc.cases()))
def test_draw_entry_equals_numpy(cid):
    """path as integers, draws on their uint64 views, the final states field by field."""
    from mcmc_gpu_amd.engine import GsmEngine
    n, values, kind, R, pending = pc.cases()[cid]
    plan = pc.plan(n, values, kind)
    ref_gens = pc.generators(R, pending)
    ref = [plan.draws(g) for g in ref_gens]
    rc, text, path, draws, states, work = _entry(plan, pc.generators(R, pending), 1 if kind == "truncated" else 0)
    assert rc == 0, text
    L = ref[0][0].size
    assert all(p.size == L for p, _ in ref)
    flat = plan.inds[:, 0] * plan.W + plan.inds[:, 1]
    for r, (p, d) in enumerate(ref):
        assert np.array_equal(path[r, :L], p), f"path of realisation {r}"
        assert np.array_equal(draws[r, :L].view(np.uint64), d.view(np.uint64)), f"draws of realisation {r}"
        if n:
            assert np.array_equal(np.sort(work[r]), np.sort(flat)), f"work of realisation {r} is no permutation of the cells"
    for r, st in enumerate(GsmEngine.unpack_pcg64_states(states)):
        want = ref_gens[r].bit_generator.state
        assert st["state"] == want["state"] and st["has_uint32"] == want["has_uint32"] and st["uinteger"] == want["uinteger"], r
    if cid == pc.MANY_NORMALS:
        assert R * L >= 50_000 and (np.abs(draws[:, :L]) > pc.ZIGGURAT_NOR_R).any()          # tails came through the device
    if kind == "truncated" and L:
        lo, hi = plan.bounds[0].ravel()[path[0, :L]], plan.bounds[1].ravel()[path[0, :L]]
        assert np.all(draws[0, :L][lo == hi] == 0.0)
        if L > 40:
            assert (lo == hi).any() and (np.isnan(lo) | np.isnan(hi)).any()


@pytest.mark.parametrize("delta", [-1, 1])
def test_wrong_path_length_is_a_device_data_error(delta):
    from mcmc_gpu_amd.engine import GsmEngine
    plan = pc.plan(129, "some", "normal")
    flat = plan.inds[:, 0] * plan.W + plan.inds[:, 1]
    L = int(np.count_nonzero(~plan.cond.ravel()[flat]))
    rc, text, path, draws, states, _ = _entry(plan, pc.generators(3, False), 0, path_len=L + delta)
    assert rc == -5 and "path length" in text
    assert np.all(draws == float(SENTINEL))                                      # no draw was made


def test_argument_errors_return_e_arg_and_write_nothing():
    plan_n, plan_t = pc.plan(129, "some", "normal"), pc.plan(129, "some", "truncated")
    flat = plan_n.inds[:, 0] * plan_n.W + plan_n.inds[:, 1]
    L = int(np.count_nonzero(~plan_n.cond.ravel()[flat]))
    bad = [dict(plan=plan_n, kind=0, null=("states",)), dict(plan=plan_n, kind=0, null=("cells",)),
           dict(plan=plan_n, kind=0, null=("has_value",)), dict(plan=plan_n, kind=0, null=("work",)),
           dict(plan=plan_n, kind=0, null=("path",)), dict(plan=plan_n, kind=0, null=("draws",)),
           dict(plan=plan_n, kind=0, n_cells=-1), dict(plan=plan_n, kind=0, n_cells=pc.H * pc.W + 1),
           dict(plan=plan_n, kind=0, path_len=-1), dict(plan=plan_n, kind=0, path_len=130),
           dict(plan=plan_t, kind=1, null=("lower",)), dict(plan=plan_t, kind=1, null=("upper",)),
           dict(plan=plan_n, kind=1),                                            # truncated without bounds
           dict(plan=plan_n, kind=2), dict(plan=plan_n, kind=-1)]
    for kw in bad:
        gens = pc.generators(2, True)
        before = np.array([[int(g.bit_generator.state["state"]["state"]) & (2 ** 64 - 1)] for g in gens], dtype=np.uint64)
        p = kw.pop("plan")
        kind = kw.pop("kind")
        rc, text, path, draws, states, work = _entry(p, gens, kind, **kw)
        assert rc == -1 and text, kw
        assert np.all(path == SENTINEL) and np.all(draws == float(SENTINEL)) and np.all(work == SENTINEL), kw
        assert np.array_equal(states[:, :1], before), kw
    assert L == 92


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def _cases():
    xx, yy, grid, cases = ic.small()
    out = [(f"small-{t}", xx, yy, grid, *cases[t][:2]) for t in ("a", "b", "c")]
    xx, yy, grid, cases = nc.small()
    return out + [("nonstationary-a", xx, yy, grid, *cases["a"][:2])]


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c[0])
def test_pcg64_mode_equals_replay_end_to_end(case):
    from mcmc_gpu_amd import interpolate
    _, xx, yy, grid, vario, kw = case
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        g_dev, g_host = np.random.default_rng(99), np.random.default_rng(99)
        g_dev.integers(0, 10), g_host.integers(0, 10)                           # the generators enter with a cached word
        dev = interpolate.sgs_many(xx, yy, grid, vario, [21, g_dev, 5], mode="pcg64", **kw)
        host = interpolate.sgs_many(xx, yy, grid, vario, [21, g_host, 5], **kw)
        assert dev.shape == host.shape == (3,) + grid.shape
        assert np.array_equal(dev, host, equal_nan=True)
        assert g_dev.bit_generator.state == g_host.bit_generator.state
        assert np.array_equal(interpolate.sgs_many(xx, yy, grid, vario, [21, 5], mode="replay", **kw), host[[0, 2]], equal_nan=True)
        one = interpolate.sgs(xx, yy, grid, vario, seed=7, mode="pcg64", **kw)
        assert np.array_equal(one, interpolate.sgs(xx, yy, grid, vario, seed=7, **kw), equal_nan=True)
        assert not np.array_equal(one, dev[0], equal_nan=True)
        plan = interpolate._Plan(xx, yy, grid, vario, kw["radius"], kw["num_points"], kw["ktype"], kw.get("sim_mask"), None, None,
                                 kw.get("bounds"))
        t_dev, t_host = [np.random.default_rng(s) for s in (31, 32)], [np.random.default_rng(s) for s in (31, 32)]
        ns_d, (paths_d, tr_d) = interpolate._run(plan, t_dev, trace=True, mode="pcg64")
        ns_h, (paths_h, tr_h) = interpolate._run(plan, t_host, trace=True)
    assert len(paths_d) == len(paths_h) == 2
    for a, b in zip(paths_d, paths_h):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert np.array_equal(tr_d, tr_h, equal_nan=True) and np.array_equal(ns_d, ns_h, equal_nan=True)
    assert [g.bit_generator.state for g in t_dev] == [g.bit_generator.state for g in t_host]


def test_generator_with_a_cached_word_after_the_shuffle_ends_where_numpy_leaves_it():
    """The 30 x 30 problem of the host test: the shuffle leaves has_uint32 == 1, the uniforms behind it must leave it alone."""
    from mcmc_gpu_amd import interpolate
    xx, yy, grid, vario, kw = pc.small_30()
    g_dev, g_host = np.random.default_rng(pc.SEED_30), np.random.default_rng(pc.SEED_30)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        dev = interpolate.sgs(xx, yy, grid, vario, seed=g_dev, mode="pcg64", **kw)
        host = interpolate.sgs(xx, yy, grid, vario, seed=g_host, **kw)
    assert np.array_equal(dev, host) and not np.isnan(dev).any()
    assert g_dev.bit_generator.state == g_host.bit_generator.state and g_dev.bit_generator.state["has_uint32"] == 1
