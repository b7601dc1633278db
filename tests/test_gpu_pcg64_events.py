"""-m gpu: the device PCG64 decoder (csrc/pcg64_device.h) at the rare stream events of tests/pcg64_event_cases.py, each case through
its kernel against NumPy in the reference's call order: every output bit for bit, all six words of every generator state, and the
output planes -- handed in filled with NaN -- untouched beyond what the call owns.  tests/test_pcg64_events_host.py shows that
each case reaches its event.  Cases that share a block table (a cell count) run as the chains (realisations) of one launch."""
import ctypes as C

import numpy as np
import pytest
import torch

import pcg64_event_cases as ec
from test_gpu_pcg64 import _host_draws

pytestmark = pytest.mark.gpu

GRID = 64                                        # the whole-grid draw kernel's grid
PAD = 64                                         # words behind the last realisation's path / draws
SENTINEL = -7


def _diff(fails, case, what, got, want):
    """Bitwise comparison; a difference is recorded with the case's name and the first differing index."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape:
        fails.append(f"{case.name}: {what}: shape {got.shape}, NumPy {want.shape}")
        return
    g = got.view(np.uint64) if got.dtype == np.float64 else got
    w = want.view(np.uint64) if want.dtype == np.float64 else want
    bad = np.flatnonzero(g.ravel() != w.ravel())
    if bad.size:
        fails.append(f"{case.name}: {what} differs first at index {bad[0]} ({bad.size} in all): device {got.ravel()[bad[0]]!r}, "
                     f"NumPy {want.ravel()[bad[0]]!r}")


def _state(fails, case, what, words, gen):
    got, want = tuple(int(x) for x in words), ec.pack(gen.bit_generator.state)
    names = ("state lo", "state hi", "inc lo", "inc hi", "has_uint32", "uinteger")
    for k in range(6):
        if got[k] != want[k]:
            fails.append(f"{case.name}: {what} generator: word {k} ({names[k]}) is {got[k]:#x}, NumPy {want[k]:#x}")
            return


def _untouched(fails, case, what, tail):
    bad = np.flatnonzero(~np.isnan(tail)) if tail.dtype == np.float64 else np.flatnonzero(tail != SENTINEL)
    if bad.size:
        fails.append(f"{case.name}: {what} written beyond its end, first at offset {bad[0]}")


# ---- one-wave Stream::normals: gsm_sgs_grid_draw_pcg64 ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sorted({c.shape for c in ec.CASES if c.harness == "grid"}))
def test_grid_cases_equal_numpy(n):
    from mcmc_gpu_amd import interpolate
    from mcmc_gpu_amd.engine import GsmEngine, _ptr
    cases = [c for c in ec.CASES if c.harness == "grid" and c.shape == n]
    R = len(cases)
    plan = interpolate._Plan.__new__(interpolate._Plan)                     # what _Plan.draws reads, without a fitted transformer
    plan.W, plan.cond, plan.bounds = GRID, np.zeros((GRID, GRID), dtype=bool), None
    plan.inds = np.stack([np.arange(n) // GRID, np.arange(n) % GRID], axis=1)
    eng = GsmEngine(GRID, GRID, R)
    try:
        dev = eng.dev
        states = torch.as_tensor(np.array([ec.words(c) for c in cases], dtype=np.uint64).view(np.int64)).to(dev)
        cells = torch.arange(n, dtype=torch.int32, device=dev)
        has_value = torch.zeros(GRID * GRID, dtype=torch.uint8, device=dev)
        work = torch.full((R, n), SENTINEL, dtype=torch.int32, device=dev)
        path = torch.full((R * n + PAD,), SENTINEL, dtype=torch.int32, device=dev)
        draws = torch.full((R * n + PAD,), float("nan"), dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            rc = eng.lib.gsm_sgs_grid_draw_pcg64(eng.h, _ptr(states), _ptr(cells), n, _ptr(has_value), None, None, 0, _ptr(work), _ptr(path),
                                                 _ptr(draws), n, eng._stream())
            torch.cuda.synchronize(dev)
        assert rc == 0, eng.lib.gsm_last_error(eng.h).decode()
        st, path, draws = states.cpu().numpy().view(np.uint64), path.cpu().numpy(), draws.cpu().numpy()
    finally:
        eng.close()
    fails = []
    for r, c in enumerate(cases):
        g = ec.generator(ec.words(c))
        p, d = plan.draws(g)
        _diff(fails, c, "path", path[r * n:(r + 1) * n], p)
        _diff(fails, c, "normals", draws[r * n:(r + 1) * n], d)
        _state(fails, c, "the", st[r], g)
    _untouched(fails, cases[-1], "draws", draws[R * n:])
    _untouched(fails, cases[-1], "path", path[R * n:])
    assert not fails, "\n".join(fails)


# ---- four-wave Stream::normals_mw<4>, bounded: gsm_draw_pcg64 -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain96():
    from mcmc_gpu_amd import synthetic
    prob, ch, _ = synthetic.template(96)
    return prob, ch


@pytest.mark.parametrize("shape", sorted({c.shape for c in ec.CASES if c.harness == "draw"}), ids=lambda s: "x".join(str(v) for v in s))
def test_draw_cases_equal_numpy(shape, chain96):
    from mcmc_gpu_amd import MCMC_gpu
    from mcmc_gpu_amd.engine import GsmEngine
    prob, ch = chain96
    H = 96
    cases = [c for c in ec.CASES if c.harness == "draw" and c.shape == shape]
    n = len(cases)
    rf = MCMC_gpu.RandField(10e3, 50e3, 12e3, 40e3, 50, 150, shape[5], "Matern", True, smoothness=0.9125)
    rf.set_block_sizes(*shape[:5])
    assert np.array_equal(rf.pairs, ec.pairs(shape))
    rf.set_weight_param(2, 0, 6, 1, 49900.0, prob["resolution"])
    rf.set_generation_method(True)
    of = lambda c, stream: ec.words(c) if c.params.get("stream", "rf") == stream else ec.OTHER_STATE
    eng = ch._make_engine(rf, n, 0)
    try:
        d_rf = torch.as_tensor(np.array([of(c, "rf") for c in cases], dtype=np.uint64).view(np.int64)).to(eng.dev)
        d_ch = torch.as_tensor(np.array([of(c, "ch") for c in cases], dtype=np.uint64).view(np.int64)).to(eng.dev)
        bufs = eng.alloc_pcg64_buffers(1, shape[5] > 0.0)
        for k in ("noise_re", "noise_im", "nugget"):
            if bufs[k] is not None:
                bufs[k].fill_(float("nan"))
        d = eng.draw_pcg64(1, rf, d_rf, d_ch, None, buffers=bufs)
        torch.cuda.synchronize()
        assert d["noise_re"] is bufs["noise_re"] and (d["nugget"] is None) == (shape[5] == 0.0)
        st_rf, st_ch = d_rf.cpu().numpy().view(np.uint64), d_ch.cpu().numpy().view(np.uint64)
        out = {k: (v.cpu().numpy() if v is not None else None) for k, v in d.items()}
    finally:
        eng.close()
    fails = []
    for c, case in enumerate(cases):
        assert all(case.params.get("H", H) == H for case in cases)
        g_rf, g_ch = ec.generator(of(case, "rf")), ec.generator(of(case, "ch"))
        h = _host_draws(rf, g_rf, g_ch, 1, H, H, None)
        B = h["re"][0].size
        _diff(fails, case, "size index", out["size_idx"][c], np.array(h["size_idx"], dtype=np.int32))
        _diff(fails, case, "centre", out["centre"][c], np.array(h["centre"], dtype=np.int32))
        _diff(fails, case, "u", out["u"][c], np.array(h["u"]))
        _diff(fails, case, "RandField scalars", out["rf_scalars"][c], np.array(h["sc"]))
        planes = [("real plane", out["noise_re"], h["re"]), ("imaginary plane", out["noise_im"], h["im"])]
        if out["nugget"] is not None:
            planes.append(("nugget plane", out["nugget"], h["ng"]))
        for what, got, want in planes:
            _diff(fails, case, what, got[c, 0, :B], want[0].ravel())
            _untouched(fails, case, what, got[c, 0, B:])
        _state(fails, case, "RandField", st_rf[c], g_rf)
        _state(fails, case, "chain", st_ch[c], g_ch)
    assert not fails, "\n".join(fails)


# ---- sgs_draw_pcg64_kernel: integers, interval, normals ---------------------------------------------------------------------------
def test_small_scale_cases_equal_numpy():
    from mcmc_gpu_amd.engine import GsmEngine, _ptr
    cases = [c for c in ec.CASES if c.harness == "small"]
    ch, is_data = ec.small_template()
    H, n = ec.SMALL_H, len(cases)
    assert all(c.shape == (H, ch.block_min_x, ch.block_max_x, ch.block_min_y, ch.block_max_y) for c in cases)
    max_cells = (ch.block_max_x - 1) * (ch.block_max_y - 1)
    eng = GsmEngine(H, H, n)
    try:
        dev = eng.dev
        d_gen = torch.as_tensor(np.array([ec.words(c) for c in cases], dtype=np.uint64).view(np.int64)).to(dev)
        i32 = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.int32, device=dev)
        d_win, d_blk, d_off, d_cnt, d_cells = i32(1, n, 4), i32(1, n, 4), i32(1, n), i32(1, n), i32(n * max_cells + PAD, 2)
        d_z = torch.full((n * max_cells + PAD,), float("nan"), dtype=torch.float64, device=dev)
        d_u = torch.full((1, n), float("nan"), dtype=torch.float64, device=dev)
        d_reg = torch.as_tensor(np.ascontiguousarray(ch.region_mask == 1, dtype=np.uint8)).to(dev)
        d_isd = torch.as_tensor(np.ascontiguousarray(is_data, dtype=np.uint8)).to(dev)
        eng._check(eng.lib.gsm_sgs_draw_pcg64(eng.h, _ptr(d_gen), 1, _ptr(d_reg), _ptr(d_isd), ch.block_min_x, ch.block_max_x, ch.block_min_y,
                                              ch.block_max_y, max_cells, _ptr(d_win), _ptr(d_blk), _ptr(d_off), _ptr(d_cnt), _ptr(d_cells),
                                              _ptr(d_z), _ptr(d_u), eng._stream()))
        eng._check(eng.lib.gsm_sgs_check(eng.h, eng._stream()))
        win, blk, cnt = d_win.cpu().numpy()[0], d_blk.cpu().numpy()[0], d_cnt.cpu().numpy()[0]
        cells, z, u = d_cells.cpu().numpy(), d_z.cpu().numpy(), d_u.cpu().numpy()[0]
        st = d_gen.cpu().numpy().view(np.uint64)
    finally:
        eng.close()
    fails = []
    for c, case in enumerate(cases):
        g = ec.generator(ec.words(case))
        b, w, inds, zz, uu = ch._draw_iteration(g, is_data)
        k = inds.shape[0]
        _diff(fails, case, "block", blk[c], np.array([int(v) for v in b], dtype=np.int32))
        _diff(fails, case, "window", win[c], np.array(w, dtype=np.int32))
        _diff(fails, case, "cell count", cnt[c], np.int32(k))
        _diff(fails, case, "cells", cells[c * max_cells:c * max_cells + k], inds)
        _diff(fails, case, "normals", z[c * max_cells:c * max_cells + k], zz)
        _diff(fails, case, "u", u[c], np.float64(uu))
        _untouched(fails, case, "normals", z[c * max_cells + k:(c + 1) * max_cells])
        _untouched(fails, case, "cells", cells[c * max_cells + k:(c + 1) * max_cells].ravel())
        _state(fails, case, "the", st[c], g)
    _untouched(fails, cases[-1], "normals", z[n * max_cells:])
    _untouched(fails, cases[-1], "cells", cells[n * max_cells:].ravel())
    assert not fails, "\n".join(fails)


# ---- flag 128 of pcg64_draw_kernel ------------------------------------------------------------------------------------------------
def test_no_centre_inside_the_region_mask_is_a_device_data_error():
    """An all-zero region mask: the chain generator gives up after 2^20 + 2 centres (its draws are NumPy's all the same), the step's
    RandField outputs equal NumPy's, and the next gsm_run_replay reports GSM_E_DEVICE_DATA."""
    from mcmc_gpu_amd import synthetic
    from mcmc_gpu_amd._lib import GsmError
    H = 64
    prob, ch, rf = synthetic.template(H)
    eng = ch._make_engine(rf, 1, 0)
    try:
        eng.set_state(prob["bed"][None].copy())
        g_rf, g_ch = np.random.default_rng(5), np.random.default_rng(6)
        d_rf, d_ch = eng.pcg64_to_device([np.random.default_rng(5)]), eng.pcg64_to_device([np.random.default_rng(6)])
        d_reg = torch.zeros((H, H), dtype=torch.uint8, device=eng.dev)
        d = eng.draw_pcg64(1, rf, d_rf, d_ch, d_reg)
        torch.cuda.synchronize()
        h = _host_draws(rf, g_rf, np.random.default_rng(0), 1, H, H, None)       # the RandField generator's part of the step
        B = h["re"][0].size
        assert int(d["size_idx"][0, 0]) == h["size_idx"][0]
        assert np.array_equal(d["rf_scalars"][0].cpu().numpy(), np.array(h["sc"]))
        assert np.array_equal(d["noise_re"][0, 0, :B].cpu().numpy(), h["re"][0].ravel())
        assert np.array_equal(d["noise_im"][0, 0, :B].cpu().numpy(), h["im"][0].ravel())
        assert eng.pcg64_from_device(d_rf)[0] == g_rf.bit_generator.state
        tries = g_ch.integers(low=0, high=H, size=2 * ((1 << 20) + 2))           # 32-bit words through the generator's own cache
        assert tuple(d["centre"][0, 0].cpu().numpy()) == (int(tries[-2]), int(tries[-1]))
        assert float(d["u"][0, 0]) == g_ch.random()
        assert eng.pcg64_from_device(d_ch)[0] == g_ch.bit_generator.state
        fields = torch.zeros((1, 1, eng.field_stride), dtype=torch.float64, device=eng.dev)
        loss = torch.empty((1, 1), dtype=torch.float64, device=eng.dev)
        acc = torch.empty((1, 1), dtype=torch.uint8, device=eng.dev)
        with pytest.raises(GsmError) as ei:
            eng.call(eng.lib.gsm_run_replay, 1, eng.beds, eng.energy, eng.resampled, eng.loss_sum, d["size_idx"], d["centre"], d["u"], fields,
                     eng.field_stride, loss, acc)
        assert ei.value.code == -5 and "gsm_run_replay" in str(ei.value)           # GSM_E_DEVICE_DATA
        eng.call(eng.lib.gsm_run_replay, 1, eng.beds, eng.energy, eng.resampled, eng.loss_sum, d["size_idx"], d["centre"], d["u"], fields,
                 eng.field_stride, loss, acc)                                      # the flag was cleared: the same call passes
    finally:
        eng.close()
