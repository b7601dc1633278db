"""GPU: gsm_gaussian_filter (csrc/trend_kernel.hip) through the C ABI against the long-double restatement and the bar of
tests/trend_common.py (derived from the number format and the length of the sums, shown fair for scipy by tests/test_trend_host.py).

Per case, a batch of 3 distinct fields: every field within B of the restatement and within 2 B of scipy; each field of the batch equal
to the one-field call bit for bit; one NaN cell gives exactly scipy's set of NaN cells.  The refusals return GSM_E_ARG."""
import ctypes as C

import numpy as np
import pytest
from scipy.ndimage import gaussian_filter

import trend_common as tc

pytestmark = pytest.mark.gpu
GSM_E_ARG = -1


def _weights(sigma):
    from mcmc_gpu_amd.sgs import gaussian_weights
    s0, s1 = tc.sigmas(sigma)
    return gaussian_weights(s0), gaussian_weights(s1)


def _engine(H, W):
    from mcmc_gpu_amd.engine import GsmEngine
    return GsmEngine(H, W, 1)


def _raw(eng, x_ptr, out_ptr, n, H, W, w0, w1, lw0=None, lw1=None):
    """The return code of gsm_gaussian_filter on raw pointers."""
    import torch
    dp = C.POINTER(C.c_double)
    p0 = w0.ctypes.data_as(dp) if w0 is not None else dp()
    p1 = w1.ctypes.data_as(dp) if w1 is not None else dp()
    with torch.cuda.device(eng.dev):
        return eng.lib.gsm_gaussian_filter(eng.h, x_ptr, out_ptr, n, H, W, p0, (w0.size // 2) if lw0 is None else lw0,
                                           p1, (w1.size // 2) if lw1 is None else lw1, eng._stream())


@pytest.mark.parametrize("case", tc.GPU_CASES, ids=tc.case_id)
def test_filter_within_bar_and_batch_rows_equal_single_calls(case):
    import torch
    H, W, sigma = case
    x = tc.fields(H, W)
    w0, w1 = _weights(sigma)
    eng = _engine(H, W)
    try:
        got = eng.gaussian_filter(x, w0, w1)
        singles = [eng.gaussian_filter(x[r:r + 1], w0, w1) for r in range(x.shape[0])]
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        for r in range(x.shape[0]):
            ratio = tc.worst_ratio(got[r], x[r], sigma)
            sc = gaussian_filter(x[r], sigma=sigma)
            to_scipy = float(np.max(np.abs(got[r] - sc) / tc.bar(x[r], sigma)))
            print(f"{tc.case_id(case)} field {r}: device error = {ratio:.3f} B, device - scipy = {to_scipy:.3f} B")
            assert ratio <= 1.0
            assert to_scipy <= 2.0
            np.testing.assert_array_equal(singles[r].cpu().numpy()[0], got[r])
    finally:
        eng.close()


@pytest.mark.parametrize("case", [(96, 130, 10), (13, 37, 10), (45, 70, (3, 10))], ids=tc.case_id)
def test_one_nan_cell_gives_scipys_nan_cells(case):
    H, W, sigma = case
    x = tc.fields(H, W)
    x[1, H // 3, W // 2] = np.nan
    w0, w1 = _weights(sigma)
    eng = _engine(H, W)
    try:
        got = eng.gaussian_filter(x, w0, w1).cpu().numpy()
    finally:
        eng.close()
    for r in range(3):
        np.testing.assert_array_equal(np.isnan(got[r]), np.isnan(gaussian_filter(x[r], sigma=sigma)))
    assert np.isnan(got[1]).any() and not np.isnan(got[0]).any() and not np.isnan(got[2]).any()
    if case[0] == 96:
        assert not np.isnan(got[1]).all()            # wider than the reach of a NaN: some cells stay finite


def test_trend_of_runs_on_the_device():
    from mcmc_gpu_amd import sgs
    x = tc.fields(33, 100)
    t = sgs.trend_of(x, sigma=3)                     # device=None with a GPU: the kernels
    assert t.shape == x.shape and t.dtype == np.float64
    for r in range(3):
        assert tc.worst_ratio(t[r], x[r], 3) <= 1.0
    one = sgs.trend_of(x[2], sigma=3, device=True)
    np.testing.assert_array_equal(one, t[2])


def test_refusals():
    import torch
    H, W = 12, 20
    eng = _engine(H, W)
    try:
        x = torch.zeros((2, H, W), dtype=torch.float64, device=eng.dev)
        out = torch.full_like(x, 7.0)
        vp = lambda t: C.c_void_p(t.data_ptr())
        w0, w1 = _weights(3)
        null = C.c_void_p(0)
        big = np.full(2 * 129 + 1, 1.0 / 259)
        bad = [
            _raw(eng, null, vp(out), 2, H, W, w0, w1),
            _raw(eng, vp(x), null, 2, H, W, w0, w1),
            _raw(eng, vp(x), vp(out), 2, H, W, None, w1, lw0=3),
            _raw(eng, vp(x), vp(out), 2, H, W, w0, None, lw1=3),
            _raw(eng, vp(x), vp(x), 2, H, W, w0, w1),                     # aliasing
            _raw(eng, vp(x), vp(out), 0, H, W, w0, w1),
            _raw(eng, vp(x), vp(out), -1, H, W, w0, w1),
            _raw(eng, vp(x), vp(out), 2, H, W, big, w1),                  # lw = 129: above the cap of 128
            _raw(eng, vp(x), vp(out), 2, H, W, w0, big),
            _raw(eng, vp(x), vp(out), 2, H, W, w0, w1, lw0=-1),
            _raw(eng, vp(x), vp(out), 2, H + 1, W, w0, w1),               # not the handle's grid
            _raw(eng, vp(x), vp(out), 2, W, H, w0, w1),
        ]
        assert bad == [GSM_E_ARG] * len(bad)
        assert b"gsm_gaussian_filter" in eng.lib.gsm_last_error(eng.h)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())                                   # nothing was launched
        cap = np.full(2 * 128 + 1, 1.0 / 257)                             # the cap itself is taken
        assert _raw(eng, vp(x), vp(out), 2, H, W, cap, cap) == 0
        torch.cuda.synchronize()
        assert bool((out == 0.0).all())
    finally:
        eng.close()
    # a handle of a grid with a side below 3 cells serves the filter alone
    small = _engine(2, 3)
    try:
        with torch.cuda.device(small.dev):
            assert small.lib.gsm_sgs_check(small.h, small._stream()) == GSM_E_ARG
            assert b"side below 3" in small.lib.gsm_last_error(small.h)
            assert small.lib.gsm_enable_timing(small.h, 1) == GSM_E_ARG
    finally:
        small.close()
