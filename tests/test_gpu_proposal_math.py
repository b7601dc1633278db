"""-m gpu: the scalar arithmetic of the Philox proposal path as the device computes it (gsm_debug_proposal_math: the device compile of
csrc/proposal_device.h, csrc/math_tables.h and csrc/philox.h, the math table read from LDS) against mpmath at the constructed arguments and
the bars of tests/proposal_math_common.py -- which tests/test_proposal_math_host.py shows to be fair on a g++ restatement and which are not
tuned to the device.  Each test prints the largest |error| / bar it met (DESIGN.md records them)."""
import ctypes as C

import numpy as np
import pytest

import philox_oracle as po
import proposal_math_common as pm

pytestmark = pytest.mark.gpu
PER = {pm.PHILOX: 4, pm.LOG_TAB: 1, pm.SINCOS_TAB: 2, pm.SQRT_LEAN: 1, pm.EXP_LEAN: 1, pm.NORMALS4_WORDS: 4, pm.NORMALS2_WORDS: 2,
       pm.SPECTRAL_AMP: 1}      # values per element of the output


def _dev(which, *xs, model=0, nu=0.0):
    """Output of one gsm_debug_proposal_math launch on the arrays xs (float64, or uint32 words for the selectors that take them)."""
    import torch
    from mcmc_gpu_amd import _lib
    lib = _lib.load()
    words = which in (pm.PHILOX, pm.NORMALS4_WORDS, pm.NORMALS2_WORDS)
    # torch has no uint32 arithmetic, and needs none: the words travel as the bytes of an int32 tensor
    d = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint32).view(np.int32) if words else np.ascontiguousarray(x, dtype=np.float64)).to("cuda:0")
         for x in xs]
    n = xs[0].shape[0]
    if which == pm.PHILOX:
        out = torch.full((n, 4), -1, dtype=torch.int32, device="cuda:0")
    else:
        out = torch.full((n * PER[which],), 12345.0, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    ptr = [C.c_void_p(t.data_ptr()) for t in d] + [None] * (4 - len(d))
    rc = lib.gsm_debug_proposal_math(which, model, nu, n, *ptr, C.c_void_p(out.data_ptr()), None)
    assert rc == 0, rc
    o = out.cpu().numpy()
    return o.view(np.uint32) if which == pm.PHILOX else o


def _worst(name, r):
    w = float(np.max(r))
    print(f"{name}: largest |error| / bar = {w:.3f} over {r.size} values")
    return w


def test_philox_draw_bit_for_bit():
    rows, exp = pm.philox_points()
    assert np.array_equal(_dev(pm.PHILOX, rows), exp)


def test_log_tab_meets_its_bar():
    x = pm.log_points()
    got = _dev(pm.LOG_TAB, x)
    assert _worst("log_tab", pm.log_ratio(got)) <= 1.0
    assert np.all(got[x == 1.0] == 0.0)


def test_sincos_tab_meets_its_bar():
    assert _worst("sincos_tab", pm.sincos_ratio(_dev(pm.SINCOS_TAB, pm.sincos_points()))) <= 1.0


def test_sqrt_lean_meets_its_bar():
    assert _worst("sqrt_lean", pm.sqrt_ratio(_dev(pm.SQRT_LEAN, pm.sqrt_points()))) <= 1.0


def test_exp_lean_meets_its_bar():
    assert _worst("exp_lean", pm.exp_ratio(_dev(pm.EXP_LEAN, pm.exp_points()))) <= 1.0


@pytest.mark.parametrize("layout", [4, 2])
def test_normals_on_words_meet_their_bar(layout):
    """normals4 (layout 4: the coefficient phase) and normals2 (layout 2: nugget pass, Cholesky generator) on constructed Philox words.
    With the rounded log c_0 in the table (math_tables.h before it was set so that log_tab(1) = 0) the u == 1 points of both layouts failed
    here with |g| up to 4.928096e-9, and no other point did (u < 1: 0.257 and 0.364 of the bar, as now)."""
    got = _dev(pm.NORMALS4_WORDS if layout == 4 else pm.NORMALS2_WORDS, pm.normals4_points() if layout == 4 else pm.normals2_points())
    r = pm.normals_ratio(layout, got).reshape(-1, 2)
    one = pm.radius_is_one(layout)
    w = _worst(f"normals{layout}_words, u < 1", r[~one])
    w1 = _worst(f"normals{layout}_words, u == 1 (|g| / 1e-149 where above it)", r[one])
    assert w <= 1.0 and w1 <= 1.0


@pytest.mark.parametrize("model,nu", [(pm.GAUSSIAN, 0.0), (pm.EXPONENTIAL, 0.0)] + [(pm.MATERN, nu) for nu in pm.MATERN_NU])
def test_spectral_amp_meets_its_bar(model, nu):
    got = _dev(pm.SPECTRAL_AMP, *pm.spectral_points(model, nu), model=model, nu=nu)
    assert np.all(np.isfinite(got)) and np.all(got >= 0)
    assert _worst(f"spectral_amp model {model} nu {nu}", pm.spectral_ratio(model, nu, got)) <= 1.0


def test_hook_agrees_with_debug_normals_byte_for_byte():
    """gsm_debug_normals draws its words on the device; NORMALS2_WORDS gets the oracle's words for the same counters: the same bytes, so the
    hook runs the body production runs and the device's philox_draw is the oracle's."""
    import torch
    from mcmc_gpu_amd import _lib
    lib = _lib.load()
    n = 3000
    for seed, step, stream, idx0 in ((7, 0, po.STREAM_SPECTRUM, 0), (2 ** 63 + 12345, -5, po.STREAM_NUGGET, 2 ** 32 - 1000)):
        out = torch.empty(2 * n, dtype=torch.float64, device="cuda:0")
        assert lib.gsm_debug_normals(C.c_uint64(seed), step, stream, idx0, n, C.c_void_p(out.data_ptr()), None) == 0
        idx = ((np.arange(n, dtype=np.uint64) + np.uint64(idx0)) & np.uint64(0xFFFFFFFF))
        words = po.draw(seed, step & (2 ** 64 - 1), stream, idx)
        assert out.cpu().numpy().tobytes() == _dev(pm.NORMALS2_WORDS, words).tobytes()


def test_refuses_bad_arguments_and_writes_nothing():
    import torch
    from mcmc_gpu_amd import _lib
    lib = _lib.load()
    x = torch.full((64,), 0.5, dtype=torch.float64, device="cuda:0")
    out = torch.full((256,), 12345.0, dtype=torch.float64, device="cuda:0")
    p, o = C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr())
    call = lib.gsm_debug_proposal_math
    assert call(8, 0, 0.0, 4, p, p, p, p, o, None) == -1                     # unknown selector
    assert call(-1, 0, 0.0, 4, p, p, p, p, o, None) == -1
    assert call(pm.LOG_TAB, 0, 0.0, 0, p, None, None, None, o, None) == -1      # n < 1
    assert call(pm.LOG_TAB, 0, 0.0, -3, p, None, None, None, o, None) == -1
    assert call(pm.LOG_TAB, 0, 0.0, 4, None, None, None, None, o, None) == -1   # NULL input
    assert call(pm.LOG_TAB, 0, 0.0, 4, p, None, None, None, None, None) == -1   # NULL output
    assert call(pm.NORMALS4_WORDS, 0, 0.0, 4, None, None, None, None, o, None) == -1
    assert call(pm.SPECTRAL_AMP, 0, 0.0, 4, p, p, p, None, o, None) == -1       # spectral_amp reads four arrays
    assert call(pm.SPECTRAL_AMP, 0, 0.0, 4, p, None, p, p, o, None) == -1
    assert call(pm.SPECTRAL_AMP, 3, 0.0, 4, p, p, p, p, o, None) == -1          # unknown model
    torch.cuda.synchronize()
    assert bool((out == 12345.0).all())
    assert call(pm.LOG_TAB, 0, 0.0, 4, p, None, None, None, o, None) == 0
    got = out.cpu().numpy()
    assert np.all(got[:4] != 12345.0) and np.all(got[4:] == 12345.0)         # n elements, no more
