"""CPU: the Gaussian trend filter's checker and host surface (mcmc_gpu_amd.sgs.trend_of, gaussian_weights).

test_scipy_within_bar shows that the bar of tests/trend_common.py is fair: scipy.ndimage.gaussian_filter itself lies within B of the
long-double restatement on every host case (its largest error on these cases is about 0.2 B; each ratio is printed).  The device is held
to the same B by tests/test_gpu_trend.py."""
import numpy as np
import pytest
from scipy.ndimage import gaussian_filter

import trend_common as tc
from mcmc_gpu_amd import sgs


@pytest.mark.parametrize("case", tc.HOST_CASES, ids=tc.case_id)
def test_scipy_within_bar(case):
    H, W, sigma = case
    for x in tc.fields(H, W):
        ratio = tc.worst_ratio(gaussian_filter(x, sigma=sigma), x, sigma)
        print(f"{tc.case_id(case)}: scipy's largest error = {ratio:.3f} B")
        assert ratio <= 1.0


def test_weights_are_scipys():
    """gaussian_weights against the weights scipy applies, recovered by filtering a unit impulse far from the edges (one product per
    output cell, no sum: exact)."""
    for sigma, trunc in ((10, 4.0), (3, 4.0), (0.7, 4.0), (2.5, 3.0)):
        w = sgs.gaussian_weights(sigma, trunc)
        lw = int(trunc * float(sigma) + 0.5)
        assert w.size == 2 * lw + 1 and w.dtype == np.float64
        x = np.zeros((1, 4 * lw + 3))
        x[0, 2 * lw + 1] = 1.0
        got = gaussian_filter(x, sigma=(1e-16, sigma), truncate=trunc)[0, lw + 1:3 * lw + 2]       # axis 0 skipped by scipy (sigma <= 1e-15)
        np.testing.assert_array_equal(got, w[::-1])
        np.testing.assert_array_equal(w, w[::-1])


def test_restatement_reflects_like_scipy():
    """The reflection of the restatement on axes shorter than the half-width, against scipy at float64 accuracy, and refl itself."""
    np.testing.assert_array_equal(tc.refl(np.arange(-9, 9), 3), [2, 1, 0, 0, 1, 2] * 3)          # .. c b a | a b c | c b a ..
    np.testing.assert_array_equal(tc.refl(np.arange(-3, 4), 1), 0)
    x = tc.fields(2, 3)[0]
    np.testing.assert_allclose(np.asarray(tc.restatement(x, 10), dtype=np.float64), gaussian_filter(x, sigma=10), rtol=1e-13)


def test_trend_of_host_is_scipy_bit_for_bit():
    x = tc.fields(13, 37)
    for sigma in (10, 3, (3, 10)):
        want = np.stack([gaussian_filter(b, sigma=sigma) for b in x])
        np.testing.assert_array_equal(sgs.trend_of(x, sigma=sigma, device=False), want)
        np.testing.assert_array_equal(sgs.trend_of(x[1], sigma=sigma, device=False), want[1])
    np.testing.assert_array_equal(sgs.trend_of(x[0], sigma=2, truncate=3.0, device=False), gaussian_filter(x[0], sigma=2, truncate=3.0))
    assert sgs.trend_of(x[0].astype(np.float32), device=False).dtype == np.float64


def test_trend_of_argument_errors():
    import torch
    x = tc.fields(8, 9)
    with pytest.raises(ValueError, match="reflect"):
        sgs.trend_of(x, mode="nearest", device=False)
    with pytest.raises(ValueError, match="reflect"):
        sgs.trend_of(x, mode="constant")
    for bad in (0, -1.0, np.nan, (1, 2, 3), np.inf):
        with pytest.raises(ValueError, match="sigma"):
            sgs.trend_of(x, sigma=bad, device=False)
    with pytest.raises(ValueError, match="truncate"):
        sgs.trend_of(x, truncate=0, device=False)
    for shape in ((5,), (2, 3, 4, 5), (0, 4)):
        with pytest.raises(ValueError, match="beds"):
            sgs.trend_of(np.zeros(shape), device=False)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no ROCm/HIP device"):
            sgs.trend_of(x, device=True)
        np.testing.assert_array_equal(sgs.trend_of(x[0]), gaussian_filter(x[0], sigma=10))        # device=None: scipy without a GPU
