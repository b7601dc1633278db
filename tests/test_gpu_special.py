"""-m gpu: the scalar special functions as the device computes them (gsm_debug_special: the device compiler's code and ROCm's
exp / log / log1p / expm1 / hypot / sqrt where tests/test_special_host.py has g++ and glibc) against scipy 1.15, and for
truncnorm.ppf and local_cov_of against mpmath -- at the point sets and bounds of tests/special_common.py, which are the host
build's and are not tuned to the device.  Each test prints the largest |error| / bound it met (DESIGN.md records them)."""
import ctypes as C

import numpy as np
import pytest

import special_common as sc

pytestmark = pytest.mark.gpu
NDTR, NDTRI, ERFC, LOG_NDTR, NDTRI_EXP, ERFCX_POS, LOG_GAUSS_MASS, PPF, DRAW, LOCAL_COV = range(10)   # GSM_SPECIAL_* (include/gsm.h)


def _dev(which, *xs, vtype=0):
    """(out, flag word) of one gsm_debug_special launch on the arrays xs."""
    import torch
    from mcmc_gpu_amd import _lib
    lib = _lib.load()
    d = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to("cuda:0") for x in xs]
    out = torch.full_like(d[0], 12345.0)
    flag = torch.full((1,), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    ptr = [C.c_void_p(t.data_ptr()) for t in d] + [None] * (5 - len(d))
    rc = lib.gsm_debug_special(which, vtype, d[0].numel(), *ptr, C.c_void_p(out.data_ptr()), C.c_void_p(flag.data_ptr()), None)
    assert rc == 0, rc
    return out.cpu().numpy(), int(flag.item())


def _worst(name, r):
    w = float(np.nanmax(r))
    print(f"{name}: largest |error| / bound = {w:.3f} over {int(np.sum(~np.isnan(r)))} points")
    return w


def test_normal_score_functions_meet_the_host_bounds():
    p, x = sc.normal_score_points()
    got = _dev(NDTRI, p)[0]
    assert _worst("ndtri", sc.ndtri_ratio(p, got)) <= 1.0
    assert _worst("ndtri vs mpmath", sc.ndtri_mp_ratio(got)) <= 1.0
    assert _worst("ndtr", sc.ndtr_ratio(x, _dev(NDTR, x)[0])) <= 1.0
    assert _worst("erfc_c", sc.erfc_ratio(x, _dev(ERFC, x)[0])) <= 1.0


def test_truncnorm_scalar_functions_meet_the_host_bounds():
    x, y, e = sc.truncnorm_scalar_points()
    assert _worst("log_ndtr", sc.log_ndtr_ratio(x, _dev(LOG_NDTR, x)[0])) <= 1.0
    assert _worst("ndtri_exp", sc.ndtri_exp_ratio(y, _dev(NDTRI_EXP, y)[0])) <= 1.0
    assert _worst("erfcx_pos", sc.erfcx_ratio(e, _dev(ERFCX_POS, e)[0])) <= 1.0


@pytest.mark.parametrize("region", sc.PPF_REGIMES + ("edges",))
def test_ppf_and_log_gauss_mass_meet_the_host_bounds(region):
    q, a, b = sc.ppf_points(region)
    got, flag = _dev(PPF, q, a, b)
    assert flag == 0
    assert _worst(f"ppf {region} vs scipy", sc.ppf_ratio(region, got)) <= 1.0
    assert _worst(f"ppf {region} vs mpmath", sc.ppf_mp_ratio(region, got)[0]) <= 1.0
    assert _worst(f"log_gauss_mass {region}", sc.log_gauss_mass_ratio(a, b, _dev(LOG_GAUSS_MASS, a, b)[0])) <= 1.0


@pytest.mark.parametrize("vtype", [0, 1, 2])
def test_local_cov_of_against_mpmath(vtype):
    h2, c0, sill = sc.local_cov_points()
    got, _ = _dev(LOCAL_COV, h2, c0, sill, vtype=vtype)
    assert _worst(f"local_cov_of vtype {vtype}", sc.local_cov_ratio(vtype, got)) <= 1.0


@pytest.mark.parametrize("region", sc.PPF_REGIMES)
def test_truncnorm_draw_is_the_ppf_scaled_and_shifted(region):
    """Valid rows: ppf(u, (lo - est) / sd, (hi - est) / sd) * sd + est bit for bit, ppf from the ppf selector on the standardised
    bounds (a subtraction and a division: the same doubles on the host); no flag."""
    u, a, b = sc.ppf_points(region)
    rng = np.random.default_rng(23)
    est, sd = rng.normal(0.0, 2.0, u.size), 10.0 ** rng.uniform(-3, 0.5, u.size)
    lo, hi = a * sd + est, b * sd + est
    with np.errstate(invalid="ignore"):
        ta, tb = (lo - est) / sd, (hi - est) / sd
    ok = ta < tb                                  # the narrow regime loses rows where 1e-8 sd is below the spacing of the bounds
    assert ok.mean() > 0.9
    est, sd, lo, hi, u, ta, tb = (v[ok] for v in (est, sd, lo, hi, u, ta, tb))
    got, flag = _dev(DRAW, est, sd, lo, hi, u)
    ppf, _ = _dev(PPF, u, ta, tb)
    assert flag == 0
    with np.errstate(invalid="ignore"):
        np.testing.assert_array_equal(got, ppf * sd + est)
    assert np.isfinite(got).mean() > 0.85


def test_truncnorm_draw_domain_errors_flag_128_and_leave_the_rest_alone():
    """sd in {0, -1, NaN}, lo == hi, lo > hi and a NaN estimate: NaN and flag 128 (scipy returns loc for scale 0 and raises for the
    others; gsm_sgs_grid reports the flag); the valid element of the same launch is what it is alone."""
    rows = np.array([(0.2, 0.5, -1.0, 1.0, 0.3),                       # valid
                     (0.2, 0.0, -1.0, 1.0, 0.3), (0.2, -1.0, -1.0, 1.0, 0.3), (0.2, np.nan, -1.0, 1.0, 0.3),
                     (0.2, 0.5, 0.7, 0.7, 0.3), (0.2, 0.5, 1.0, -1.0, 0.3), (np.nan, 0.5, -1.0, 1.0, 0.3),
                     (0.2, 0.5, np.nan, 1.0, 0.3), (0.2, 0.5, -1.0, np.nan, 0.3)])
    alone, flag = _dev(DRAW, *rows[:1].T)
    assert flag == 0 and np.isfinite(alone[0]) and -1.0 <= alone[0] <= 1.0
    for k in range(1, rows.shape[0]):
        got, flag = _dev(DRAW, *rows[[k, 0]].T)
        assert flag == 128 and np.isnan(got[0]) and got[1] == alone[0], (k, got, flag)
    got, flag = _dev(DRAW, *rows.T)
    assert flag == 128 and got[0] == alone[0] and np.all(np.isnan(got[1:]))
    # a NaN uniform is no domain error: NaN without a flag
    got, flag = _dev(DRAW, *np.array([(0.2, 0.5, -1.0, 1.0, np.nan), rows[0]]).T)
    assert flag == 0 and np.isnan(got[0]) and got[1] == alone[0]


def test_debug_special_rejects_bad_arguments():
    import torch
    from mcmc_gpu_amd import _lib
    lib = _lib.load()
    x = torch.zeros(4, dtype=torch.float64, device="cuda:0")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    p, f = C.c_void_p(x.data_ptr()), C.c_void_p(flag.data_ptr())
    assert lib.gsm_debug_special(10, 0, 4, p, p, p, p, p, p, f, None) == -1             # unknown selector
    assert lib.gsm_debug_special(-1, 0, 4, p, p, p, p, p, p, f, None) == -1
    assert lib.gsm_debug_special(PPF, 0, 4, p, p, None, None, None, p, f, None) == -1    # ppf reads three arrays
    assert lib.gsm_debug_special(NDTR, 0, 0, p, None, None, None, None, p, f, None) == -1
    assert lib.gsm_debug_special(NDTR, 0, 4, p, None, None, None, None, None, f, None) == -1
    assert lib.gsm_debug_special(NDTR, 0, 4, p, None, None, None, None, p, None, None) == -1
    assert lib.gsm_debug_special(LOCAL_COV, 3, 4, p, p, p, None, None, p, f, None) == -1   # Matern: not evaluated on the device
    assert lib.gsm_debug_special(NDTR, 0, 4, p, None, None, None, None, p, f, None) == 0
