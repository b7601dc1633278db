"""CPU: the bar tests/test_gpu_special.py holds the device to is fair -- csrc/normal_score.h and csrc/truncnorm.h, built with g++
against glibc, meet every bound of tests/special_common.py on every point set, with room to spare against mpmath (truncnorm.ppf:
at most half the model bound, and the bound's exclusion rule leaves out at most 2 % of a regime).  local_cov_of is device code
(sgs_search.h); its bounds are checked on the same operations in NumPy's IEEE doubles.  DESIGN.md records the maxima."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import special_common as sc

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """name -> function on arrays, from the g++ builds of tests/native/truncnorm_host.cpp and normal_score_host.cpp."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not found")
    tmp = tmp_path_factory.mktemp("special")
    libs = {}
    for name in ("truncnorm_host", "normal_score_host"):
        so = tmp / f"lib{name}.so"
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", str(ROOT / "mcmc_gpu_amd" / "csrc"), "-o", str(so),
                        str(ROOT / "tests" / "native" / f"{name}.cpp")], check=True)
        libs[name] = C.CDLL(str(so))
    dp = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")

    def wrap(fn, n_in):
        fn.argtypes = [dp] * (n_in + 1) + [C.c_int]
        fn.restype = None

        def call(*xs):
            xs = [np.ascontiguousarray(x, dtype=np.float64) for x in xs]
            out = np.empty_like(xs[0])
            fn(*xs, out, out.size)
            return out
        return call
    tn, ns = libs["truncnorm_host"], libs["normal_score_host"]
    return dict(ndtr=wrap(ns.ns_ndtr, 1), ndtri=wrap(ns.ns_ndtri, 1), erfc=wrap(ns.ns_erfc, 1), log_ndtr=wrap(tn.tn_log_ndtr, 1),
                ndtri_exp=wrap(tn.tn_ndtri_exp, 1), erfcx_pos=wrap(tn.tn_erfcx_pos, 1), log_gauss_mass=wrap(tn.tn_log_gauss_mass, 2),
                ppf=wrap(tn.tn_ppf, 3))


def _worst(name, r):
    w = float(np.nanmax(r))
    print(f"{name}: largest |error| / bound = {w:.3f} over {int(np.sum(~np.isnan(r)))} points")
    return w


def test_normal_score_functions_meet_their_bounds(host):
    p, x = sc.normal_score_points()
    got = host["ndtri"](p)
    assert _worst("ndtri", sc.ndtri_ratio(p, got)) <= 1.0
    assert _worst("ndtri vs mpmath", sc.ndtri_mp_ratio(got)) <= 1.0
    assert _worst("ndtr", sc.ndtr_ratio(x, host["ndtr"](x))) <= 1.0
    assert _worst("erfc_c", sc.erfc_ratio(x, host["erfc"](x))) <= 1.0


def test_scipy_ndtri_leaves_the_elementwise_bound_in_the_asymptotic_form():
    """Why ndtri_ratio holds the asymptotic form to 4 eps (|x| + 1) and not to 4e-16 max(1, |x|): scipy itself, with glibc's
    log, is further than that from mpmath (1.3 x on these points, at |x| in [1.1, 2.2]) and inside the corrected bound."""
    import scipy.special as sp
    p = sc.normal_score_points()[0]
    with np.errstate(all="ignore"):
        ref = sp.ndtri(p)
    assert _worst("scipy ndtri vs mpmath, 4e-16 max(1, |x|)", sc.ndtri_mp_ratio(ref, elementwise=True)) > 1.0
    assert _worst("scipy ndtri vs mpmath, corrected bound", sc.ndtri_mp_ratio(ref)) <= 1.0


def test_truncnorm_scalar_functions_meet_their_bounds(host):
    x, y, e = sc.truncnorm_scalar_points()
    assert _worst("log_ndtr", sc.log_ndtr_ratio(x, host["log_ndtr"](x))) <= 1.0
    assert _worst("ndtri_exp", sc.ndtri_exp_ratio(y, host["ndtri_exp"](y))) <= 1.0
    assert _worst("erfcx_pos", sc.erfcx_ratio(e, host["erfcx_pos"](e))) <= 1.0


@pytest.mark.parametrize("region", sc.PPF_REGIMES + ("edges",))
def test_ppf_and_log_gauss_mass_meet_their_bounds(host, region):
    q, a, b = sc.ppf_points(region)
    got = host["ppf"](q, a, b)
    assert _worst(f"ppf {region} vs scipy", sc.ppf_ratio(region, got)) <= 1.0
    r, kept = sc.ppf_mp_ratio(region, got)
    print(f"ppf {region} vs mpmath: kept share {kept:.4f}")
    if region != "infinite":                    # the finite regimes; with no bound at all the third of the q that approach 1 reach
        assert kept >= 0.98                     # Phi(x) = 1 (x > 7.5) in one case of nine
    else:
        assert kept >= 0.85
    assert _worst(f"ppf {region} vs mpmath", r) <= 0.5
    assert _worst(f"log_gauss_mass {region}", sc.log_gauss_mass_ratio(a, b, host["log_gauss_mass"](a, b))) <= 1.0


@pytest.mark.parametrize("vtype", [0, 1, 2])
def test_local_cov_bounds_hold_for_ieee_doubles(vtype):
    assert _worst(f"local_cov_of vtype {vtype}", sc.local_cov_ratio(vtype, sc.local_cov_numpy(vtype))) <= 1.0
