"""CPU: the bars tests/test_gpu_proposal_math.py holds the device to are fair, and its point sets reach what they are for.
tests/native/proposal_math_host.cpp -- csrc/math_tables.h itself plus a restatement of exp_lean, sqrt_lean, the two Box-Muller bodies and
spectral_amp with the same fmas, built with g++ -ffp-contract=off -- stays inside every bar of tests/proposal_math_common.py on every point.
Each test prints the largest |error| / bar it met (DESIGN.md records them)."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import proposal_math_common as pm

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """host(selector, *arrays, model=0, nu=0.0) -> the program's output doubles"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not found")
    exe = tmp_path_factory.mktemp("proposal_math") / "proposal_math_host"
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-I", str(ROOT / "mcmc_gpu_amd" / "csrc"), "-o", str(exe),
                    str(ROOT / "tests" / "native" / "proposal_math_host.cpp")], check=True)

    def call(which, *arrays, model=0, nu=0.0):
        n = arrays[0].shape[0]
        r = subprocess.run([str(exe), str(which), str(model), repr(float(nu)), str(n)], input=b"".join(np.ascontiguousarray(a).tobytes() for a in arrays),
                           capture_output=True)
        assert r.returncode == 0, r.stderr
        return np.frombuffer(r.stdout, dtype=np.float64)
    return call


def _worst(name, r):
    w = float(np.max(r))
    print(f"{name}: largest |error| / bar = {w:.3f} over {r.size} values")
    return w


def test_log_tab(host):
    x = pm.log_points()
    assert np.all(x > 0) and np.all(np.isfinite(x)) and np.all(x >= 2.0 ** -1022)
    e, i = pm.log_interval(x)
    assert set(i.tolist()) == set(range(128)) and e.min() <= -53 and e.max() >= 40     # every table interval, the whole exponent range
    for ex in (-1, 0):                                                                  # both sides of every interval boundary next to 1
        assert set(i[e == ex].tolist()) == set(range(128))
    assert 1.0 in x and 2.0 ** -32 in x and np.sum((x > 1.0) & (x < 1.0 + 1e-9)) >= 3  # u == 1, the smallest uniform, the k = 0 arguments
    got = host(pm.LOG_TAB, x)
    assert _worst("log_tab", pm.log_ratio(got)) <= 1.0
    assert got[x == 1.0].tolist() == [0.0] * int(np.sum(x == 1.0))                      # exactly: the radius of u == 1 is sqrt_lean's stand-in for 0


def test_sincos_tab(host):
    u = pm.sincos_points()
    a = u * 64.0
    assert {float(j) for j in range(64)} <= set(a.tolist()) and {j + 0.5 for j in range(64)} <= set(a.tolist())   # every node, every rint tie
    assert 0.0 in u and 1.0 - 2.0 ** -53 in u and 1.0 - 2.0 ** -32 in u
    assert _worst("sincos_tab", pm.sincos_ratio(host(pm.SINCOS_TAB, u))) <= 1.0


def test_sqrt_lean(host):
    t = pm.sqrt_points()
    assert np.sum(t <= pm.SQRT_FLOOR) >= 4 and 73.5 in t and 2.0 ** 499 in t
    assert _worst("sqrt_lean", pm.sqrt_ratio(host(pm.SQRT_LEAN, t))) <= 1.0


def test_exp_lean(host):
    x = pm.exp_points()
    truth = pm.exp_truth()[0]
    assert any(0 < v < pm.MIN_NORMAL for v in truth) and np.sum(x <= pm.EXP_ZERO_BELOW) >= 4     # subnormal results, zero results
    assert x.min() <= -1e300 and np.any((x < -2.0 ** 31 * np.log(2.0)) & (x > -1e10))            # k = rint(x / ln 2) beyond -2^31
    got = host(pm.EXP_LEAN, x)
    assert np.any((got > 0) & (got < 2.0 ** -1022)) and np.any(got == 0.0)
    assert _worst("exp_lean", pm.exp_ratio(got)) <= 1.0


@pytest.mark.parametrize("layout", [4, 2])
def test_normals_on_words(host, layout):
    words = pm.normals4_points() if layout == 4 else pm.normals2_points()
    one = pm.radius_is_one(layout)
    assert one.any() and not one.all()                                                           # u == 1 is there
    got = host(pm.NORMALS4_WORDS if layout == 4 else pm.NORMALS2_WORDS, words)
    r = pm.normals_ratio(layout, got)
    assert _worst(f"normals{layout}_words, u < 1", r.reshape(-1, 2)[~one]) <= 1.0
    assert _worst(f"normals{layout}_words, u == 1", r.reshape(-1, 2)[one]) <= 1.0


@pytest.mark.parametrize("model,nu", [(pm.GAUSSIAN, 0.0), (pm.EXPONENTIAL, 0.0)] + [(pm.MATERN, nu) for nu in pm.MATERN_NU])
def test_spectral_amp(host, model, nu):
    pts = pm.spectral_points(model, nu)
    assert np.any(pts[3] < 1.1e-20) and np.any(pts[3] > 0.19)                                    # the DC entry of a k2 table (1e-10 squared), a Nyquist corner at 10 m
    got = host(pm.SPECTRAL_AMP, *pts, model=model, nu=nu)
    assert np.all(np.isfinite(got)) and np.all(got >= 0)
    if model == pm.GAUSSIAN:
        assert np.any(got == 0.0) and np.any((got > 0.99) & (got <= 1.0))
    assert _worst(f"spectral_amp model {model} nu {nu}", pm.spectral_ratio(model, nu, got)) <= 1.0


def test_philox_points_hold_the_known_answers():
    rows, exp = pm.philox_points()
    assert rows.shape[1] == 6 and exp.shape == (rows.shape[0], 4)
    assert np.any(rows[:, 5] == 2 ** 32 - 1) and np.any(rows[:, 3] == 0xFFFFFFFF) and np.any((rows[:, 3] > 0) & (rows[:, 3] < 0xFFFFFFFF))
    assert np.any(rows[:, 1] >= 2 ** 31)
