"""not gpu: the whole-grid path of the CPU restatement (oracle/sgs_oracle.sgs with `bounds`) against golden F14 -- the unmodified
reference's interpolate.sgs (scripts/make_fixtures_interp_sgs.py).  The oracle runs on the normal-score grid and the transformed
bounds of interpolate._Plan (scikit-learn's transformer, the reference's own call), so every neighbour search, kriging solve,
draw and generator advance of the reference is restated here.  Equality, not a tolerance: this is what pins the oracle that
tests/test_gpu_interp_sgs_geometry.py compares the device with on grids the fixtures do not hold."""
import json
import warnings
from pathlib import Path

import numpy as np
import pytest

import interp_sgs_common as ic
import sgs_oracle as so

GOLD = Path(__file__).resolve().parent / "golden"
pytest.importorskip("scipy.stats")
pytest.importorskip("sklearn.preprocessing")


@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_oracle_reproduces_interpolate_sgs_fixture(tag):
    from mcmc_gpu_amd import interpolate
    xx, yy, grid, cases = (ic.t2_like() if tag == "d" else ic.small())
    vario, kw, seeds = cases[tag]
    g = np.load(GOLD / f"f14{tag}_interp_sgs.npz", allow_pickle=False)
    plan = interpolate._Plan(xx, yy, grid, vario, kw["radius"], kw["num_points"], kw["ktype"], kw.get("sim_mask"), None, None,
                             kw.get("bounds"))
    assert so.STABLE_TIES is False                      # the fixtures are tie-free: the reference's own sort
    for s in seeds:
        rng = np.random.default_rng(s)
        trace = []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = so.sgs(xx, yy, plan.grid_ns, dict(vario), kw["radius"], kw["num_points"], kw["ktype"], sim_mask=kw.get("sim_mask"),
                         rng=rng, trace=trace, bounds=plan.bounds)
        assert rng.bit_generator.state == json.loads(str(g[f"{s}_state"]))
        assert np.array_equal(interpolate._inverse(plan, out), g[f"{s}_sim"], equal_nan=True)
        if tag == "d":                                  # outputs only
            continue
        tr = np.array(trace)
        assert np.array_equal(out, g[f"{s}_ns"], equal_nan=True)
        assert np.array_equal(tr[:, 0] * xx.shape[1] + tr[:, 1], g[f"{s}_cells"])
        assert np.array_equal(tr[:, 2], g[f"{s}_n"])
        assert np.array_equal(tr[:, 3:], g[f"{s}_est_var"])
