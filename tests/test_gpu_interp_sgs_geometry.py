"""GPU: mcmc_gpu_amd.interpolate (gsm_sgs_grid, csrc/sgs_grid_kernel.hip) against the CPU oracle (oracle/sgs_oracle.sgs, pinned
bit for bit to the unmodified reference by golden F14, tests/test_oracle_interp_sgs_golden.py) on the grids F14 leaves out
(interp_sgs_common.geometry): square cells with distance ties, descending axes, cells far from square, several widenings of
the radius, the reference's default arguments.  Same bounds as test_gpu_interp_sgs.py uses against the reference.  The oracle
runs with the device's rule for equidistant candidates (ascending (distance, row, column); the reference's default argsort is
unstable there).  Then the error contract of gsm_sgs_grid for inputs the kernels check before they index anything."""
import functools
import warnings

import numpy as np
import pytest

import interp_sgs_common as ic
import sgs_oracle as so

pytestmark = pytest.mark.gpu
CASES = ic.geometry()


def _plan(cid):
    from mcmc_gpu_amd import interpolate
    xx, yy, grid, vario, kw, _ = CASES[cid]
    return interpolate._Plan(xx, yy, grid, vario, kw["radius"], kw["num_points"], kw["ktype"], kw.get("sim_mask"), None, None,
                             kw.get("bounds"))


@functools.lru_cache(maxsize=None)
def _oracle(cid):
    """seed -> (normal-score grid, trace [cells, (i, j, n, est, var)], generator state, logs of seed 5) of the oracle."""
    xx, yy, grid, vario, kw, seeds = CASES[cid]
    plan = _plan(cid)
    runs = {}
    for s in seeds:
        rng = np.random.default_rng(s)
        trace = []
        so.STABLE_TIES = True
        if s == 5:
            so.TIE_LOG, so.NBR_LOG, so.SEARCH_LOG = [], [], []
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                out = so.sgs(xx, yy, plan.grid_ns, dict(vario), kw["radius"], kw["num_points"], kw["ktype"],
                             sim_mask=kw.get("sim_mask"), rng=rng, trace=trace, bounds=plan.bounds)
            logs = (so.TIE_LOG, so.NBR_LOG, so.SEARCH_LOG)
        finally:
            so.STABLE_TIES, so.TIE_LOG, so.NBR_LOG, so.SEARCH_LOG = False, None, None, None
        runs[s] = (out, np.array(trace), rng.bit_generator.state, logs)
    return runs


def _assert_case_reaches_what_it_is_for(cid):
    """On the oracle's realisation of seed 5 alone: the property the case exists for."""
    xx, yy = CASES[cid][:2]
    _, tr, _, (ties, nbrs, searches) = _oracle(cid)[5]
    n = tr[:, 2]
    empty = [q for q in searches if q[3] == 0]
    if cid in ("G1", "G2", "G3", "G8"):
        assert len(ties) > 0, "no sector cut falls between equidistant candidates"
    if cid in ("G1", "G5", "G7"):
        assert len(empty) > 0, "no search comes back empty"
    if cid == "G3":
        assert n.max() == 48
    if cid == "G4":
        assert n.max() == 16
    if cid == "G5":
        assert max(q[2] for q in searches) == 10e3 + 200e3, "no search widens twice"
        assert n.min() == 1
    if cid == "G6":
        far = max(np.hypot(xx[i, j] - xx[a, b], yy[i, j] - yy[a, b]) for i, j, nb in nbrs for a, b in nb)
        assert far > 64 * 500.0, "no chosen neighbour beyond the 64 certification rings"
    if cid == "G7":
        assert max(max(a for a, _ in nb) - min(a for a, _ in nb) for _, _, nb in nbrs if nb) > 14


def _compare(cid, plan, ns, path, t, rng, ref):
    """One realisation of the device (normal scores, path, trace, generator) against the oracle's."""
    _compare_run(CASES[cid][2], CASES[cid][3], plan, ns, path, t, rng, ref[:3])


def _compare_run(grid, vario, plan, ns, path, t, rng, ref):
    out, tr, state = ref
    W = plan.W
    assert rng.bit_generator.state == state
    np.testing.assert_array_equal(path, tr[:, 0] * W + tr[:, 1])                                     # visiting order
    solved = t[:, 0] >= 0                                            # cells whose bounds coincide solve no system on the device
    if plan.bounds is not None:
        lo, hi = plan.bounds
        np.testing.assert_array_equal(~solved, (lo.ravel() == hi.ravel())[path])
    else:
        assert solved.all()
    np.testing.assert_array_equal(t[solved, 0], tr[solved, 2])                                       # neighbour counts
    np.testing.assert_allclose(t[solved, 1], tr[solved, 3], rtol=1e-9, atol=1e-12)                   # kriging estimates
    np.testing.assert_allclose(t[solved, 2], tr[solved, 4], rtol=1e-7, atol=1e-9 * vario["sill"])
    np.testing.assert_array_equal(np.isnan(ns), np.isnan(out))
    np.testing.assert_allclose(ns, out, rtol=0, atol=1e-8, equal_nan=True)                           # normal scores
    cond = ~np.isnan(grid)
    assert np.array_equal(ns[cond], out[cond])


@pytest.mark.parametrize("cid", sorted(CASES))
def test_interpolate_sgs_equals_oracle_trace(cid):
    from mcmc_gpu_amd import interpolate
    _assert_case_reaches_what_it_is_for(cid)
    seeds = CASES[cid][5]
    ref = _oracle(cid)
    plan = _plan(cid)
    rngs = [np.random.default_rng(s) for s in seeds]
    ns, (paths, tr) = interpolate._run(plan, rngs, trace=True)
    off = np.concatenate([[0], np.cumsum([p.size for p in paths])])
    for r, s in enumerate(seeds):
        _compare(cid, plan, ns[r], paths[r], tr[off[r]:off[r + 1]], rngs[r], ref[s])


def test_interpolate_sgs_through_the_truncnorm_regimes():
    """interp_sgs_common.regimes(): bounded draws far in both tails (standardised a >= 6, b <= -6) and from intervals of at most
    1e-3 sd -- the branches of truncnorm.h that the other cases' moderate bounds leave alone -- at the same bounds."""
    from mcmc_gpu_amd import interpolate
    c = ic.regimes()
    rng = np.random.default_rng(c["seed"])
    ns, (paths, tr) = interpolate._run(c["plan"], [rng], trace=True)
    _compare_run(c["grid"], c["vario"], c["plan"], ns[0], paths[0], tr, rng, (c["out"], c["trace"], c["state"]))


def test_sgs_many_equals_oracle_maps_on_square_north_up_cells():
    """G1 through the public entry: maps in data units, cells whose bounds coincide bit for bit."""
    from mcmc_gpu_amd import interpolate
    xx, yy, grid, vario, kw, seeds = CASES["G1"]
    ref = _oracle("G1")
    plan = _plan("G1")
    maps = interpolate.sgs_many(xx, yy, grid, vario, seeds, **kw)
    span = float(np.nanmax(grid) - np.nanmin(grid))
    deg = (plan.bounds[0] == plan.bounds[1]) & np.isnan(grid)
    assert deg.any()
    for r, s in enumerate(seeds):
        exp = interpolate._inverse(plan, ref[s][0])
        np.testing.assert_allclose(maps[r], exp, rtol=0, atol=1e-6 * span)
        assert np.array_equal(maps[r][deg], exp[deg])


@pytest.mark.parametrize("cid", ["G1", "G5"])
def test_segments_and_batching_change_no_bit(cid):
    from mcmc_gpu_amd import interpolate
    seeds = CASES[cid][5]
    assert len(seeds) == 3
    plan = _plan(cid)
    auto, _ = interpolate._run(plan, [np.random.default_rng(s) for s in seeds])
    seg, _ = interpolate._run(plan, [np.random.default_rng(s) for s in seeds], segment_cells=64)
    assert np.array_equal(seg, auto, equal_nan=True)
    for r, s in enumerate(seeds):
        one, _ = interpolate._run(plan, [np.random.default_rng(s)])
        assert np.array_equal(one[0], auto[r], equal_nan=True)


# ---- error contract of gsm_sgs_grid: inputs the kernels check before they index anything ------------------------------------------
def _small_plan():
    from mcmc_gpu_amd import interpolate
    xx, yy, grid, cases = ic.small()
    vario, kw, _ = cases["a"]
    return interpolate._Plan(xx, yy, grid, vario, kw["radius"], kw["num_points"], kw["ktype"], None, None, None, None)


def _with_path(plan, doctor):
    """`plan` whose draws list the path `doctor` makes of the real one (same length, so the draws still line up)."""
    draws = plan.draws

    def doctored(rng):
        path, d = draws(rng)
        path = path.copy()
        doctor(path)
        return path, d
    plan.draws = doctored
    return plan


def test_path_cell_listed_twice_or_holding_a_value_raises():
    from mcmc_gpu_amd import interpolate, _lib
    good, _ = interpolate._run(_small_plan(), [np.random.default_rng(3)])

    def twice(path):
        path[-1] = path[0]

    def holds_a_value(path):
        path[7] = 0                                                      # cell (0, 0) is conditioning data
    assert _small_plan().cond[0, 0]
    for doctor in (twice, holds_a_value):
        with pytest.raises(_lib.GsmError, match="listed twice"):
            interpolate._run(_with_path(_small_plan(), doctor), [np.random.default_rng(3)])
        again, _ = interpolate._run(_small_plan(), [np.random.default_rng(3)])
        assert np.array_equal(again, good, equal_nan=True)


def test_lag_table_too_small_raises(monkeypatch):
    from mcmc_gpu_amd import interpolate, _lib
    good, _ = interpolate._run(_small_plan(), [np.random.default_rng(3)])
    with monkeypatch.context() as m:
        m.setattr(interpolate, "_lag_extents", lambda plan, eng, torch: (1, 1))
        with pytest.raises(_lib.GsmError, match="lag covariance table"):
            interpolate._run(_small_plan(), [np.random.default_rng(3)])
    again, _ = interpolate._run(_small_plan(), [np.random.default_rng(3)])
    assert np.array_equal(again, good, equal_nan=True)
