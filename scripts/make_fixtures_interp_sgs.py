"""TEST INFRASTRUCTURE ONLY -- golden vector F14 for mcmc_gpu_amd.interpolate (build container only; needs the reference tree).

Runs the UNMODIFIED gstatsim_custom.interpolate.sgs (gstatsMCMC/gstatsim_custom/interpolate.py:92-191), imported through
oracle/ref_loader.py, on synthetic tie-free grids (rows sgs_common.TIE_FREE_DY apart: the reference's argsort is unstable on
equidistant candidates; tests/interp_sgs_common.py builds the inputs).  This script wraps interpolate's ok_solve / sk_solve to record, per visited cell in visiting order, the
cell, its neighbour count, kriging estimate and |variance|, and the transformer's inverse_transform to record the simulated
grid in normal-score space, and writes tests/golden/f14{a,b,c,d}_interp_sgs.npz (one file per case, each
<= 200 KB).  Cases:
    a  40 x 44, ordinary kriging, Matern, no bounds, two seeds, a data gap wider than the radius (the search widens)
    b  the same grid, exponential model, a numeric lower bound and an upper-bound map with lower == upper cells
    c  simple kriging, spherical model, a sim_mask, bounds
    d  96 x 96, 48 neighbours, bounds as T2_StatisticalAnalysis.ipynb sets them (outputs only)

    PYTHONDONTWRITEBYTECODE=1 python scripts/make_fixtures_interp_sgs.py
"""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "oracle"))
sys.path.insert(0, str(ROOT / "tests"))
import ref_loader  # noqa: E402
import interp_sgs_common as ic  # noqa: E402

GOLD = ROOT / "tests" / "golden"


def state_json(rng):
    return json.dumps(rng.bit_generator.state)


def run(interp, xx, yy, grid, vario, seed, **kw):
    rec, ns = [], []
    ok0, sk0, gt0 = interp.ok_solve, interp.sk_solve, interp.gaussian_transformation

    def ok(sim_xy, nearest, v, rcond=None, precompute=False):
        est, var = ok0(sim_xy, nearest, v, rcond, precompute)
        rec.append((sim_xy[0], sim_xy[1], nearest.shape[0], est, abs(var)))
        return est, var

    def sk(sim_xy, nearest, v, gm, rcond=None, precompute=False):
        est, var = sk0(sim_xy, nearest, v, gm, rcond, precompute)
        rec.append((sim_xy[0], sim_xy[1], nearest.shape[0], est, abs(var)))
        return est, var

    def gt(g, m, n_quantiles=500):
        out, nst = gt0(g, m, n_quantiles)
        inv = nst.inverse_transform

        def record(x):
            ns.append(np.array(x, copy=True))
            return inv(x)
        nst.inverse_transform = record
        return out, nst

    interp.ok_solve, interp.sk_solve, interp.gaussian_transformation = ok, sk, gt
    try:
        rng = np.random.default_rng(seed)
        sim = interp.sgs(xx, yy, grid, vario, seed=rng, quiet=True, **kw)
    finally:
        interp.ok_solve, interp.sk_solve, interp.gaussian_transformation = ok0, sk0, gt0
    xs, ys = xx[0, :], yy[:, 0]
    t = np.array(rec, dtype=np.float64).reshape(-1, 5)
    cells = (np.searchsorted(ys, t[:, 1]) * xx.shape[1] + np.searchsorted(xs, t[:, 0])).astype(np.int32)
    assert np.array_equal(xs[cells % xx.shape[1]], t[:, 0]) and np.array_equal(ys[cells // xx.shape[1]], t[:, 1])
    return sim, ns[0].reshape(xx.shape), cells, t[:, 2:], state_json(rng)


def main():
    _, _, _, C = ref_loader.load_reference()
    interp = C.interpolate
    for setup, traces in ((ic.small, True), (ic.t2_like, False)):
        xx, yy, grid, cases = setup()
        for tag, (vario, kw, seeds) in cases.items():
            out = {}
            for s in seeds:
                sim, ns, cells, tr, st = run(interp, xx, yy, grid, vario, s, **kw)
                assert np.isfinite(sim[kw.get("sim_mask", np.ones(grid.shape, bool))]).all()
                out[f"{s}_sim"], out[f"{s}_state"] = sim, st
                if traces:
                    out[f"{s}_ns"], out[f"{s}_cells"] = ns, cells
                    out[f"{s}_n"], out[f"{s}_est_var"] = tr[:, 0].astype(np.int8), tr[:, 1:]
                print(tag, s, "visited", cells.size)
            path = GOLD / f"f14{tag}_interp_sgs.npz"
            np.savez_compressed(path, **out)
            print(path.name, path.stat().st_size, "bytes")
            assert path.stat().st_size <= 200 * 1024


if __name__ == "__main__":
    main()
