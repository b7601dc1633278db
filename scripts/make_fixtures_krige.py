"""TEST INFRASTRUCTURE ONLY -- golden vector F15 for mcmc_gpu_amd.interpolate.krige (build container only; needs the reference tree).

Runs gstatsim_custom.interpolate.krige (gstatsMCMC/gstatsim_custom/interpolate.py:13-89), imported through oracle/ref_loader.py,
on cases a, b and c of tests/interp_sgs_common.small() (each case's variogram, radius, num_points, ktype and sim_mask; `bounds`
dropped, krige has none).  The reference's krige cannot be called as it stands: it unpacks seven values from
_preprocess(xx, yy, grid, variogram, sim_mask, radius, stencil), and _preprocess now takes an eighth argument `bounds` and
returns eight values.  This script installs a shim for that call alone (bounds=None, the first seven values) and changes nothing
else.  It wraps interpolate's ok_solve / sk_solve to record, per solved cell in visiting order, the neighbour count, kriging
estimate and signed variance, and the transformer's inverse_transform to record the two grids in normal-score space, and writes
tests/golden/f15{a,b,c}_krige.npz (outputs only, each <= 200 KB):
    est, std        krige's return value, data units
    est_ns, std_ns  the grids krige hands to inverse_transform
    n (int8), est_var [cells, 2]   per solved cell, in C order of the cells of sim_mask that hold no value

    PYTHONDONTWRITEBYTECODE=1 python scripts/make_fixtures_krige.py
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "oracle"))
sys.path.insert(0, str(ROOT / "tests"))
import ref_loader  # noqa: E402
import interp_sgs_common as ic  # noqa: E402

GOLD = ROOT / "tests" / "golden"


def run(interp, xx, yy, grid, vario, **kw):
    rec, ns = [], []
    ok0, sk0, gt0, pp0 = interp.ok_solve, interp.sk_solve, interp.gaussian_transformation, interp._preprocess

    def ok(sim_xy, nearest, v, *a, **k):
        est, var = ok0(sim_xy, nearest, v, *a, **k)
        rec.append((sim_xy[0], sim_xy[1], nearest.shape[0], est, var))
        return est, var

    def sk(sim_xy, nearest, v, gm, *a, **k):
        est, var = sk0(sim_xy, nearest, v, gm, *a, **k)
        rec.append((sim_xy[0], sim_xy[1], nearest.shape[0], est, var))
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
    interp._preprocess = lambda *a: pp0(*a, None)[:7]
    try:
        est, std = interp.krige(xx, yy, grid, vario, quiet=True, **kw)
    finally:
        interp.ok_solve, interp.sk_solve, interp.gaussian_transformation, interp._preprocess = ok0, sk0, gt0, pp0
    xs, ys = xx[0, :], yy[:, 0]
    t = np.array(rec, dtype=np.float64).reshape(-1, 5)
    cells = (np.searchsorted(ys, t[:, 1]) * xx.shape[1] + np.searchsorted(xs, t[:, 0])).astype(np.int32)
    assert np.array_equal(xs[cells % xx.shape[1]], t[:, 0]) and np.array_equal(ys[cells // xx.shape[1]], t[:, 1])
    assert len(ns) == 2
    return est, std, ns[0].reshape(xx.shape), ns[1].reshape(xx.shape), cells, t[:, 2:]


def main():
    _, _, _, C = ref_loader.load_reference()
    xx, yy, grid, cases = ic.small()
    for tag in ("a", "b", "c"):
        vario, kw, _ = cases[tag]
        kw = {k: v for k, v in kw.items() if k != "bounds"}
        est, std, est_ns, std_ns, cells, tr = run(C.interpolate, xx, yy, grid, vario, **kw)
        mask = kw.get("sim_mask", np.ones(grid.shape, bool))
        assert np.array_equal(cells, np.flatnonzero(mask & np.isnan(grid)))          # C order
        assert np.isfinite(est[mask]).all() and np.isfinite(std[mask]).all()
        assert tr[:, 2].min() > 1e-3, tr[:, 2].min()                                  # sqrt in the sd comparison is well conditioned
        path = GOLD / f"f15{tag}_krige.npz"
        np.savez_compressed(path, est=est, std=std, est_ns=est_ns, std_ns=std_ns, n=tr[:, 0].astype(np.int8), est_var=tr[:, 1:])
        print(path.name, path.stat().st_size, "bytes; cells", cells.size, "n", int(tr[:, 0].min()), "..", int(tr[:, 0].max()),
              "min var", float(tr[:, 2].min()))
        assert path.stat().st_size <= 200 * 1024


if __name__ == "__main__":
    main()
