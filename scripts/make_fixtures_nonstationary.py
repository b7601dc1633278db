"""TEST INFRASTRUCTURE ONLY -- golden vectors F16 and F17: non-stationary interpolate.sgs and interpolate.krige, every variogram
parameter a map of the grid's shape (build container only; needs the reference tree).

F16 runs the UNMODIFIED gstatsim_custom.interpolate.sgs (gstatsMCMC/gstatsim_custom/interpolate.py:92-191), imported through
oracle/ref_loader.py, on the cases of tests/nonstationary_common.small() (interp_sgs_common.small()'s 40 x 44 tie-free grid
under smooth parameter maps) exactly as scripts/make_fixtures_interp_sgs.py runs the stationary ones: ok_solve / sk_solve are
wrapped to record, per visited cell in visiting order, the cell, its neighbour count, kriging estimate and |variance|, the
transformer's inverse_transform to record the simulated grid in normal-score space.  tests/golden/f16{a,b,c}_nonstationary.npz:
    a  exponential, ordinary kriging, 16 points, two seeds
    b  spherical, ordinary kriging, 24 points, bounds (truncated draws, lower == upper cells)
    c  gaussian, simple kriging, 8 points, a sim_mask, ranges x 0.25

F17 runs interpolate.krige on cases a and c (bounds dropped) as scripts/make_fixtures_krige.py does, its shim for the
_preprocess call included.  tests/golden/f17{a,c}_krige_nonstationary.npz hold what F15's files hold.

Outputs only, each file <= 200 KB.

    PYTHONDONTWRITEBYTECODE=1 python scripts/make_fixtures_nonstationary.py
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "oracle"))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "scripts"))
import ref_loader  # noqa: E402
import nonstationary_common as nc  # noqa: E402
import make_fixtures_interp_sgs as f14  # noqa: E402
import make_fixtures_krige as f15  # noqa: E402

GOLD = ROOT / "tests" / "golden"


def _save(path, out):
    np.savez_compressed(path, **out)
    print(path.name, path.stat().st_size, "bytes")
    assert path.stat().st_size <= 200 * 1024


def main():
    _, _, _, C = ref_loader.load_reference()
    interp = C.interpolate
    xx, yy, grid, cases = nc.small()
    for tag, (vario, kw, seeds) in cases.items():
        out = {}
        for s in seeds:
            sim, ns, cells, tr, st = f14.run(interp, xx, yy, grid, vario, s, **kw)
            assert np.isfinite(sim[kw.get("sim_mask", np.ones(grid.shape, bool))]).all()
            out[f"{s}_sim"], out[f"{s}_state"] = sim, st
            out[f"{s}_ns"], out[f"{s}_cells"] = ns, cells
            out[f"{s}_n"], out[f"{s}_est_var"] = tr[:, 0].astype(np.int8), tr[:, 1:]
            print(tag, s, "visited", cells.size, "n", int(tr[:, 0].min()), "..", int(tr[:, 0].max()))
        _save(GOLD / f"f16{tag}_nonstationary.npz", out)
    for tag in nc.KRIGE_TAGS:
        vario, kw, _ = cases[tag]
        kw = {k: v for k, v in kw.items() if k != "bounds"}
        est, std, est_ns, std_ns, cells, tr = f15.run(interp, xx, yy, grid, vario, **kw)
        mask = kw.get("sim_mask", np.ones(grid.shape, bool))
        assert np.array_equal(cells, np.flatnonzero(mask & np.isnan(grid)))          # C order
        assert np.isfinite(est[mask]).all() and np.isfinite(std[mask]).all()
        assert tr[:, 2].min() > 1e-3, tr[:, 2].min()                                  # sqrt in the sd comparison is well conditioned
        print(tag, "krige cells", cells.size, "n", int(tr[:, 0].min()), "..", int(tr[:, 0].max()), "min var", float(tr[:, 2].min()))
        _save(GOLD / f"f17{tag}_krige_nonstationary.npz",
              dict(est=est, std=std, est_ns=est_ns, std_ns=std_ns, n=tr[:, 0].astype(np.int8), est_var=tr[:, 1:]))


if __name__ == "__main__":
    main()
