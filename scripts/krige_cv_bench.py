"""Throughput of kriging cross-validation on the device (gsm_krige_cv, csrc/krige_cv_kernel.hip) on the grid of
scripts/krige_bench.py: 566 x 566 cells of 500 m, data on flight lines, 48 neighbours within 50 km, Matern.  HIP events around
the calls (each the whole call: launches and the error word's read-back), uploads outside the timed window, one warm-up call,
then the median of --repeats.  Every comparison is made in the same process on the same operands, the whole-grid lag tables
included.

    (a) loo           leave-one-out at every data cell, one model: targets per second -- beside gsm_krige_grid on as many
                      cells WITHOUT a value (every k-th of them), the kernel this one was derived from
    (b) models        one call with four models (Matern, exponential, gaussian, spherical tables) against four one-model calls:
                      what sharing the neighbour search buys
    (c) folds         5 random folds in one call against the composition, five gsm_krige_grid calls on copies of the grid with a
                      fold set to NaN (the copies are made and uploaded outside the timed window, which flatters the composition)

    python scripts/krige_cv_bench.py [--size 566] [--repeats 5] [--out profiles/krige_cv_bench.json]
"""
import argparse
import ctypes as C
import json
import math
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "scripts"))


def main():
    import torch
    from mcmc_gpu_amd import interpolate
    from mcmc_gpu_amd.engine import GsmEngine, _ptr
    from mcmc_gpu_amd.sgs import lag_cov_table
    from sgs_grid_bench import problem
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=566)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "krige_cv_bench.json"))
    args = ap.parse_args()
    xx, yy, grid, matern, _ = problem(args.size)
    radius, num_points = 50e3, 48
    plan = interpolate._krige_plan(xx, yy, grid, matern, radius, num_points, "ok", None, None)
    H, W = plan.H, plan.W
    models = [matern,
              dict(major_range=30e3, minor_range=30e3, azimuth=0.0, sill=1.0, nugget=0.0, vtype="Exponential"),
              dict(major_range=1.0e3, minor_range=1.0e3, azimuth=0.0, sill=1.0, nugget=0.0, vtype="Gaussian"),   # two cells: no nugget
              dict(major_range=30e3, minor_range=30e3, azimuth=0.0, sill=1.0, nugget=0.0, vtype="Spherical")]
    data = np.flatnonzero(plan.cond).astype(np.int32)
    empty = np.flatnonzero(~plan.cond)
    empty = np.ascontiguousarray(empty[::empty.size // data.size][:data.size], dtype=np.int32)
    fold = interpolate.random_folds(plan.cond, k=5, seed=0)
    eng = GsmEngine(H, W, 1)
    try:
        dev, lib, h = eng.dev, eng.lib, eng.h
        hw = int(math.ceil(radius / abs(plan.dx)))
        f64 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
        i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
        d_grid, d_xs, d_ys, d_gm = f64(plan.grid_ns), f64(plan.xs), f64(plan.ys), f64([plan.global_mean])
        d_tab = f64(np.stack([lag_cov_table(m, hw, plan.dx, plan.dy, H - 1, W - 1) for m in models]))
        d_tab1 = [d_tab[m] for m in range(len(models))]
        sills = [float(m["sill"]) for m in models]
        d_data, d_empty, d_fold = i32(data), i32(empty), i32(fold.ravel())
        fold_cells = [i32(data[fold.ravel()[data] == f]) for f in range(5)]
        fold_grids = [f64(np.where(fold == f, np.nan, plan.grid_ns)) for f in range(5)]
        n = data.size
        d_est = torch.empty((len(models), n), dtype=torch.float64, device=dev)
        d_var = torch.empty_like(d_est)
        d_n = torch.empty(n, dtype=torch.int32, device=dev)
        eng._check(lib.gsm_sgs_set_kriging(h, 0, _ptr(d_gm)))

        flagged = []                                      # calls that reported a device-found error (they complete all the same)

        def cv(d_cells, count, d_f, tab, sill):
            rc = lib.gsm_krige_cv(h, _ptr(d_grid), _ptr(d_cells), count, _ptr(d_f), 0.0, _ptr(d_xs), _ptr(d_ys), len(sill), _ptr(tab),
                                  H - 1, W - 1, hw, radius, num_points, (C.c_double * len(sill))(*sill), _ptr(d_est), _ptr(d_var),
                                  _ptr(d_n), eng._stream())
            if rc == -5:                                  # GSM_E_DEVICE_DATA
                flagged.append(lib.gsm_last_error(h).decode())
            else:
                eng._check(rc)

        def krige(d_g, d_cells, count):
            eng._check(lib.gsm_krige_grid(h, _ptr(d_g), _ptr(d_cells), count, _ptr(d_xs), _ptr(d_ys), _ptr(d_tab1[0]), H - 1, W - 1, hw, radius,
                                          num_points, sills[0], _ptr(d_est), _ptr(d_var), _ptr(d_n), eng._stream()))

        fns = {
            "loo_1_model": lambda: cv(d_data, n, None, d_tab1[0], sills[:1]),
            "krige_grid_same_count": lambda: krige(d_grid, d_empty, n),
            "loo_4_models_one_call": lambda: cv(d_data, n, None, d_tab, sills),
            "loo_4_models_four_calls": lambda: [cv(d_data, n, None, d_tab1[m], sills[m:m + 1]) for m in range(4)],
            "folds5_one_call": lambda: cv(d_data, n, d_fold, d_tab1[0], sills[:1]),
            "folds5_five_krige_grid_calls": lambda: [krige(fold_grids[f], fold_cells[f], int(fold_cells[f].numel())) for f in range(5)],
        }
        # the runs alternate within every repeat, so that a drift of the machine touches both sides of a comparison alike
        runs = {k: [] for k in fns}
        with torch.cuda.device(dev):
            for k in range(args.repeats + 1):
                for name, fn in fns.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    torch.cuda.synchronize()
                    if k:
                        runs[name].append(e0.elapsed_time(e1))
        mean_n = float(d_n.cpu().numpy().mean())
    finally:
        eng.close()
    med = {k: float(np.median(v)) for k, v in runs.items()}
    row = {"grid": f"{H}x{W}", "targets": int(n), "num_points": num_points, "radius_m": radius, "repeats": args.repeats, "ms": runs,
           "ms_median": med,
           "targets_per_s_loo": n / (1e-3 * med["loo_1_model"]), "cells_per_s_krige_grid": n / (1e-3 * med["krige_grid_same_count"]),
           "four_calls_over_one_call": med["loo_4_models_four_calls"] / med["loo_4_models_one_call"],
           "five_krige_grid_calls_over_one_call": med["folds5_five_krige_grid_calls"] / med["folds5_one_call"],
           "mean_neighbours_last_run": mean_n, "device_data_errors": sorted(set(flagged))}
    print(json.dumps(row), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(0), "row": row}, indent=1))


if __name__ == "__main__":
    main()
