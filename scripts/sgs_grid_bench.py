"""Throughput of interpolate.sgs_many on the device (gsm_sgs_grid): simulated cells per second over whole grids, 48 neighbours
within 50 km, Matern, bounds on (T2_StatisticalAnalysis.ipynb's call), split into the host draw plan, the device call (weights
and values; per-kernel times: run under rocprofv3 --kernel-trace --stats) and the inverse transform.

--local: the cost of a variogram per cell (gsm_sgs_grid_local: every covariance evaluated in the kernel) against the table path.
The same problem is run twice in the same process, first with scalar parameters, then with every parameter a constant map of
the grid's shape -- with the exponential model in both runs, because the device evaluates no Matern -- and a third line gives
local_over_table, the ratio of the two cells_per_s_device.

--mode pcg64: the shuffle and the draws on the device (gsm_sgs_grid_draw_pcg64) beside the host's.  Every row keeps draw_plan_ms
(the host draws) and device_ms (the SGS call in the default mode, as without the option) and adds draw_device_ms -- the new entry
alone on buffers made beforehand, the host clock around a synchronise, warmed up, median of 5 --, pcg64_ms (the whole _run call in
mode 'pcg64': uploads, draws, SGS, download), cells_per_s_total of the pcg64 path (fit + pcg64_ms + inverse transform; the default
mode's figure moves to cells_per_s_total_replay) and equal_to_replay (the two modes' grids compared bit for bit).

    python scripts/sgs_grid_bench.py [--sizes 256,566] [--reals 10,64] [--local] [--mode pcg64] [--out profiles/sgs_grid_bench.json]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def problem(n):
    import interp_sgs_common as ic
    xx, yy = np.meshgrid(np.arange(n) * 500.0, np.arange(n) * 500.0)
    bed = ic.field(n, n, 3)
    cond = np.zeros((n, n), bool)
    cond[::10, :] = True                                      # flight lines 5 km apart, crossing lines every 7.5 km
    cond[:, ::15] = True
    grid = np.where(cond, bed, np.nan)
    vario = dict(major_range=30e3, minor_range=30e3, azimuth=0.0, sill=1.0, nugget=0.0, vtype="Matern", s=1.5)
    bounds = (float(np.nanmin(grid)) - 200.0, bed + 500.0)
    return xx, yy, grid, vario, bounds


def time_draw_entry(interpolate, torch, plan, R, repeats=5):
    """Milliseconds of one gsm_sgs_grid_draw_pcg64 call for R realisations (median of `repeats` after a warm-up call)."""
    from mcmc_gpu_amd.engine import GsmEngine, _ptr
    eng = GsmEngine(plan.H, plan.W, R)
    try:
        dev = eng.dev
        flat = np.ascontiguousarray(plan.inds[:, 0] * plan.W + plan.inds[:, 1], dtype=np.int32)
        path_len = int(np.count_nonzero(~plan.cond.ravel()[flat]))
        states = torch.as_tensor(GsmEngine.pack_pcg64_states([np.random.default_rng(s) for s in range(R)]).view(np.int64)).to(dev)
        cells, has = torch.as_tensor(flat).to(dev), torch.as_tensor(plan.cond.astype(np.uint8).ravel()).to(dev)
        lo = hi = None
        if plan.bounds is not None:
            lo, hi = (torch.as_tensor(b).to(dev) for b in plan.bounds)
        work = torch.empty(max(1, R * flat.size), dtype=torch.int32, device=dev)
        path = torch.empty(max(1, R * path_len), dtype=torch.int32, device=dev)
        draws = torch.empty(max(1, R * path_len), dtype=torch.float64, device=dev)
        times = []
        for _ in range(repeats + 1):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            with torch.cuda.device(dev):
                eng._check(eng.lib.gsm_sgs_grid_draw_pcg64(eng.h, _ptr(states), _ptr(cells), int(flat.size), _ptr(has), _ptr(lo), _ptr(hi),
                                                           0 if lo is None else 1, _ptr(work), _ptr(path), _ptr(draws), path_len,
                                                           eng._stream()))
            torch.cuda.synchronize(dev)
            times.append(1e3 * (time.perf_counter() - t0))
        return float(np.median(times[1:]))
    finally:
        eng.close()


def measure(interpolate, torch, n, R, xx, yy, grid, vario, bounds, label=None, mode="replay"):
    t0 = time.perf_counter()
    plan = interpolate._Plan(xx, yy, grid, vario, 50e3, 48, "ok", None, None, None, bounds)
    t1 = time.perf_counter()
    gens = [np.random.default_rng(s) for s in range(R)]
    draws = [plan.draws(np.random.default_rng(s)) for s in range(R)]
    t2 = time.perf_counter()
    ns, _ = interpolate._run(plan, gens)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    out = interpolate._inverse(plan, ns)
    t4 = time.perf_counter()
    cells = int(sum(p.size for p, _ in draws))
    dev_s = (t3 - t2) - (t2 - t1)                             # _run draws again on the host before its device call
    row = {"grid": f"{n}x{n}", "realisations": R, "simulated_cells": cells, "fit_ms": 1e3 * (t1 - t0),
           "draw_plan_ms": 1e3 * (t2 - t1), "device_ms": 1e3 * dev_s, "inverse_transform_ms": 1e3 * (t4 - t3),
           "cells_per_s_device": cells / dev_s, "cells_per_s_total": cells / (t4 - t0 - (t2 - t1)),
           "nan_cells": int(np.isnan(out).sum())}
    if label:
        row["variogram"] = label
    if mode == "pcg64":
        row["draw_device_ms"] = time_draw_entry(interpolate, torch, plan, R)
        t5 = time.perf_counter()
        ns_dev, _ = interpolate._run(plan, [np.random.default_rng(s) for s in range(R)], mode="pcg64")
        torch.cuda.synchronize()
        t6 = time.perf_counter()
        row["pcg64_ms"] = 1e3 * (t6 - t5)
        row["cells_per_s_total_replay"] = row["cells_per_s_total"]
        row["cells_per_s_total"] = cells / ((t1 - t0) + (t6 - t5) + (t4 - t3))
        row["equal_to_replay"] = bool(np.array_equal(ns_dev, ns, equal_nan=True))
        row["mode"] = "pcg64"
    print(json.dumps(row), flush=True)
    return row


def main():
    import torch
    from mcmc_gpu_amd import interpolate
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,566")
    ap.add_argument("--reals", default="10,64")
    ap.add_argument("--local", action="store_true")
    ap.add_argument("--mode", choices=["replay", "pcg64"], default="replay")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []
    for n in [int(s) for s in args.sizes.split(",")]:
        xx, yy, grid, vario, bounds = problem(n)
        for R in [int(s) for s in args.reals.split(",")]:
            if not args.local:
                rows.append(measure(interpolate, torch, n, R, xx, yy, grid, vario, bounds, mode=args.mode))
                continue
            scalar = {k: v for k, v in dict(vario, vtype="Exponential").items() if k != "s"}
            maps = {k: (v if k == "vtype" else np.full(grid.shape, v)) for k, v in scalar.items()}
            table = measure(interpolate, torch, n, R, xx, yy, grid, scalar, bounds, "exponential, scalars (lag table)", args.mode)
            local = measure(interpolate, torch, n, R, xx, yy, grid, maps, bounds, "exponential, constant maps (per cell)", args.mode)
            ratio = {"grid": f"{n}x{n}", "realisations": R, "local_over_table": local["cells_per_s_device"] / table["cells_per_s_device"]}
            print(json.dumps(ratio), flush=True)
            rows += [table, local, ratio]
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(0), "rows": rows}, indent=1))


if __name__ == "__main__":
    main()
