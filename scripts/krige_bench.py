"""Throughput of interpolate.krige on the device (gsm_krige_grid): estimated cells per second over a whole grid, 48 neighbours
within 50 km, Matern (the grid of scripts/sgs_grid_bench.py), with gsm_sgs_grid on the same grid and arguments in the same
process as the yardstick: its weights pass calls the same search and solve per cell (octant_ring_search and krige_solve of
csrc/sgs_search.h).

    cells_per_s_device      HIP events around gsm_krige_grid (the whole call: one kernel and the error word's read-back)
    cells_per_s_total       interpolate.krige end to end: transformer fit, lag table, uploads, device call, inverse transform
    sgs_device_ms           the gsm_sgs_grid call, --reals realisations (ranks, weights pass, value pass)
The weights pass cannot be timed from outside gsm_sgs_grid (the value pass follows it on the same stream): for the per-cell
rates of krige_grid_kernel against sgs_grid_weights_kernel run this script under `rocprofv3 --kernel-trace --stats` and
divide `cells` and `sgs_cells` by the two kernels' total times in kernel_stats.csv.

--local: the cost of a variogram per cell (gsm_krige_grid_local / gsm_sgs_grid_local: every covariance evaluated in the kernel)
against the table path.  The same problem is run twice in the same process, first with scalar parameters, then with every
parameter a constant map of the grid's shape -- with the exponential model in both runs, because the device evaluates no
Matern -- and a third line gives the ratios of the two runs' cells per second (kriging kernel; SGS call).

    python scripts/krige_bench.py [--size 566] [--reals 8] [--repeats 5] [--local] [--out profiles/krige_bench.json]
"""
import argparse
import json
import math
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "scripts"))


def device_call_ms(plan, repeats):
    """gsm_krige_grid alone, uploads outside the timed window: milliseconds of every repeat after one warm-up call."""
    import torch
    from mcmc_gpu_amd import interpolate
    from mcmc_gpu_amd.engine import GsmEngine, _ptr
    from mcmc_gpu_amd.sgs import lag_cov_table
    cells = interpolate._krige_cells(plan)
    eng = GsmEngine(plan.H, plan.W, 1)
    try:
        dev = eng.dev
        hw = int(math.ceil(plan.radius / abs(plan.dx)))
        f64 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
        d_grid, d_cells, d_xs, d_ys = f64(plan.grid_ns), torch.as_tensor(cells).to(dev), f64(plan.xs), f64(plan.ys)
        if plan.local is None:
            mi, mj = interpolate._lag_extents(plan, eng, torch)
            d_lag = f64(lag_cov_table(plan.vario, hw, plan.dx, plan.dy, mi, mj))
        else:
            d_local = f64(plan.local)
        d_gm = f64(np.full(1, plan.global_mean))
        d_est = torch.empty(cells.size, dtype=torch.float64, device=dev)
        d_var = torch.empty_like(d_est)
        d_n = torch.empty(cells.size, dtype=torch.int32, device=dev)
        eng._check(eng.lib.gsm_sgs_set_kriging(eng.h, 1 if plan.ktype == "sk" else 0, _ptr(d_gm)))
        ms = []
        for k in range(repeats + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            head = (eng.h, _ptr(d_grid), _ptr(d_cells), int(cells.size), _ptr(d_xs), _ptr(d_ys))
            if plan.local is None:
                eng._check(eng.lib.gsm_krige_grid(*head, _ptr(d_lag), mi, mj, hw, plan.radius, plan.num_points,
                                                  float(plan.vario["sill"]), _ptr(d_est), _ptr(d_var), _ptr(d_n), eng._stream()))
            else:
                eng._check(eng.lib.gsm_krige_grid_local(*head, _ptr(d_local), interpolate.LOCAL_VTYPES[plan.vtype], hw, plan.radius,
                                                        plan.num_points, _ptr(d_est), _ptr(d_var), _ptr(d_n), eng._stream()))
            e1.record()
            torch.cuda.synchronize()
            if k:
                ms.append(e0.elapsed_time(e1))
        n = d_n.cpu().numpy()
    finally:
        eng.close()
    return cells.size, ms, float(n.mean())


def measure(interpolate, torch, args, xx, yy, grid, vario, label=None):
    n, kw = args.size, dict(radius=50e3, num_points=48, ktype="ok")
    plan = interpolate._krige_plan(xx, yy, grid, vario, kw["radius"], kw["num_points"], kw["ktype"], None, None)
    cells, ms, mean_n = device_call_ms(plan, args.repeats)
    interpolate.krige(xx, yy, grid, vario, **kw)                             # warm
    t0 = time.perf_counter()
    sim, std = interpolate.krige(xx, yy, grid, vario, **kw)
    t1 = time.perf_counter()
    # the yardstick: gsm_sgs_grid, same grid, variogram, radius and num_points, no bounds
    R = args.reals
    draws = [plan.draws(np.random.default_rng(s)) for s in range(R)]
    t2 = time.perf_counter()
    [plan.draws(np.random.default_rng(s)) for s in range(R)]
    t3 = time.perf_counter()
    interpolate._run(plan, [np.random.default_rng(s) for s in range(R)])
    torch.cuda.synchronize()
    t4 = time.perf_counter()
    sgs_cells = int(sum(p.size for p, _ in draws))
    sgs_dev_s = (t4 - t3) - (t3 - t2)                                        # _run draws again on the host before its device call
    row = {"grid": f"{n}x{n}", "cells": int(cells), "mean_neighbours": mean_n, "device_ms": ms, "device_ms_median": float(np.median(ms)),
           "cells_per_s_device": cells / (1e-3 * float(np.median(ms))), "total_ms": 1e3 * (t1 - t0),
           "cells_per_s_total": cells / (t1 - t0), "nan_cells": int(np.isnan(sim).sum() + np.isnan(std).sum()),
           "sgs_realisations": R, "sgs_cells": sgs_cells, "sgs_device_ms": 1e3 * sgs_dev_s}
    if label:
        row["variogram"] = label
    print(json.dumps(row), flush=True)
    return row


def main():
    import torch
    from mcmc_gpu_amd import interpolate
    from sgs_grid_bench import problem
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=566)
    ap.add_argument("--reals", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--local", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    xx, yy, grid, vario, _ = problem(args.size)
    if not args.local:
        row = measure(interpolate, torch, args, xx, yy, grid, vario)
    else:
        scalar = {k: v for k, v in dict(vario, vtype="Exponential").items() if k != "s"}
        maps = {k: (v if k == "vtype" else np.full(grid.shape, v)) for k, v in scalar.items()}
        table = measure(interpolate, torch, args, xx, yy, grid, scalar, "exponential, scalars (lag table)")
        local = measure(interpolate, torch, args, xx, yy, grid, maps, "exponential, constant maps (per cell)")
        ratio = {"krige_local_over_table": local["cells_per_s_device"] / table["cells_per_s_device"],
                 "sgs_local_over_table": table["sgs_device_ms"] / local["sgs_device_ms"]}
        print(json.dumps(ratio), flush=True)
        row = {"table": table, "local": local, "ratio": ratio}
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(0), "row": row}, indent=1))


if __name__ == "__main__":
    main()
