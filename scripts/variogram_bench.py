"""Throughput of the variogram map on the device (gsm_variogram_map, csrc/variogram_kernel.hip): pair updates per second.

A pair update is one (cell, offset) pair with both cells inside the grid: one difference, one square, one addition and one
count.  Their number follows from the shapes -- sum over the offsets (di, dj) of the half plane of (H - di) (W - |dj|) -- and
the fields hold no missing cell, so the counts the device returns must add up to it (asserted).  HIP events around the whole
call (the pair kernel and, when the rows are split into parts, the kernel that adds the parts), uploads outside the timed
window, one warm-up call; the median of `--repeats` calls is reported with the range.

    256 x 256 cells x 1024 fields, offsets within 50 cells     the beds of 1024 chains
    566 x 566 cells x   64 fields, offsets within 50 cells     realisations on the grid of scripts/sgs_grid_bench.py

    python scripts/variogram_bench.py [--repeats 5] [--rows-per-part 0] [--out profiles/variogram_bench.json]
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SHAPES = [(256, 256, 1024, 50), (566, 566, 64, 50)]


def pair_updates(H, W, mi, mj):
    di, dj = np.meshgrid(np.arange(mi + 1), np.arange(-mj, mj + 1), indexing="ij")
    n = (H - di) * (W - np.abs(dj))
    n[(di == 0) & (dj <= 0)] = 0
    return int(n.sum())


def shape_row(H, W, R, lag, repeats, rows_per_part):
    import torch
    from mcmc_gpu_amd.engine import GsmEngine, _ptr
    eng = GsmEngine(H, W, 1)
    try:
        dev = eng.dev
        gen = torch.Generator(device=dev).manual_seed(7)
        d_f = 300.0 + 50.0 * torch.randn((R, H, W), dtype=torch.float64, device=dev, generator=gen)
        mi = mj = min(lag, H - 1, W - 1)
        d_s = torch.empty((R, mi + 1, 2 * mj + 1), dtype=torch.float64, device=dev)
        d_c = torch.empty((R, mi + 1, 2 * mj + 1), dtype=torch.int64, device=dev)
        ms = []
        for k in range(repeats + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            eng._check(eng.lib.gsm_variogram_map(eng.h, _ptr(d_f), R, None, mi, mj, rows_per_part, _ptr(d_s), _ptr(d_c), eng._stream()))
            e1.record()
            torch.cuda.synchronize()
            if k:
                ms.append(e0.elapsed_time(e1))
        counted = int(d_c.sum().item())
    finally:
        eng.close()
    pairs = R * pair_updates(H, W, mi, mj)
    assert counted == pairs, (counted, pairs)
    med = float(np.median(ms))
    return {"grid": f"{H}x{W}", "fields": R, "mi": mi, "mj": mj, "rows_per_part": rows_per_part, "pair_updates": pairs, "device_ms": ms,
            "device_ms_median": med, "pair_updates_per_s": pairs / (1e-3 * med),
            "pair_updates_per_s_range": [pairs / (1e-3 * max(ms)), pairs / (1e-3 * min(ms))]}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rows-per-part", type=int, default=0, help="0 = the library's default split")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []
    for H, W, R, lag in SHAPES:
        rows.append(shape_row(H, W, R, lag, args.repeats, args.rows_per_part))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(0), "rows": rows}, indent=1))


if __name__ == "__main__":
    main()
