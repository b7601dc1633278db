"""Cost of the local variogram maps on the device (gsm_variogram_local, csrc/variogram_local_kernel.hip) beside the global map.

Per shape, alternating in one process so that clocks and caches are shared:
    tile         gsm_variogram_local with half_window 0: the tile pass alone
    window       gsm_variogram_local with half_window k: tile pass, window pass, and the call's scratch allocation
    global       gsm_variogram_map on the same fields and extents
The three do the same pair updates (scripts/variogram_bench.py: one difference, square, addition and count per (cell, offset)
pair inside the grid; the fields hold no missing cell and the returned counts must add up to that number -- asserted for all
three, the window tables through the number of windows that hold each tile), so tile / global is the price of the tiling.
For one 566 x 566 field also
    crops        the composition that needs no new kernel: one gsm_variogram_map call per window on a cropped copy of the
                 window's cells (crops made outside the timed window, one handle per crop shape).  It counts the pairs with both
                 ends in the crop, every pair once per window that holds it, and is not the same statistic at the crop's rim.
HIP events around whole calls, uploads outside the timed window, one warm-up round; the median of `--repeats` with its range.

    566 x 566 cells x  1 field,  T 16, k 2, offsets within 25 cells
    566 x 566 cells x 64 fields, T 16, k 2, offsets within 25 cells
    256 x 256 cells x 64 fields, T 16, k 2, offsets within 25 cells

    python scripts/variogram_local_bench.py [--repeats 5] [--out profiles/variogram_local_bench.json]
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

from variogram_bench import pair_updates  # noqa: E402

SHAPES = [(566, 566, 1, 16, 2, 25, True), (566, 566, 64, 16, 2, 25, False), (256, 256, 64, 16, 2, 25, False)]


def _timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def _stats(ms, pairs):
    med = float(np.median(ms))
    return {"device_ms": ms, "device_ms_median": med, "device_ms_range": [min(ms), max(ms)], "pair_updates_per_s": pairs / (1e-3 * med)}


def shape_row(H, W, R, T, k, lag, with_crops, repeats):
    import torch
    from mcmc_gpu_amd.engine import GsmEngine, _ptr
    eng = GsmEngine(H, W, 1)
    crop_engines = {}
    try:
        dev = eng.dev
        gen = torch.Generator(device=dev).manual_seed(7)
        d_f = 300.0 + 50.0 * torch.randn((R, H, W), dtype=torch.float64, device=dev, generator=gen)
        mi = mj = min(lag, H - 1, W - 1)
        Ty, Tx = -(-H // T), -(-W // T)
        table = (mi + 1, 2 * mj + 1)
        d_s = torch.empty((R, Ty, Tx) + table, dtype=torch.float64, device=dev)
        d_c = torch.empty((R, Ty, Tx) + table, dtype=torch.int64, device=dev)
        d_gs = torch.empty((R,) + table, dtype=torch.float64, device=dev)
        d_gc = torch.empty((R,) + table, dtype=torch.int64, device=dev)
        pairs = R * pair_updates(H, W, mi, mj)
        # windows that hold each tile, per axis: the window counts must add up to pairs weighted with it
        cover = [np.array([sum(1 for w in range(n) if abs(w - t) <= k) for t in range(n)]) for n in (Ty, Tx)]

        def local(half):
            eng._check(eng.lib.gsm_variogram_local(eng.h, _ptr(d_f), R, None, mi, mj, T, half, _ptr(d_s), _ptr(d_c), eng._stream()))

        def glob():
            eng._check(eng.lib.gsm_variogram_map(eng.h, _ptr(d_f), R, None, mi, mj, 0, _ptr(d_gs), _ptr(d_gc), eng._stream()))

        crops = []
        if with_crops:
            for a in range(Ty):
                for b in range(Tx):
                    i0, i1 = max(0, a - k) * T, min(H, (a + k + 1) * T)
                    j0, j1 = max(0, b - k) * T, min(W, (b + k + 1) * T)
                    shape = (i1 - i0, j1 - j0)
                    if shape not in crop_engines:
                        crop_engines[shape] = GsmEngine(shape[0], shape[1], 1)
                    crops.append((crop_engines[shape], d_f[0, i0:i1, j0:j1].contiguous(), min(mi, shape[0] - 1), min(mj, shape[1] - 1)))
            d_ws = torch.empty((len(crops),) + table, dtype=torch.float64, device=dev)
            d_wc = torch.empty((len(crops),) + table, dtype=torch.int64, device=dev)

        def per_window():
            for n, (e, crop, ci, cj) in enumerate(crops):
                e._check(e.lib.gsm_variogram_map(e.h, _ptr(crop), 1, None, ci, cj, 0, _ptr(d_ws[n]), _ptr(d_wc[n]), eng._stream()))

        ms = {"tile": [], "window": [], "global": [], "crops": []}
        for rep in range(repeats + 1):
            t = {"tile": _timed(lambda: local(0))}
            tiles = int(d_c.sum().item())
            t["window"] = _timed(lambda: local(k))
            in_windows = int(d_c.sum().item())
            t["global"] = _timed(glob)
            assert tiles == pairs == int(d_gc.sum().item()), (tiles, pairs)
            if rep == 0:                                             # the windows' counts: every tile's pairs once per window that holds it
                local(0)
                torch.cuda.synchronize()
                tile_pairs = d_c.sum(dim=(0, 3, 4)).cpu().numpy()
                assert in_windows == int((tile_pairs * cover[0][:, None] * cover[1][None, :]).sum())
            if with_crops:
                t["crops"] = _timed(per_window)
            if rep:
                for key, v in t.items():
                    ms[key].append(v)
    finally:
        for e in crop_engines.values():
            e.close()
        eng.close()
    row = {"grid": f"{H}x{W}", "fields": R, "tile": T, "half_window": k, "mi": mi, "mj": mj, "tiles": [Ty, Tx], "pair_updates": pairs,
           "tile_pass": _stats(ms["tile"], pairs), "tile_and_window_pass": _stats(ms["window"], pairs), "global_map": _stats(ms["global"], pairs)}
    row["tile_pass_over_global_map"] = row["tile_pass"]["device_ms_median"] / row["global_map"]["device_ms_median"]
    row["tile_and_window_over_global_map"] = row["tile_and_window_pass"]["device_ms_median"] / row["global_map"]["device_ms_median"]
    if with_crops:
        crop_pairs = sum(pair_updates(c.shape[0], c.shape[1], ci, cj) for _, c, ci, cj in crops)
        row["global_map_per_cropped_window"] = dict(_stats(ms["crops"], crop_pairs), calls=len(crops), pair_updates=crop_pairs)
        row["cropped_windows_over_tile_and_window"] = (row["global_map_per_cropped_window"]["device_ms_median"] /
                                                       row["tile_and_window_pass"]["device_ms_median"])
    return row


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []
    for shape in SHAPES:
        rows.append(shape_row(*shape, args.repeats))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(0), "rows": rows}, indent=1))


if __name__ == "__main__":
    main()
