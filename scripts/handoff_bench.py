"""The join between the two samplers, measured on one device: the trend of a stack of beds (gsm_gaussian_filter) and the small-scale
chain with chain groups (run_many_sgs(groups=)).  Medians of `--repeats` (>= 7) measurements, the sides of a comparison taken in turn
within every repeat; the ranges are kept in the JSON.

  (a) gsm_gaussian_filter at 1024 x 256^2 and 64 x 566^2, sigma = 10 (81 taps per axis), HIP events around whole calls, beside
        - gsm_debug_stream_copy of the bytes the two passes must move: four planes (x read, the axis-0 result written and read, out
          written) = two stream copies of one plane-stack each, inside one pair of events;
        - scipy.ndimage.gaussian_filter on the host for the same stack, wall clock, with the download of the beds and the upload of
          the trends that the host path costs a caller whose beds are on the device.
  (b) the small-scale chain at the driver's configuration (64^2, pcg64 draws, the set-up of scripts/sgs_bench.py), wall clock of whole
      run_many_sgs calls after a warm-up call:
        - 256 chains without groups;
        - 256 chains in 64 groups of 4 (sgs.handoff of 64 beds);
        - the same 64 groups as 64 separate 4-chain calls, each on a template with its group's trend and transformer.
  (c) --parent-tree DIR (a checkout of the parent commit with its library built): scripts/sgs_bench.py --pcg64 at 256 and at 4 chains,
      run from DIR and from this tree in turn, each in a fresh process; the rates printed by the script.

  (d) --fit: the normal-score transformers of the same two stacks, 1000 quantiles (profiles/handoff_bench_fit.json):
        - gsm_qt_fit, HIP events around whole calls, beside
        - gsm_debug_stream_copy of one plane-stack: the bytes one read and one write of the keys move (the sort makes
          2 + ceil(log2(cells / 4096)) such passes and a read);
        - the scikit-learn loop on the host, QuantileTransformer(1000, subsample=None).fit per field, wall clock, arrays already there;
        - sgs.handoff(fit='device') against sgs.handoff(fit='host') on those stacks as beds, wall clock of whole calls (clamp, trend,
          transformers; the trend on the device in both).

    python scripts/handoff_bench.py [--repeats 7] [--iters 2000] [--skip-host] [--parent-tree DIR] [--out profiles/handoff_bench.json]
    python scripts/handoff_bench.py --fit --skip-filter --skip-chain --out profiles/handoff_bench_fit.json
"""
import argparse
import json
import re
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

FILTER_SHAPES = [(1024, 256, 256), (64, 566, 566)]


def _summary(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "all": [float(x) for x in v]}


def filter_rows(repeats, skip_host):
    import ctypes as C
    import torch
    from scipy.ndimage import gaussian_filter
    from mcmc_gpu_amd import sgs
    from mcmc_gpu_amd.engine import GsmEngine, _ptr
    rows = []
    for n, H, W in FILTER_SHAPES:
        eng = GsmEngine(H, W, 1)
        try:
            dev = eng.dev
            gen = torch.Generator(device=dev).manual_seed(3)
            x = 300.0 + 50.0 * torch.randn((n, H, W), dtype=torch.float64, device=dev, generator=gen)
            out, b = torch.empty_like(x), torch.empty_like(x)
            w = np.ascontiguousarray(sgs.gaussian_weights(10))
            wp, lw, m = w.ctypes.data_as(C.POINTER(C.c_double)), w.size // 2, x.numel()

            def timed(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); fn(); e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1)

            def filt():
                eng._check(eng.lib.gsm_gaussian_filter(eng.h, _ptr(x), _ptr(out), n, H, W, wp, lw, wp, lw, eng._stream()))

            def copy4():
                eng._check(eng.lib.gsm_debug_stream_copy(_ptr(x), _ptr(b), m, eng._stream()))
                eng._check(eng.lib.gsm_debug_stream_copy(_ptr(b), _ptr(out), m, eng._stream()))

            def host():
                t0 = time.perf_counter()
                xh = x.cpu().numpy()
                th = np.stack([gaussian_filter(f, sigma=10) for f in xh])
                torch.as_tensor(th).to(dev)
                torch.cuda.synchronize()
                return 1e3 * (time.perf_counter() - t0)

            timed(copy4); timed(filt)                          # warm-up: first launches, the handle's scratch
            t_f, t_c, t_h = [], [], []
            for _ in range(repeats):
                t_f.append(timed(filt)); t_c.append(timed(copy4))
                if not skip_host:
                    t_h.append(host())
            timed(filt)                                        # the last copy overwrote `out`
            # the device's result against scipy on the first field (the tests hold it to its bar; here only that the call did its work)
            err = float(np.abs(out[0].cpu().numpy() - gaussian_filter(x[0].cpu().numpy(), sigma=10)).max())
        finally:
            eng.close()
        plane_bytes = 8 * m
        row = {"fields": n, "grid": f"{H}x{W}", "sigma": 10, "taps": int(w.size), "filter_ms": _summary(t_f), "copy_four_planes_ms": _summary(t_c),
               "filter_over_copy": float(np.median(t_f) / np.median(t_c)), "copy_TB_per_s": 4 * plane_bytes / (1e-3 * np.median(t_c)) / 1e12,
               "filter_effective_TB_per_s": 4 * plane_bytes / (1e-3 * np.median(t_f)) / 1e12,
               "multiply_adds_per_s": 2.0 * w.size * m / (1e-3 * np.median(t_f)), "max_abs_diff_to_scipy_field0": err}
        if t_h:
            row.update(host_scipy_with_copies_ms=_summary(t_h), host_over_filter=float(np.median(t_h) / np.median(t_f)))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def fit_rows(repeats, skip_host):
    import torch
    from sklearn.preprocessing import QuantileTransformer
    from mcmc_gpu_amd import sgs, synthetic
    from mcmc_gpu_amd.engine import GsmEngine, _ptr
    nq = 1000
    rows = []
    for n, H, W in FILTER_SHAPES:
        eng = GsmEngine(H, W, 1)
        try:
            dev = eng.dev
            gen = torch.Generator(device=dev).manual_seed(5)
            x = 40.0 * torch.randn((n, H * W), dtype=torch.float64, device=dev, generator=gen)
            b = torch.empty_like(x)
            q = sgs.quantile_probabilities(nq)

            def timed(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); out = fn(); e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1), out

            fit = lambda: eng.qt_fit(x, q)
            copy = lambda: eng._check(eng.lib.gsm_debug_stream_copy(_ptr(x), _ptr(b), x.numel(), eng._stream()))
            timed(copy); timed(fit)                            # warm-up: first launches, the handle's key buffers
            xh = x.cpu().numpy()

            def host():
                t0 = time.perf_counter()
                fits = [QuantileTransformer(n_quantiles=nq, output_distribution="normal", subsample=None, random_state=0).fit(f.reshape(-1, 1))
                        for f in xh]
                return 1e3 * (time.perf_counter() - t0), fits

            t_f, t_c, t_h, tables, fits = [], [], [], None, None
            for _ in range(repeats):
                t, out = timed(fit); t_f.append(t); tables = out[0]
                t_c.append(timed(copy)[0])
                if not skip_host:
                    t, fits = host(); t_h.append(t)
        finally:
            eng.close()
        row = {"fields": n, "grid": f"{H}x{W}", "n_quantiles": nq, "merge_passes": int(np.ceil(np.log2(np.ceil(H * W / 4096)))),
               "qt_fit_ms": _summary(t_f), "copy_one_plane_stack_ms": _summary(t_c), "fit_over_copy": float(np.median(t_f) / np.median(t_c)),
               "copy_TB_per_s": 16 * x.numel() / (1e-3 * np.median(t_c)) / 1e12, "keys_per_s": x.numel() / (1e-3 * np.median(t_f))}
        if t_h:
            tab = tables.cpu().numpy()
            row.update(host_sklearn_loop_ms=_summary(t_h), host_over_fit=float(np.median(t_h) / np.median(t_f)),
                       tables_equal_sklearn=bool(all(np.array_equal(tab[r], fits[r].quantiles_[:, 0]) for r in range(n))))
        # whole hand-offs: the stack as large-scale beds of a template on this grid (H == W)
        del x, b
        torch.cuda.empty_cache()
        _, ch = synthetic.sgs_template(H)
        lsc = np.asarray(ch.surf)[None] - 300.0 + xh.reshape(n, H, W)
        of = np.arange(n)
        sides = {"device": [], "host": []}
        sgs.handoff(ch, lsc[:2], of[:2], fit="device")          # warm-up
        for _ in range(repeats):
            for side in (("device",) if skip_host else ("device", "host")):
                t0 = time.perf_counter()
                sgs.handoff(ch, lsc, of, sigma=10, n_quantiles=nq, random_state=0, fit=side)
                sides[side].append(1e3 * (time.perf_counter() - t0))
        row["handoff_fit_device_ms"] = _summary(sides["device"])
        if sides["host"]:
            row.update(handoff_fit_host_ms=_summary(sides["host"]),
                       handoff_host_over_device=float(np.median(sides["host"]) / np.median(sides["device"])))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def chain_rows(repeats, iters):
    from mcmc_gpu_amd import sgs, synthetic
    H, n_groups, per = 64, 64, 4
    n = n_groups * per
    prob, ch = synthetic.sgs_template(H)
    beds = [prob["bed"] + np.random.default_rng(40 + i).normal(0, 3, prob["bed"].shape) for i in range(n)]
    lsc = np.stack([prob["bed"] + np.random.default_rng(2000 + g).normal(0, 3, prob["bed"].shape) for g in range(n_groups)])
    of = np.repeat(np.arange(n_groups), per)
    t0 = time.perf_counter()
    g_beds, groups = sgs.handoff(ch, lsc, of, sigma=10, n_quantiles=1000, random_state=0)
    t_handoff = time.perf_counter() - t0
    templates = []
    for g in range(n_groups):
        _, t = synthetic.sgs_template(H)
        t.set_trend(groups["trend"][g], detrend_map=True)
        t.set_normal_transformation(groups["nst_trans"][g], do_transform=True)
        templates.append(t)
    rngs = lambda idx: [np.random.default_rng(900 + int(i)) for i in idx]

    def plain():
        t0 = time.perf_counter()
        sgs.run_many_sgs(ch, beds, rngs(range(n)), iters, pcg64=True)
        return n * iters / (time.perf_counter() - t0)

    def grouped():
        t0 = time.perf_counter()
        sgs.run_many_sgs(ch, g_beds, rngs(range(n)), iters, pcg64=True, groups=groups)
        return n * iters / (time.perf_counter() - t0)

    def separate():
        t0 = time.perf_counter()
        for g in range(n_groups):
            idx = range(g * per, (g + 1) * per)
            sgs.run_many_sgs(templates[g], [g_beds[i] for i in idx], rngs(idx), iters, pcg64=True)
        return n * iters / (time.perf_counter() - t0)

    sgs.run_many_sgs(ch, beds[:4], rngs(range(4)), 20, pcg64=True)          # warm-up (library load, first launches)
    r_p, r_g, r_s = [], [], []
    for _ in range(repeats):
        r_p.append(plain()); r_g.append(grouped()); r_s.append(separate())
    row = {"grid": f"{H}x{H}", "draws": "pcg64", "iterations": iters, "handoff_of_64_beds_s": t_handoff,
           "chain_iterations_per_s": {"256_chains_no_groups": _summary(r_p), "256_chains_in_64_groups_of_4": _summary(r_g),
                                      "64_separate_runs_of_4_chains": _summary(r_s)},
           "grouped_over_ungrouped": float(np.median(r_g) / np.median(r_p)), "grouped_over_separate": float(np.median(r_g) / np.median(r_s))}
    print(json.dumps(row), flush=True)
    return row


def parent_rows(parent, repeats, iters):
    """scripts/sgs_bench.py --pcg64 from the parent's tree and from this one in turn, a fresh process each"""
    rows = {}
    for chains in (256, 4):
        rates = {"parent": [], "this": []}
        for _ in range(repeats):
            for tag, tree in (("parent", Path(parent)), ("this", ROOT)):
                r = subprocess.run([sys.executable, "scripts/sgs_bench.py", "--pcg64", "--chains", str(chains), "--iters", str(iters)], cwd=str(tree),
                                   capture_output=True, text=True, timeout=600)
                m = re.search(r"= (\d+) chain-iterations/s", r.stdout)
                if r.returncode != 0 or not m:
                    raise RuntimeError(f"sgs_bench in {tree} failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
                rates[tag].append(float(m.group(1)))
        rows[f"{chains}_chains"] = {"parent": _summary(rates["parent"]), "this": _summary(rates["this"]),
                                    "this_over_parent": float(np.median(rates["this"]) / np.median(rates["parent"]))}
        print(json.dumps({f"{chains}_chains": rows[f"{chains}_chains"]}), flush=True)
    return rows


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=2000, help="iterations per chain in (b): the set-up of a call (per group: the conditioning data through its transformer on the host) is in the wall time")
    ap.add_argument("--skip-host", action="store_true", help="leave scipy on the host out of (a)")
    ap.add_argument("--skip-chain", action="store_true", help="leave (b) out")
    ap.add_argument("--skip-filter", action="store_true", help="leave (a) out")
    ap.add_argument("--fit", action="store_true", help="add (d): gsm_qt_fit beside a stream copy, the scikit-learn loop and whole hand-offs")
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built: adds (c)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.repeats < 7:
        ap.error("--repeats must be at least 7")
    res = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats}
    if not args.skip_filter:
        res["filter"] = filter_rows(args.repeats, args.skip_host)
    if args.fit:
        res["fit"] = fit_rows(args.repeats, args.skip_host)
    if not args.skip_chain:
        res["chain"] = chain_rows(args.repeats, args.iters)
    if args.parent_tree:
        res["ungrouped_parent_against_this"] = parent_rows(args.parent_tree, args.repeats, max(args.iters, 1000))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
