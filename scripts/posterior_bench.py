"""Cost of the posterior accumulator (mcmc_gpu_amd/posterior.py) on the device.

  kernels     bytes/s of one snapshot: the per-chain accumulate (48 B per chain-cell with fp64 state: 8 bed, 8 ref, 16 read and
              16 written of the sums; 40 B with fp32 state) and the pooled form (its 8 / 4 B per chain-cell), each against
              gsm_debug_stream_copy moving the same number of bytes in the same process.  Device events around `reps` calls,
              after a warm-up; the median and the range are reported.  The bytes are what the algorithm needs, from the shapes.
  end to end  wall time of MCMC_gpu.run_many (Philox mode, results left on the device) without `posterior` and with it at
              several `thin`, rhat on and off: the overhead per snapshot.  The configurations alternate within each repeat.
  --hist      only the histogram pass (gsm_posterior_histogram, 64 bins, 2 levels) at 1024 chains of 256 x 256, fp64 and fp32
              state: time per snapshot beside the pooled form and the stream copy of the same bytes, timed in the same process,
              and its ratio to the pooled form.  The beds are N(g, 1) and the histogram spans g +- 4, so that a part of 256
              chains fills about fifty bins of every cell: nearly every counter is flushed.  Counted bytes: the beds alone.
  --ess       only the lagged pass (gsm_posterior_lagged) at 1024 chains of 256 x 256, 7 and 15 lags, fp64 and fp32 state, ring
              full: time per snapshot beside gsm_debug_stream_copy moving the same bytes, (K + 2) state values per chain-cell
              (K + 1 read, 1 written), and beside the pooled pass and ITS stream copy, all timed in the same process; then the
              wall time of MCMC_gpu.run_many without `posterior`, with it, and with `ess` (7 and 15 lags) at thin=100.
  --cov K     only the two covariance passes (gsm_posterior_project, gsm_posterior_cross) with K probes at 1024 chains of 256 x 256,
              fp64 and fp32 state: time per snapshot of each beside gsm_debug_stream_copy moving the same bytes and beside the
              pooled pass and ITS stream copy, all timed in the same process; then the wall time of MCMC_gpu.run_many without
              `posterior`, with it, and with `cov` (K Gaussian probes) at thin=100.  Counted bytes.  project: the beds, and g and
              the probes once (every chain re-reads them from the caches: `cache_bytes` is that traffic).  cross: the beds, every
              part's [K, H, W] slab written and read back, `cross` read and written, and the projections.  The default --out is
              profiles/posterior_bench_cov.json.

  --residual  only the fused residual pass (gsm_posterior_residual, 2 levels) at 1024 chains of 256 x 256, fp64 and fp32 state: (a) the
              pass, (b) the pooled pass of the same run, (c) gsm_debug_stream_copy moving the bytes the pass must move (the state once,
              the slabs and the planes) and (d), fp64 state only, the composition of existing entry points -- gsm_residual into a
              scratch array of the state's size, then gsm_posterior_accumulate_pooled on that scratch (three state-sized transfers).
              Each the median of 20 calls, three repeats, the four alternating; then the wall time of MCMC_gpu.run_many without
              `posterior`, with it, and with `residual` at thin=100 (--no-end-to-end leaves that out).  The default --out is
              profiles/posterior_bench_residual.json.

  --local R [R ...]  only the pass of the covariance with the neighbours (gsm_posterior_local) at 1024 chains of 256 x 256, for every reach
              given (1 2 4 for the published table), fp64 and fp32 state: (a) the pass, (b) gsm_debug_stream_copy moving the beds'
              bytes and (c) the composition that needs no new kernel, in torch on the same beds: d = beds - g once, then for each of
              the K = 2 R^2 + 2 R offsets a sliced multiply and a sum over the chains added to that offset's plane (the beds are read K
              times over).  (a) and (b) are the median of 20 calls, (c) of 5, three repeats, the three alternating; then the wall
              time of MCMC_gpu.run_many without `posterior`, with it, and with `local` at every reach given, at thin=100
              (--no-end-to-end leaves that out).  Counted bytes of (a): the beds, every part's [K, H, W] slab written and read back,
              `cross` read and written.  The default --out is profiles/posterior_bench_local.json.

  --regions K [--hyps B]  only the pass of the region functionals (gsm_posterior_regions) with K regions (the whole domain and K - 1
              overlapping rectangles) and B hypsometry bins at 1024 chains of 256 x 256, fp64 and fp32 state: (a) the pass, (b)
              gsm_debug_stream_copy moving the beds' bytes, (c) gsm_posterior_project with K probes and (d) the composition that needs no
              new kernel, torch clamp and masked sums, counts, amin and amax over the same beds (without the hypsometry).  (a), (b), (c)
              the median of 20 calls, (d) of 5, three repeats, the four alternating; then the wall time of MCMC_gpu.run_many without
              `posterior`, with it, and with `regions` at thin=100 (--no-end-to-end leaves that out).  Counted bytes: the beds alone.
              The default --out is profiles/posterior_bench_regions.json.

    python scripts/posterior_bench.py [--out profiles/posterior_bench.json] [--quick] [--hist | --ess | --cov K | --residual | --local R ... |
                                      --regions K [--hyps B]]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def _timed(fn, reps, warmup=3):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def _rate(name, nbytes, ms):
    med = statistics.median(ms)
    return {"what": name, "bytes": int(nbytes), "ms_median": med, "ms_min": min(ms), "ms_max": max(ms), "reps": len(ms),
            "TB_per_s_median": nbytes / med / 1e9, "TB_per_s_range": [nbytes / max(ms) / 1e9, nbytes / min(ms) / 1e9]}


def kernel_rows(n_chains, H, W, state, reps):
    import ctypes as C
    import torch
    from mcmc_gpu_amd.engine import GsmEngine
    eng = GsmEngine(H, W, n_chains, state_dtype=state)
    rows = []
    try:
        dev, n, sb = eng.dev, n_chains * H * W, 8 if state == "f64" else 4
        eng.beds = (1000.0 + torch.randn((n_chains, H, W), dtype=torch.float64, device=dev)).to(eng.state_dtype)
        ref = torch.empty_like(eng.beds)
        s1 = torch.zeros(n, dtype=torch.float64, device=dev)
        s2 = torch.zeros(n, dtype=torch.float64, device=dev)
        eng.posterior_accumulate(ref, s1, s2, True)
        per_chain = (2 * sb + 32) * n
        acc = _rate(f"accumulate {n_chains}x{H}x{W} {state}", per_chain, _timed(lambda: eng.posterior_accumulate(ref, s1, s2, False), reps))

        def copy_row(nbytes, label):
            m = nbytes // 16                                   # doubles: 8 B read + 8 B written each
            src = torch.ones(m, dtype=torch.float64, device=dev)
            dst = torch.empty(m, dtype=torch.float64, device=dev)
            st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            r = _rate(label, 16 * m, _timed(lambda: eng._check(eng.lib.gsm_debug_stream_copy(C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), m, st)), reps))
            del src, dst
            return r

        cp = copy_row(per_chain, f"stream copy of the accumulate's bytes ({n_chains}x{H}x{W} {state})")
        acc["fraction_of_copy"] = acc["TB_per_s_median"] / cp["TB_per_s_median"]
        rows += [acc, cp]
        del ref, s1, s2
        g = torch.full((H, W), 1000.0, dtype=torch.float64, device=dev)
        p1 = torch.zeros((H, W), dtype=torch.float64, device=dev)
        p2 = torch.zeros((H, W), dtype=torch.float64, device=dev)
        pooled = sb * n
        po = _rate(f"pooled accumulate {n_chains}x{H}x{W} {state}", pooled, _timed(lambda: eng.posterior_accumulate_pooled(g, p1, p2), reps))
        cp2 = copy_row(pooled, f"stream copy of the pooled form's bytes ({n_chains}x{H}x{W} {state})")
        po["fraction_of_copy"] = po["TB_per_s_median"] / cp2["TB_per_s_median"]
        rows += [po, cp2]
    finally:
        eng.close()
    for r in rows:
        print(json.dumps(r), flush=True)
    return rows


def hist_rows(n_chains, H, W, state, reps, bins=64, levels=(1000.0, 999.0)):
    import ctypes as C
    import torch
    from mcmc_gpu_amd.engine import GsmEngine
    eng = GsmEngine(H, W, n_chains, state_dtype=state)
    try:
        dev, n, sb = eng.dev, n_chains * H * W, 8 if state == "f64" else 4
        eng.beds = (1000.0 + torch.randn((n_chains, H, W), dtype=torch.float64, device=dev)).to(eng.state_dtype)
        g = torch.full((H, W), 1000.0, dtype=torch.float64, device=dev)
        p1 = torch.zeros((H, W), dtype=torch.float64, device=dev)
        p2 = torch.zeros((H, W), dtype=torch.float64, device=dev)
        counts = torch.zeros((bins + 3 + len(levels), H, W), dtype=torch.int32, device=dev)
        shape = f"{n_chains}x{H}x{W} {state}"
        po = _rate(f"pooled accumulate {shape}", sb * n, _timed(lambda: eng.posterior_accumulate_pooled(g, p1, p2), reps))
        m = sb * n // 16
        src = torch.ones(m, dtype=torch.float64, device=dev)
        dst = torch.empty(m, dtype=torch.float64, device=dev)
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        cp = _rate(f"stream copy of the beds' bytes ({shape})", 16 * m,
                   _timed(lambda: eng._check(eng.lib.gsm_debug_stream_copy(C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), m, st)), reps))
        inv_w = bins / (2 * 4.0)
        hi = _rate(f"histogram {bins} bins {len(levels)} levels {shape}", sb * n,
                   _timed(lambda: eng.posterior_histogram(g, inv_w, bins, levels, counts), reps))
        hi["ms_per_snapshot"] = hi["ms_median"]
        hi["ratio_to_pooled"] = hi["ms_median"] / po["ms_median"]
        hi["fraction_of_copy"] = hi["TB_per_s_median"] / cp["TB_per_s_median"]
        calls = 3 + reps
        hi["counts_check"] = bool((counts[:bins + 3].sum(dim=0) == calls * n_chains).all().item())
        rows = [po, cp, hi]
    finally:
        eng.close()
    for r in rows:
        print(json.dumps(r), flush=True)
    return rows


def ess_rows(n_chains, H, W, state, lags, reps):
    import ctypes as C
    import torch
    from mcmc_gpu_amd.engine import GsmEngine
    eng = GsmEngine(H, W, n_chains, state_dtype=state)
    rows = []
    try:
        dev, n, sb = eng.dev, n_chains * H * W, 8 if state == "f64" else 4
        eng.beds = (1000.0 + torch.randn((n_chains, H, W), dtype=torch.float64, device=dev)).to(eng.state_dtype)
        shape = f"{n_chains}x{H}x{W} {state}"
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def copy_row(nbytes, label):
            m = nbytes // 16                                   # doubles: 8 B read + 8 B written each
            src = torch.ones(m, dtype=torch.float64, device=dev)
            dst = torch.empty(m, dtype=torch.float64, device=dev)
            r = _rate(label, 16 * m, _timed(lambda: eng._check(eng.lib.gsm_debug_stream_copy(C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), m, st)), reps))
            del src, dst
            return r

        g = torch.full((H, W), 1000.0, dtype=torch.float64, device=dev)
        p1 = torch.zeros((H, W), dtype=torch.float64, device=dev)
        p2 = torch.zeros((H, W), dtype=torch.float64, device=dev)
        po = _rate(f"pooled accumulate {shape}", sb * n, _timed(lambda: eng.posterior_accumulate_pooled(g, p1, p2), reps))
        cp = copy_row(sb * n, f"stream copy of the pooled form's bytes ({shape})")
        po["fraction_of_copy"] = po["TB_per_s_median"] / cp["TB_per_s_median"]
        po["fraction_of_copy_range"] = [po["TB_per_s_range"][0] / cp["TB_per_s_median"], po["TB_per_s_range"][1] / cp["TB_per_s_median"]]
        rows += [po, cp]
        for K in lags:
            ring = torch.empty((K, n_chains, H * W), dtype=eng.state_dtype, device=dev)
            out = torch.zeros((K, H, W), dtype=torch.float64, device=dev)
            state_ = {"head": 0, "valid": 0}

            def call():
                eng.posterior_lagged(ring, K, state_["head"], state_["valid"], out)
                state_["head"] = (state_["head"] + 1) % K
                state_["valid"] = min(state_["valid"] + 1, K)

            for _ in range(K):                                 # fill the ring: the timed calls move the full (K + 2) values
                call()
            nbytes = (K + 2) * sb * n
            la = _rate(f"lagged pass {K} lags {shape}", nbytes, _timed(call, reps))
            cl = copy_row(nbytes, f"stream copy of the lagged pass's bytes ({K} lags, {shape})")
            la["ms_per_snapshot"] = la["ms_median"]
            la["fraction_of_copy"] = la["TB_per_s_median"] / cl["TB_per_s_median"]
            la["fraction_of_copy_range"] = [la["TB_per_s_range"][0] / cl["TB_per_s_median"], la["TB_per_s_range"][1] / cl["TB_per_s_median"]]
            la["ring_GiB"] = K * sb * n / 2 ** 30
            la["sums_check"] = bool((out == 0).all().item())   # the beds never change: every difference is 0
            rows += [la, cl]
            del ring, out
    finally:
        eng.close()
    for r in rows:
        print(json.dumps(r), flush=True)
    return rows


def cov_rows(n_chains, H, W, state, K, reps):
    import ctypes as C
    import torch
    from mcmc_gpu_amd.engine import GsmEngine
    eng = GsmEngine(H, W, n_chains, state_dtype=state)
    rows = []
    try:
        dev, plane, sb = eng.dev, H * W, 8 if state == "f64" else 4
        n = n_chains * plane
        eng.beds = (1000.0 + torch.randn((n_chains, H, W), dtype=torch.float64, device=dev)).to(eng.state_dtype)
        shape = f"{n_chains}x{H}x{W} {state}"
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def copy_row(nbytes, label):
            m = nbytes // 16                                   # doubles: 8 B read + 8 B written each
            src = torch.ones(m, dtype=torch.float64, device=dev)
            dst = torch.empty(m, dtype=torch.float64, device=dev)
            r = _rate(label, 16 * m, _timed(lambda: eng._check(eng.lib.gsm_debug_stream_copy(C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), m, st)), reps))
            del src, dst
            return r

        def share(row, cp):
            row["ms_per_snapshot"] = row["ms_median"]
            row["fraction_of_copy"] = row["TB_per_s_median"] / cp["TB_per_s_median"]
            row["fraction_of_copy_range"] = [row["TB_per_s_range"][0] / cp["TB_per_s_median"], row["TB_per_s_range"][1] / cp["TB_per_s_median"]]

        g = torch.full((H, W), 1000.0, dtype=torch.float64, device=dev)
        p1 = torch.zeros((H, W), dtype=torch.float64, device=dev)
        p2 = torch.zeros((H, W), dtype=torch.float64, device=dev)
        po = _rate(f"pooled accumulate {shape}", sb * n, _timed(lambda: eng.posterior_accumulate_pooled(g, p1, p2), reps))
        cp = copy_row(sb * n, f"stream copy of the pooled form's bytes ({shape})")
        share(po, cp)
        rows += [po, cp]
        probes = torch.randn((K, H, W), dtype=torch.float64, device=dev)
        proj = torch.empty((n_chains, K), dtype=torch.float64, device=dev)
        cross = torch.zeros((K, H, W), dtype=torch.float64, device=dev)
        pj_bytes = sb * n + (K + 1) * 8 * plane + 8 * n_chains * K
        pj = _rate(f"project pass {K} probes {shape}", pj_bytes, _timed(lambda: eng.posterior_project(g, probes, proj), reps))
        cpj = copy_row(pj_bytes, f"stream copy of the project pass's bytes ({K} probes, {shape})")
        share(pj, cpj)
        pj["cache_bytes"] = (K + 1) * 8 * n                    # g and the probes, re-read by every chain
        pj["cache_TB_per_s_median"] = (pj["cache_bytes"] + sb * n) / pj["ms_median"] / 1e9
        vec = (4 if plane % 4 == 0 else 2 if plane % 2 == 0 else 1) if sb == 4 else (2 if plane % 2 == 0 else 1)
        cell_blocks = (plane // vec + 255) // 256
        n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
        parts = max(1, min(-(-4 * n_cu // cell_blocks), n_chains))           # the rule of posterior_parts (posterior_device.h)
        cr_bytes = sb * n + 2 * parts * K * plane * 8 + 2 * K * plane * 8 + 8 * n_chains * K
        cr = _rate(f"cross pass {K} probes {shape}", cr_bytes, _timed(lambda: eng.posterior_cross(g, proj, K, cross), reps))
        ccr = copy_row(cr_bytes, f"stream copy of the cross pass's bytes ({K} probes, {shape})")
        share(cr, ccr)
        cr["parts"], cr["bed_bytes"] = parts, sb * n
        cr["bed_bytes_fraction_of_pooled_copy"] = (sb * n / cr["ms_median"] / 1e9) / cp["TB_per_s_median"]
        cr["sums_check"] = bool(torch.isfinite(cross).all().item())
        rows += [pj, cpj, cr, ccr]
    finally:
        eng.close()
    for r in rows:
        print(json.dumps(r), flush=True)
    return rows


def residual_rows(n_chains, H, state, reps, repeats, levels=(2.0, 10.0)):
    """The fused residual pass (a) beside the pooled pass of the same run (b), a stream copy of the bytes the fused pass must move (c:
    the state once, every part's slab written and read back, the planes read and written) and, with fp64 state, the composition that
    needs no new kernel (d: gsm_residual into a scratch array of the state's size, then gsm_posterior_accumulate_pooled on that
    scratch).  Each is the median of `reps` calls, `repeats` times over, the four alternating within a repeat."""
    import ctypes as C
    import torch
    from mcmc_gpu_amd import synthetic
    from mcmc_gpu_amd.engine import GsmEngine
    prob, ch, rf = synthetic.template(H)
    W = H
    eng = GsmEngine(H, W, n_chains, state_dtype=state)
    rows = []
    try:
        eng.set_static(ch.surf, ch.velx, ch.vely, ch.dhdt, ch.smb, None, np.ones((H, W), dtype=np.uint8), ch.mc_region_mask, ch.resolution, ch.sigma_mc)
        dev, plane, sb = eng.dev, H * W, 8 if state == "f64" else 4
        n = n_chains * plane
        bed0 = torch.as_tensor(np.ascontiguousarray(prob["bed"], dtype=np.float64)).to(dev)
        eng.beds = (bed0[None] + 20.0 * torch.randn((n_chains, H, W), dtype=torch.float64, device=dev)).to(eng.state_dtype)
        shape = f"{n_chains}x{H}x{W} {state}"
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        nf = 3 + len(levels)
        g = bed0.clone()
        rg = torch.zeros((H, W), dtype=torch.float64, device=dev)
        p1 = torch.zeros((H, W), dtype=torch.float64, device=dev)
        p2 = torch.zeros((H, W), dtype=torch.float64, device=dev)
        sums = torch.zeros((nf, H, W), dtype=torch.float64, device=dev)
        # the cut of the chain axis: the rule of posterior_residual_parts (posterior_device.h, posterior_residual_kernel.hip)
        vec = (4 if W % 4 == 0 else 2 if W % 2 == 0 else 1) if sb == 4 else (2 if W % 2 == 0 else 1)
        lx = 1
        while lx < 32 and lx < W // vec:
            lx *= 2
        tiles = -(-(W // vec) // lx) * -(-H // (256 // lx))
        n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
        parts = max(1, min(-(-4 * n_cu // tiles), n_chains, n_chains // 8))
        fused_bytes = sb * n + 2 * parts * nf * plane * 8 + 2 * nf * plane * 8
        m = fused_bytes // 16
        src = torch.ones(m, dtype=torch.float64, device=dev)
        dst = torch.empty(m, dtype=torch.float64, device=dev)
        calls = {"a fused residual pass": (fused_bytes, lambda: eng.posterior_residual(rg, levels, sums)),
                 "b pooled accumulate": (sb * n, lambda: eng.posterior_accumulate_pooled(g, p1, p2)),
                 "c stream copy of the fused pass's bytes": (16 * m, lambda: eng._check(eng.lib.gsm_debug_stream_copy(
                     C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), m, st)))}
        if state == "f64":
            scratch = torch.empty_like(eng.beds)

            def composition():
                eng.call(eng.lib.gsm_residual, eng.beds, scratch)
                eng.call(eng.lib.gsm_posterior_accumulate_pooled, scratch, rg, p1, p2, None, 0, None)

            calls["d gsm_residual into scratch, then the pooled pass on it"] = (3 * sb * n, composition)
        med = {name: [] for name in calls}
        for _ in range(repeats):
            for name, (nbytes, fn) in calls.items():
                row = _rate(f"{name} ({shape})", nbytes, _timed(fn, reps))
                med[name].append(row["ms_median"])
                rows.append(row)
        names = list(calls)
        summary = {"what": f"residual pass summary {shape}", "tiles": tiles, "parts": parts, "levels": list(levels), "bed_bytes": sb * n,
                   "ms_median_per_repeat": med, "fused_over_pooled": statistics.median(med[names[0]]) / statistics.median(med[names[1]]),
                   "fused_fraction_of_copy": statistics.median(med[names[2]]) / statistics.median(med[names[0]]),
                   "sums_check": bool((sums[0] <= (3 + reps) * repeats * n_chains).all().item() and torch.isfinite(sums).all().item())}
        if state == "f64":
            summary["fused_faster_than_composition_in_all_repeats"] = all(a < d for a, d in zip(med[names[0]], med[names[3]]))
            summary["composition_over_fused"] = statistics.median(med[names[3]]) / statistics.median(med[names[0]])
        rows.append(summary)
    finally:
        eng.close()
    for r in rows:
        print(json.dumps(r), flush=True)
    return rows


def local_rows(n_chains, H, state, reaches, reps, repeats):
    """The pass of the covariance with the neighbours at every reach of `reaches` beside (b) a stream copy of the beds' bytes and (c)
    the composition in torch that needs no new kernel: K sliced multiply-and-sum passes over d = beds - g.  (a) and (b) are the median
    of `reps` calls, (c) of 5, `repeats` times over, the three alternating within a repeat.  (a) and (c) are compared on their
    results too: the same sums within 1e-9 of sum |d||d'| (an fp64 reduction in another order)."""
    import ctypes as C
    import torch
    from mcmc_gpu_amd import synthetic
    from mcmc_gpu_amd.engine import GsmEngine
    prob, ch, rf = synthetic.template(H)
    W = H
    eng = GsmEngine(H, W, n_chains, state_dtype=state)
    rows = []
    try:
        dev, plane, sb = eng.dev, H * W, 8 if state == "f64" else 4
        n = n_chains * plane
        bed0 = torch.as_tensor(np.ascontiguousarray(prob["bed"], dtype=np.float64)).to(dev)
        eng.beds = (bed0[None] + 20.0 * torch.randn((n_chains, H, W), dtype=torch.float64, device=dev)).to(eng.state_dtype)
        shape = f"{n_chains}x{H}x{W} {state}"
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        g = bed0.clone()
        n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
        tiles = -(-H // 8) * -(-W // 64)
        m = sb * n // 16
        src = torch.ones(m, dtype=torch.float64, device=dev)
        dst = torch.empty(m, dtype=torch.float64, device=dev)
        for R in reaches:
            K = 2 * R * R + 2 * R
            offs = [(0, dj) for dj in range(1, R + 1)] + [(di, dj) for di in range(1, R + 1) for dj in range(-R, R + 1)]
            # the cut of the chain axis: the rule of posterior_local_parts (include/gsm.h, posterior_device.h)
            parts = max(1, min(-(-4 * n_cu // tiles), n_chains, 160 // K, (1 << 27) // (K * plane)))
            fused_bytes = sb * n + 2 * parts * K * plane * 8 + 2 * K * plane * 8
            cross = torch.zeros((K, H, W), dtype=torch.float64, device=dev)
            comp = torch.zeros((K, H, W), dtype=torch.float64, device=dev)

            def composition():
                d = eng.beds.to(torch.float64) - g
                for k, (di, dj) in enumerate(offs):
                    i1, j0, j1 = H - di, max(0, -dj), min(W, W - dj)
                    comp[k, :i1, j0:j1] += (d[:, :i1, j0:j1] * d[:, di:, j0 + dj:j1 + dj]).sum(dim=0)

            calls = {"a fused local pass": (fused_bytes, reps, lambda: eng.posterior_local(g, R, cross)),
                     "b stream copy of the beds' bytes": (16 * m, reps, lambda: eng._check(eng.lib.gsm_debug_stream_copy(
                         C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), m, st))),
                     "c torch composition, K sliced multiply-and-sum passes": ((1 + 2 * K) * 8 * n + sb * n, min(reps, 5), composition)}
            med = {name: [] for name in calls}
            n_calls = {name: 0 for name in calls}
            for _ in range(repeats):
                for name, (nbytes, r, fn) in calls.items():
                    row = _rate(f"{name} (reach {R}, {shape})", nbytes, _timed(fn, r))
                    n_calls[name] += r + 3
                    med[name].append(row["ms_median"])
                    rows.append(row)
            names = list(calls)
            # both were added to from zeros, a different number of times: compared per call
            a, c = cross / n_calls[names[0]], comp / n_calls[names[2]]
            scale = c.abs().max().item()
            rows.append({"what": f"local pass summary reach {R} {shape}", "reach": R, "offsets": K, "tiles": tiles, "parts": parts, "bed_bytes": sb * n,
                         "fma_per_snapshot": K * n, "ms_median_per_repeat": med,
                         "composition_over_fused": statistics.median(med[names[2]]) / statistics.median(med[names[0]]),
                         "fused_faster_than_composition_in_all_repeats": all(x < y for x, y in zip(med[names[0]], med[names[2]])),
                         "fused_over_copy": statistics.median(med[names[0]]) / statistics.median(med[names[1]]),
                         "largest_difference_from_composition_over_largest_sum": (a - c).abs().max().item() / scale})
    finally:
        eng.close()
    for r in rows:
        print(json.dumps(r), flush=True)
    return rows


def _bench_regions(H, W, K):
    """[K, H, W] bool: the whole domain, then nested and overlapping rectangles -- a basin, its sub-basins, as an ensemble is reported"""
    m = np.zeros((K, H, W), dtype=bool)
    m[0] = True
    for k in range(1, K):
        i0, j0 = (k * H) // (2 * K), (k * W) // (3 * K)
        m[k, i0: i0 + H // 2, j0: j0 + (2 * W) // 3] = True
    return m


def regions_rows(n_chains, H, state, K, bins, reps, repeats):
    """The region pass (a) with K regions (and `bins` hypsometry bins, 0 = none) beside (b) a stream copy of the beds' bytes, (c)
    gsm_posterior_project with K probes (the linear functionals of the same regions: their mean-bed weights) and (d) the composition
    that needs no new kernel, in torch on the same beds: thickness and thickness above flotation by clamp, then per region masked
    sums, counts, amin and amax over the plane (the hypsometry is left out of (d)).  (a), (b) and (c) are the median of `reps` calls,
    (d) of 5, `repeats` times over, the four alternating within a repeat.  (a) and (d) are compared on their results."""
    import ctypes as C
    import torch
    from mcmc_gpu_amd import posterior, synthetic
    from mcmc_gpu_amd.engine import GsmEngine
    prob, ch, rf = synthetic.template(H)
    W = H
    eng = GsmEngine(H, W, n_chains, state_dtype=state)
    rows = []
    try:
        eng.set_static(ch.surf, ch.velx, ch.vely, ch.dhdt, ch.smb, None, np.ones((H, W), dtype=np.uint8), ch.mc_region_mask, ch.resolution, ch.sigma_mc)
        dev, plane, sb = eng.dev, H * W, 8 if state == "f64" else 4
        n = n_chains * plane
        bed0 = torch.as_tensor(np.ascontiguousarray(prob["bed"], dtype=np.float64)).to(dev)
        eng.beds = (bed0[None] + 20.0 * torch.randn((n_chains, H, W), dtype=torch.float64, device=dev)).to(eng.state_dtype)
        shape = f"{n_chains}x{H}x{W} {state}"
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        masks = _bench_regions(H, W, K)
        sea, ratio = float(np.median(prob["bed"])), 1028.0 / 917.0            # the beds straddle it: every branch is taken
        lo, hi = float(prob["bed"].min()) - 50.0, float(prob["bed"].max()) + 50.0
        d_bits = torch.as_tensor(posterior.region_bits(masks)).to(dev)
        func = torch.empty((n_chains, K, 8), dtype=torch.float64, device=dev)
        hyps = torch.zeros((n_chains, K, bins + 2), dtype=torch.int32, device=dev) if bins else None
        g = bed0.clone()
        probes = torch.as_tensor(posterior.region_mean_probes(masks)).to(dev)
        proj = torch.empty((n_chains, K), dtype=torch.float64, device=dev)
        d_masks = torch.as_tensor(masks).to(dev)
        surf = torch.as_tensor(np.ascontiguousarray(ch.surf, dtype=np.float64)).to(dev)
        comp = torch.empty((n_chains, K, 8), dtype=torch.float64, device=dev)
        m = sb * n // 16
        src = torch.ones(m, dtype=torch.float64, device=dev)
        dst = torch.empty(m, dtype=torch.float64, device=dev)

        def fused():
            if bins:
                eng.posterior_regions(d_bits, K, sea, ratio, func, lo, bins / (hi - lo), bins, hyps)
            else:
                eng.posterior_regions(d_bits, K, sea, ratio, func)

        def composition():
            x = eng.beds.to(torch.float64)
            h = surf - x
            b = x - sea
            thick = h.clamp(min=0.0)
            haf = (h + ratio * b.clamp(max=0.0)).clamp(min=0.0)
            below = b < 0
            marine = below & (haf > 0)
            inf = torch.tensor(float("inf"), dtype=torch.float64, device=dev)
            for k in range(K):
                mk = d_masks[k]
                comp[:, k, 0] = float(mk.sum().item())
                comp[:, k, 1] = (x * mk).sum(dim=(1, 2))
                comp[:, k, 2] = (thick * mk).sum(dim=(1, 2))
                comp[:, k, 3] = (haf * mk).sum(dim=(1, 2))
                comp[:, k, 4] = (below & mk).sum(dim=(1, 2))
                comp[:, k, 5] = (marine & mk).sum(dim=(1, 2))
                comp[:, k, 6] = torch.where(mk, x, inf).amin(dim=(1, 2))
                comp[:, k, 7] = torch.where(mk, x, -inf).amax(dim=(1, 2))

        calls = {"a region pass": (sb * n, reps, fused),
                 "b stream copy of the beds' bytes": (16 * m, reps, lambda: eng._check(eng.lib.gsm_debug_stream_copy(
                     C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), m, st))),
                 "c project pass, K probes": (sb * n, reps, lambda: eng.posterior_project(g, probes, proj)),
                 "d torch composition, clamp and masked sums": (sb * n, min(reps, 5), composition)}
        med = {name: [] for name in calls}
        for _ in range(repeats):
            for name, (nbytes, r, fn) in calls.items():
                row = _rate(f"{name} ({K} regions, {bins} bins, {shape})", nbytes, _timed(fn, r))
                med[name].append(row["ms_median"])
                rows.append(row)
        names = list(calls)
        mm = {name: statistics.median(v) for name, v in med.items()}
        exact = bool(all(torch.equal(func[..., f], comp[..., f]) for f in (0, 4, 5, 6, 7)))
        scale = comp[..., 1:4].abs().amax().item()
        rows.append({"what": f"region pass summary {K} regions {bins} bins {shape}", "regions": K, "bins": bins, "bed_bytes": sb * n,
                     "ms_median_per_repeat": med, "pass_over_copy": mm[names[0]] / mm[names[1]], "pass_over_project": mm[names[0]] / mm[names[2]],
                     "composition_over_pass": mm[names[3]] / mm[names[0]],
                     "pass_faster_than_composition_in_all_repeats": all(x < y for x, y in zip(med[names[0]], med[names[3]])),
                     "counts_min_max_equal_composition": exact,
                     "largest_sum_difference_from_composition_over_largest_sum": (func[..., 1:4] - comp[..., 1:4]).abs().amax().item() / scale})
    finally:
        eng.close()
    for r in rows:
        print(json.dumps(r), flush=True)
    return rows


def end_to_end_rows(H, n_chains, n_iter, thins, repeats, ess_lags=None, cov_probes=None, residual=False, local=None, regions=None):
    import torch
    from mcmc_gpu_amd import MCMC_gpu, synthetic
    prob, ch, rf = synthetic.template(H)
    beds = synthetic.initial_beds(prob, n_chains)
    seeds = list(range(1000, 1000 + n_chains))
    if regions is not None:
        K, bins = regions
        m = _bench_regions(H, H, K)
        sea = float(np.median(prob["bed"]))
        ropt = dict(masks=m, sea_level=sea, hyps=dict(lo=float(prob["bed"].min()) - 50.0, hi=float(prob["bed"].max()) + 50.0, bins=bins) if bins else None)
        configs = [("no posterior", None)] + [(f"thin={t} rhat=True", dict(burn_in=0, thin=t)) for t in thins] + \
                  [(f"thin={t} rhat=True regions {K} hyps {bins}", dict(burn_in=0, thin=t, regions=ropt)) for t in thins]
    elif local:
        configs = [("no posterior", None)] + [(f"thin={t} rhat=True", dict(burn_in=0, thin=t)) for t in thins] + \
                  [(f"thin={t} rhat=True local reach {R}", dict(burn_in=0, thin=t, local=dict(reach=R))) for t in thins for R in local]
    elif residual:
        configs = [("no posterior", None)] + [(f"thin={t} rhat=True", dict(burn_in=0, thin=t)) for t in thins] + \
                  [(f"thin={t} rhat=True residual 2 levels", dict(burn_in=0, thin=t, residual=dict(levels=(2.0, 10.0)))) for t in thins]
    elif cov_probes is not None:
        P = np.random.default_rng(0).normal(size=(cov_probes, H, H))
        configs = [("no posterior", None)] + [(f"thin={t} rhat=True", dict(burn_in=0, thin=t)) for t in thins] + \
                  [(f"thin={t} rhat=True cov {cov_probes} probes", dict(burn_in=0, thin=t, cov=dict(probes=P))) for t in thins]
    elif ess_lags is None:
        configs = [("no posterior", None)] + [(f"thin={t} rhat={r}", dict(burn_in=0, thin=t, rhat=r)) for t in thins for r in (True, False)]
    else:
        configs = [("no posterior", None)] + [(f"thin={t} rhat=True", dict(burn_in=0, thin=t)) for t in thins] + \
                  [(f"thin={t} rhat=True ess max_lag={K}", dict(burn_in=0, thin=t, ess=dict(max_lag=K))) for t in thins for K in ess_lags]

    def run(opt):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = MCMC_gpu.run_many(ch, rf, beds, seeds, n_iter, batch=32, return_device=True, posterior=opt)
        dev, accum = out if opt is not None else (out, None)
        if accum is not None:
            accum.finalize()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        dev[0].close()
        return dt, (accum.T if accum is not None else 0)

    run(None)
    run(configs[1][1])                                          # warm-up of both paths
    wall = {name: [] for name, _ in configs}
    snaps = {}
    for _ in range(repeats):
        for name, opt in configs:                              # alternating: drift of the shared box hits every configuration alike
            dt, snaps[name] = run(opt)
            wall[name].append(dt)
    base = statistics.median(wall["no posterior"])
    rows = []
    for name, _ in configs:
        med = statistics.median(wall[name])
        row = {"what": f"run_many {n_chains}x{H}x{H}, {n_iter - 1} steps, {name}", "wall_s_median": med, "wall_s_min": min(wall[name]),
               "wall_s_max": max(wall[name]), "repeats": repeats, "snapshots": snaps[name],
               "chain_steps_per_s": n_chains * (n_iter - 1) / med}
        if snaps[name]:
            row["overhead_s"] = med - base
            row["overhead_ms_per_snapshot"] = 1e3 * (med - base) / snaps[name]
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="small shapes: a rehearsal of the script, not a measurement")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--hist", action="store_true", help="only the histogram pass beside the pooled pass and the stream copy")
    ap.add_argument("--ess", action="store_true", help="only the lagged pass beside its stream copy, and run_many with and without ess")
    ap.add_argument("--cov", type=int, default=0, metavar="K", help="only the two covariance passes with K probes beside their stream copies, "
                    "and run_many with and without cov")
    ap.add_argument("--residual", action="store_true", help="only the fused residual pass beside the pooled pass, its stream copy and the "
                    "composition of existing entry points, and run_many with and without residual")
    ap.add_argument("--local", type=int, nargs="+", default=None, metavar="R", help="only the pass of the covariance with the neighbours at "
                    "every reach given, beside the stream copy of the beds and the torch composition, and run_many with and without local")
    ap.add_argument("--regions", type=int, default=0, metavar="K", help="only the region pass with K regions beside the stream copy of the beds, "
                    "the project pass at the same K and the torch composition, and run_many with and without regions")
    ap.add_argument("--hyps", type=int, default=0, metavar="B", help="with --regions: B hypsometry bins (even, <= 64; 0 = none)")
    ap.add_argument("--no-end-to-end", action="store_true", help="with --residual, --local or --regions: the kernel rows alone")
    args = ap.parse_args()
    if args.cov and not 1 <= args.cov <= 15:
        raise SystemExit("--cov takes 1 .. 15 probes")
    if args.cov and args.out is None and not args.quick:
        args.out = str(ROOT / "profiles" / "posterior_bench_cov.json")
    if args.residual and args.out is None and not args.quick:
        args.out = str(ROOT / "profiles" / "posterior_bench_residual.json")
    if args.local and not all(1 <= R <= 4 for R in args.local):
        raise SystemExit("--local takes reaches in 1 .. 4")
    if args.local and args.out is None and not args.quick:
        args.out = str(ROOT / "profiles" / "posterior_bench_local.json")
    if args.regions and not (1 <= args.regions <= 8 and (args.hyps == 0 or (2 <= args.hyps <= 64 and args.hyps % 2 == 0))):
        raise SystemExit("--regions takes 1 .. 8 regions and --hyps 0 or an even number of bins in 2 .. 64")
    if args.regions and args.out is None and not args.quick:
        args.out = str(ROOT / "profiles" / "posterior_bench_regions.json")
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured (there is no CPU fallback)")
    rows = []
    if args.regions:
        for state in ("f64", "f32"):
            rows += regions_rows(8, 64, state, args.regions, args.hyps, 3, 1) if args.quick else \
                regions_rows(1024, 256, state, args.regions, args.hyps, max(args.reps, 20), args.repeats)
        if not args.no_end_to_end:
            rows += end_to_end_rows(64, 8, 1701, [100], 1, regions=(args.regions, args.hyps)) if args.quick else \
                end_to_end_rows(256, 1024, 20001, [100], args.repeats, regions=(args.regions, args.hyps))
    elif args.hist:
        for state in ("f64", "f32"):
            rows += hist_rows(8, 64, 64, state, 3) if args.quick else hist_rows(1024, 256, 256, state, args.reps)
    elif args.local:
        for state in ("f64", "f32"):
            rows += local_rows(8, 64, state, args.local, 3, 1) if args.quick else local_rows(1024, 256, state, args.local, max(args.reps, 20), args.repeats)
        if not args.no_end_to_end:
            rows += end_to_end_rows(64, 8, 1701, [100], 1, local=args.local) if args.quick else \
                end_to_end_rows(256, 1024, 20001, [100], args.repeats, local=args.local)
    elif args.residual:
        for state in ("f64", "f32"):
            rows += residual_rows(8, 64, state, 3, 1) if args.quick else residual_rows(1024, 256, state, max(args.reps, 20), args.repeats)
        if not args.no_end_to_end:
            rows += end_to_end_rows(64, 8, 1701, [100], 1, residual=True) if args.quick else \
                end_to_end_rows(256, 1024, 20001, [100], args.repeats, residual=True)
    elif args.cov:
        for state in ("f64", "f32"):
            rows += cov_rows(8, 64, 64, state, args.cov, 3) if args.quick else cov_rows(1024, 256, 256, state, args.cov, max(args.reps, 20))
        rows += end_to_end_rows(64, 8, 1701, [100], 1, cov_probes=args.cov) if args.quick else \
            end_to_end_rows(256, 1024, 20001, [100], args.repeats, cov_probes=args.cov)
    elif args.ess:
        for state in ("f64", "f32"):
            rows += ess_rows(8, 64, 64, state, (7, 15), 3) if args.quick else ess_rows(1024, 256, 256, state, (7, 15), max(args.reps, 20))
        rows += end_to_end_rows(64, 8, 1701, [100], 1, ess_lags=(7,)) if args.quick else \
            end_to_end_rows(256, 1024, 20001, [100], args.repeats, ess_lags=(7, 15))
    elif args.quick:
        rows += kernel_rows(8, 64, 64, "f64", 3)
        rows += kernel_rows(8, 64, 64, "f32", 3)
        rows += end_to_end_rows(64, 8, 129, [64, 16], 1)
    else:
        rows += kernel_rows(1024, 256, 256, "f64", args.reps)
        rows += kernel_rows(512, 1024, 1024, "f32", args.reps)
        rows += end_to_end_rows(256, 1024, 20481, [2048, 256, 64], args.repeats)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "rows": rows}, indent=1) + "\n")


if __name__ == "__main__":
    main()
