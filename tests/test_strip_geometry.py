"""CPU: the integer geometry of the strip kernels (mcmc_gpu_amd/csrc/strip_step.h: config, rows_per_strip, small_div,
make_window on step_common.h's clip_window, lane_setup, write_masks, cell_written are __host__ __device__) run on the host for every (wave, lane) of the
workgroup, over the windows of the five tables of tests/strip_oracle_cases.py and of the small grids of test_gpu_parity:
own cells partition the window and stay inside the grid, phase A writes every window cell of the tile once, the ring cells
that exist in the grid and nothing else, fidx / tidx agree with the oracle's window_bounds, and the divisions without a divide
are exact.  The same program checks the geometry all five step kernels share (mcmc_gpu_amd/csrc/step_common.h: clip_window,
halo_tile, halo_tile_width, halo_touches, in_window, field_index) on those windows and on every centre of a 12 x 12 and a 9 x 14
grid: window and halo tile against the oracle's window_bounds, the record's tile width against the tile, and the overlap predicate
against a brute-force test over all ordered pairs of windows.  tests/native/strip_geometry_check.cpp states each property; it needs
no GPU and calls no HIP runtime function.

Also on the CPU: what makes the 'pcg64'-mode cases of tests/strip_oracle_cases.py (noise_table, noise_every_shape) fair."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else None)


@pytest.mark.skipif(HIPCC is None, reason="hipcc not found")
def test_strip_geometry_partitions_every_window(tmp_path):
    exe = tmp_path / "strip_geometry_check"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-I", str(ROOT / "mcmc_gpu_amd" / "csrc"), "-o", str(exe),
                    str(ROOT / "tests" / "native" / "strip_geometry_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "strip geometry ok" in r.stdout


def test_noise_table_decisions_are_far_from_flipping():
    """noise_table demands the oracle chain's accept mask from a device whose losses follow the oracle's within 1e-10 relative: no
    decision of its chains may lie closer than 1e-7 (relative to the loss) to flipping, and the chains of the variants meet the
    non-vacuity conditions of their tables.  Measured: 8.2e-7 (strip_g4), >= 9.6e-6 on the other tables, 7.7e-6 and 2.5e-6 on the
    two variants."""
    import numpy as np
    import strip_oracle_cases as cases
    for name, variant in cases.NOISE_CASES:
        m = cases.decision_margin(name, variant)
        print(f"    {name} {variant}: closest decision {m:.2e} x loss")
        assert m > 1e-7, (name, variant, m)
        outs = cases.noise_oracle_outs(name, variant)
        cases.oracle_conditions(name, outs)


def test_every_shape_inputs_cover_each_size_twice():
    """noise_every_shape: every size index once with an interior window and once clipped at the bottom right corner, ranges between
    0.15 and 0.6 of the block's shorter side (at least 1.5 cells), raw fields far from all-DC (|mean| / std <= 100, as in
    tests/test_spectral_shape_cases.py)."""
    import numpy as np
    import mcmc_oracle as orc
    import strip_oracle_cases as cases
    for name in cases.TABLES:
        H, W, prob, cfg, pairs, masks, rfp, si, ce, ds = cases.every_shape_inputs(name)
        assert si.tolist() == [i for i in range(pairs.shape[1]) for _ in range(2)]
        worst = 0.0
        for s, d in enumerate(ds):
            bh, bw = d["n_re"].shape
            interior = cases.window(ce[s][0], ce[s][1], bh, bw, H, W)[4]
            assert interior == (s % 2 == 0) and d["scale"] == 1e-3 and masks[si[s]].min() == 0.75
            lo = max(0.15 * min(bh, bw), 1.5) * rfp.resolution
            assert lo <= min(d["range_x"], d["range_y"]) and max(d["range_x"], d["range_y"]) <= max(0.6 * min(bh, bw), 1.5) * rfp.resolution
            f = np.fft.ifft2((d["n_re"] + 1j * d["n_im"]) * orc.spectral_amplitude((bh, bw), rfp.resolution, "Matern", d["range_x"], d["range_y"],
                                                                                  rfp.smoothness)).real
            worst = max(worst, abs(f.mean()) / (f.std() + 1e-12))
        print(f"    {name}: {len(ds)} steps, worst |mean| / std of the raw field {worst:.1f}")
        assert worst <= 100.0
