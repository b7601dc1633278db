"""CPU: the integer geometry of the strip kernels (mcmc_gpu_amd/csrc/strip_step.h: config, rows_per_strip, small_div,
make_window, lane_setup, write_masks, cell_written are __host__ __device__) run on the host for every (wave, lane) of the
workgroup, over the windows of the five tables of tests/strip_oracle_cases.py and of the small grids of test_gpu_parity:
own cells partition the window and stay inside the grid, phase A writes every window cell of the tile once, the ring cells
that exist in the grid and nothing else, fidx / tidx agree with the oracle's window_bounds, and the divisions without a divide
are exact.  tests/native/strip_geometry_check.cpp states each property; it needs no GPU and calls no HIP runtime function."""
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
