"""CPU: the trimmed window of the strip kernels (mcmc_gpu_amd/csrc/strip_step.h: make_window with the static rectangle of the update
mask) run on the host through config, lane_setup, write_masks and cell_written for every (wave, lane) of the workgroup:
tests/native/strip_trim_check.cpp states each property; it needs no GPU and calls no HIP runtime function.  Also on the CPU: the
conditions that keep the cases of tests/test_gpu_strip_trim.py from passing vacuously, on the oracle's chains."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else None)


@pytest.mark.skipif(HIPCC is None, reason="hipcc not found")
def test_trimmed_windows_are_tiled_once_and_keep_their_indices(tmp_path):
    exe = tmp_path / "strip_trim_check"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-I", str(ROOT / "mcmc_gpu_amd" / "csrc"), "-o", str(exe),
                    str(ROOT / "tests" / "native" / "strip_trim_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "strip trim ok" in r.stdout


def test_trim_cases_meet_their_conditions_on_the_oracle():
    import strip_trim_cases as cases
    for name in cases.CASES:
        for f32 in ((False, True) if name == "regroup" else (False,)):
            cases.conditions(name, *cases.oracle_blocks(cases.oracle_outs(name, f32)))


def test_rectangle_restatement():
    """strip_trim_cases.rectangle on the masks of the cases and on the two extremes."""
    import numpy as np
    import strip_trim_cases as cases
    assert cases.rectangle(cases.CASES["regroup"][6]()) == (19, 77, 21, 79)
    assert cases.rectangle(cases.CASES["l_shape"][6]()) == (17, 72, 0, 54)
    assert cases.rectangle(np.ones((8, 10), dtype=int)) == (0, 8, 0, 10)
    assert cases.rectangle(np.zeros((8, 10), dtype=int)) == (0, 0, 0, 0)
