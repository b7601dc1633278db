"""-m gpu: the oracle parity tests on the flux-tile kernels (step_flux_kernel, chain_fused_kernel) and the bed-tile kernel
(step_kernel) -- the families that run every grid above about 295 x 295, BASELINE configs[3] and configs[4] among them.

The oracle cannot run such a grid in seconds, and at the 16-256 grids of the oracle tests the strip kernels take every table
(tests/test_gpu_strip.py), so those tests pin the strip family only (table by table: tests/test_gpu_strip_oracle.py).  GSM_STRIP=0
routes a small grid to the other two: every engine made while it is set takes it as its option strip = 0, so each group of cases
runs under monkeypatch.setenv (tests/flux_tile_oracle_cases.py: run_cases).

  group A  the bodies of the oracle tests of test_gpu_parity, test_gpu_fullsize, test_gpu_fused and test_gpu_philox, unchanged
  group B  one block table per instantiation against the oracle in replay mode, windows clipped on every edge:
           step_flux_kernel KT 2 / 4 / 7 and step_kernel KMAX 7 / 12 / 20, each with fp64 and fp32 state, with NaN cells in the
           bed, velx and dhdt, and with a proposal that trips the thickness guard; every case asserts the interval of the
           dispatch rule its table lies in
  group C  Philox mode on the KT 2 / 4 / 7 tables: chain_fused_kernel == propose + replay == two-kernel pipeline, and the
           direct-sum proposal fields against the Philox oracle

Bars (the project's standing ones): accept masks, final beds and resampled counts bit-exact, losses within 1e-10 relative;
Philox-mode comparisons between device paths bit for bit; proposal fields within philox_oracle.field_atol."""
import pytest

import flux_tile_oracle_cases as cases
from gpu_common import make_engine

pytestmark = pytest.mark.gpu


def _run_group(monkeypatch, group):
    monkeypatch.setenv("GSM_STRIP", "0")
    eng, *_ = make_engine(64, 1)
    assert eng.strip_active() == 0, "GSM_STRIP=0 did not take the standard 64 table off the strip kernels"
    eng.close()
    cases.run_cases(cases.group_cases(group))


@pytest.mark.parametrize("group", ["parity", "fused", "philox_oracle"])
def test_existing_oracle_tests_on_the_flux_tile_kernels(monkeypatch, group):
    _run_group(monkeypatch, group)


@pytest.mark.parametrize("name", cases.STRIP_ELIGIBLE)
def test_table_against_oracle(monkeypatch, name):
    _run_group(monkeypatch, "table:" + name)


@pytest.mark.parametrize("name", ["bed_kmax12", "bed_kmax20"])
def test_large_table_against_oracle(name):
    """Tiles above 80 KiB never go to the strip kernels: no GSM_STRIP needed (every case still asserts strip_active() == 0)."""
    cases.run_cases(cases.table_cases(name))


def test_philox_mode_on_the_flux_tile_tables(monkeypatch):
    _run_group(monkeypatch, "philox_tables")
