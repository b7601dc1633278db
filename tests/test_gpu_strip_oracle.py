"""-m gpu: the strip kernels (chain_strip_kernel, step_strip_kernel, strip_step.h) against the oracle, one block table per
decomposition of strip::config -- the family that runs every table at 256 x 256 and below.

The other oracle tests (test_gpu_parity, test_gpu_fullsize, test_gpu_fused, test_gpu_philox) run the strip family too, but on
8-16 cell blocks (one column group, strips at most 2 rows deep) and one fp64 replay with blocks 50-80.  Here every reachable
decomposition has a table whose widths lie in its interval and whose heights are the tallest strip_table_ok admits
(tests/strip_oracle_cases.py: TABLES), on oblong grids with centres anywhere, so that windows clip on all four edges:

  replay_table      the oracle's draws replayed, fp64 and fp32 state (RowIO<float> on strips up to 16 rows deep)
  replay_table_nan  NaN cells in velx, dhdt and the initial bed
  guard_table       a proposal that trips the thickness guard in the last row of the last row strip of the last column group,
                    deeper than the 4-slot (wupd, surf) ring of phase A, with an interior and with a clipped window
  philox_table      Philox mode: fused chain kernel == propose + replay == two-kernel pipeline, fp64 and fp32 state; on two
                    tables the proposal fields against the Philox oracle
  noise_table       'pcg64' mode: gsm_draw_pcg64 + gsm_run_noise against the oracle's chains, and against gsm_spectral_from_noise +
                    gsm_run_replay bit for bit; on two tables also with an anisotropic Exponential model and a nugget
  noise_every_shape every shape of the table through the chain kernel's own DFT forms, interior and clipped, never-zero edge masks:
                    gsm_run_noise == the two calls bit for bit, the two-call fields within 1e-12 x scale of the oracle

Every oracle case asserts what keeps it from passing vacuously (strip_oracle_cases.conditions) and prints the figures.  The
integer geometry of the decompositions has a host test of its own: tests/test_strip_geometry.py.

Bars (the project's standing ones): accept masks, final beds and resampled counts bit-exact, losses within 1e-10 relative;
Philox-mode comparisons between device paths bit for bit; proposal fields within philox_oracle.field_atol."""
import pytest

import strip_oracle_cases as cases

pytestmark = pytest.mark.gpu
NAMES = list(cases.TABLES)


@pytest.mark.parametrize("state", ["f64", "f32"])
@pytest.mark.parametrize("name", NAMES)
def test_replay_table(name, state):
    cases.replay_table(name, state)


@pytest.mark.parametrize("name", NAMES)
def test_replay_table_nan(name):
    cases.replay_table_nan(name)


@pytest.mark.parametrize("name", NAMES)
def test_guard_table(name):
    cases.guard_table(name)


@pytest.mark.parametrize("state", ["f64", "f32"])
@pytest.mark.parametrize("name", NAMES)
def test_philox_table(name, state):
    cases.philox_table(name, state, fields_vs_oracle=(state == "f64" and name in cases.FIELDS_VS_ORACLE))


@pytest.mark.parametrize("name,variant", cases.NOISE_CASES)
def test_noise_table(name, variant):
    cases.noise_table(name, variant)


@pytest.mark.parametrize("name", NAMES)
def test_noise_every_shape(name):
    cases.noise_every_shape(name)
