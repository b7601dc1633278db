"""-m gpu: the strip kernels on windows cut down to the static rectangle of the update mask (strip_step.h: make_window with the
rectangle; gsm_set_static computes it).  tests/strip_trim_cases.py holds the cases and what each must have run: windows whose
trimming changes the decomposition, windows that keep it with shallower strips, whole windows, an L-shaped mask with a hole (only
its bounding box matters) and windows that the trimming leaves empty.  The loss mask is all ones in every case, so the cells that
are left out carry non-zero energies.

Bars, the project's standing ones.  Against the NumPy oracle (tests/test_gpu_strip_oracle.py): accept masks, final beds and
resampled counts bit-exact, losses within 1e-10 relative.  Against the flux-tile kernels, which do not trim, on a second engine with
the option strip = 0 (tests/test_gpu_strip.py): accept masks, beds, the ENERGY plane and resampled counts identical, losses within 1e-12
relative.  Philox mode: fused chain kernel == propose + replay == two-kernel pipeline, bit for bit."""
import numpy as np
import pytest

import mcmc_oracle as orc
import strip_trim_cases as cases
from flux_tile_oracle_cases import _bars
from gpu_common import replay_inputs

pytestmark = pytest.mark.gpu


def _flux_tile(name, state, outs):
    """The same replay on the flux-tile kernels: a second engine with the option strip = 0."""
    eng, prob, *_ = cases.engine(name, cases.N_CHAINS, state)
    eng.set_option("strip", 0)
    eng.set_state(np.stack([orc.chain_initial_bed(prob, c) for c in range(cases.N_CHAINS)]))
    loss, acc = eng.run_replay(*replay_inputs(eng, outs))
    b = dict(strip=int(eng.strip_active()), loss=loss, acc=acc, beds=eng.beds.cpu().numpy(), energy=eng.energy.cpu().numpy(),
             res=eng.resampled.cpu().numpy())
    eng.close()
    return b


@pytest.mark.parametrize("name,state", [("regroup", "f64"), ("regroup", "f32"), ("deeper", "f64"), ("deeper_some_whole", "f64"), ("l_shape", "f64"),
                                        ("empty", "f64")])
def test_trimmed_windows_replay_the_oracle_and_equal_the_flux_tile_kernels(name, state):
    f32 = state == "f32"
    outs = cases.oracle_outs(name, f32)
    cases.conditions(name, *cases.oracle_blocks(outs))
    eng, prob, cfg, *_ = cases.engine(name, cases.N_CHAINS, state)
    assert eng.strip_active() == 1, "strip_table_ok refuses the table"
    loss0 = eng.set_state(np.stack([orc.chain_initial_bed(prob, c) for c in range(cases.N_CHAINS)]))
    loss, acc = eng.run_replay(*replay_inputs(eng, outs))
    assert eng.beds.dtype.itemsize == eng.energy.dtype.itemsize == (4 if f32 else 8)
    _bars(eng, outs, loss0, loss, acc)
    a = dict(loss=loss, acc=acc, beds=eng.beds.cpu().numpy(), energy=eng.energy.cpu().numpy(), res=eng.resampled.cpu().numpy())
    eng.close()
    # the cells the trimming leaves out carry energy: outside the update mask, inside the loss mask
    outside = np.asarray(cfg.grounded_ice_mask) == 0
    assert outside.any() and (a["energy"][:, outside] != 0).mean() > 0.9
    b = _flux_tile(name, state, outs)
    assert int(b["strip"]) == 0                                    # the untrimmed kernels really ran
    for k in ("acc", "beds", "energy", "res"):
        if not np.array_equal(a[k], b[k]):
            at = tuple(int(v[0]) for v in np.nonzero(a[k] != b[k]))         # (chain, step) or (chain, row, column)
            raise AssertionError(f"{k} differs from the flux-tile kernels in {int((a[k] != b[k]).sum())} places, first at {at}: "
                                 f"{a[k][at]!r} against {b[k][at]!r}")
    np.testing.assert_allclose(a["loss"], b["loss"], rtol=1e-12)


@pytest.mark.parametrize("name,state", [("regroup", "f64"), ("empty", "f64"), ("l_shape", "f32")])
def test_philox_mode_on_trimmed_windows_fused_equals_replay_equals_pipeline(name, state):
    """tests/strip_oracle_cases.philox_table with the case's update mask: chain_strip_kernel and step_strip_kernel take the same
    trimmed geometry from the same function."""
    n_chains, n = 3, 24
    eng, prob, cfg, pairs, masks, _ = cases.engine(name, n_chains, state)
    assert eng.strip_active() == 1
    H, W = cases.CASES[name][:2]
    rfp = orc.standard_rf_params(); rfp.resolution = prob["resolution"]
    eng.set_centres(np.ones((H, W), dtype=np.uint8))
    seeds = [61, 2 ** 40 + 62, 63]
    beds0 = np.stack([orc.chain_initial_bed(prob, c) for c in range(n_chains)])

    def state_now():
        return (eng.beds.cpu().numpy().copy(), eng.resampled.cpu().numpy().copy(), eng.energy.cpu().numpy().copy())

    eng.set_fused(True)
    eng.set_state(beds0)
    loss, acc, blk = eng.run_philox(n, 9, seeds, rfp, batch=n)
    assert eng.last_run_fused() == 1
    st_a = state_now()
    t = cases.trims(name, blk)
    n_trim, n_empty = sum(x["trimmed"] for x in t), sum(x["empty"] for x in t)
    print(f"    {name} {state}: {len(t)} steps, {n_trim} trimmed ({n_empty} to nothing), accept rate {acc.mean():.2f}", flush=True)
    assert n_trim - n_empty >= 10 and (name != "empty" or n_empty >= 10)
    assert 0.2 <= acc.mean() <= (1.0 if name == "empty" else 0.95)      # an empty window is a zero change: always accepted
    outside = np.asarray(cfg.grounded_ice_mask) == 0
    assert np.array_equal(st_a[0][:, outside], beds0[:, outside].astype(st_a[0].dtype)) and not np.array_equal(st_a[0], beds0.astype(st_a[0].dtype))

    eng.set_state(beds0)
    p = eng.propose_philox(n, 9, seeds, rfp)
    si, ce = p["size_idx"].cpu().numpy(), p["centre"].cpu().numpy()
    loss_r, acc_r = eng.run_replay(si, ce, p["u"].cpu().numpy(), p["fields"])
    assert np.array_equal(loss, loss_r) and np.array_equal(acc, acc_r)
    assert np.array_equal(blk[..., :2], ce) and np.array_equal(blk[..., 2], pairs[1][si]) and np.array_equal(blk[..., 3], pairs[0][si])
    for x, y in zip(st_a, state_now()):
        assert np.array_equal(x, y)

    eng.set_fused(False)
    eng.set_state(beds0)
    loss_p, acc_p, blk_p = eng.run_philox(n, 9, seeds, rfp, batch=7)
    assert eng.last_run_fused() == 0
    assert np.array_equal(loss, loss_p) and np.array_equal(acc, acc_p) and np.array_equal(blk, blk_p)
    for x, y in zip(st_a, state_now()):
        assert np.array_equal(x, y)
    eng.close()
