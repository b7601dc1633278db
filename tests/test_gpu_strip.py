"""-m gpu: the strip kernels (chain_strip_kernel.hip: 512-thread workgroups, two chains per CU) against the flux-tile kernels
(chain_fused_kernel / step_flux_kernel, option strip = 0) on the same proposals.  Per-cell arithmetic is the same, operation for
operation (reference gstatsMCMC/MCMC.py:1279-1360, Topography.py:592-600): beds, energies, accept masks, blocks and resampled
counts must be identical; the loss differs by the order of the window sums only (tolerance 1e-12 relative, stated here).
The proposal fields of both runs are made equal with split2 = 0 (handles on the strip kernels otherwise split stage 2 of the
inverse DFT by the parity of kx, which the one-slot-per-wave flux-tile fused kernel cannot: last-bit differences in the fields).
The options are the handle's (gsm_set_option): the two engines of a comparison live side by side in this process.
The strip family against the ORACLE, one block table per decomposition of strip::config (the 4 x 64-lane one included, which no
table here reaches): tests/test_gpu_strip_oracle.py; its integer geometry on the host: tests/test_strip_geometry.py."""
import numpy as np
import pytest

import mcmc_oracle as orc
from gpu_common import make_engine
from mcmc_gpu_amd._lib import GsmError

pytestmark = pytest.mark.gpu
GSM_E_ARG = -1


def _run(eng, n, step0, seeds, rfp):
    loss, acc, blk = eng.run_philox(n, step0, seeds, rfp, batch=n)
    return dict(strip=int(eng.strip_active()), loss=loss, acc=acc, blk=blk, beds=eng.beds.cpu().numpy(),
                energy=eng.energy.cpu().numpy(), res=eng.resampled.cpu().numpy())


def _standard(H, state, **options):
    """make_engine's standard table with whole-map centres, 3 chains on their initial beds, and the options set"""
    eng, prob, cfg, pairs, masks, rfp = make_engine(H, 3, state_dtype=state)
    for name, value in options.items():
        eng.set_option(name, value)
    rfp = orc.standard_rf_params(); rfp.resolution = prob["resolution"]
    eng.set_centres(np.ones_like(cfg.region_mask))
    eng.set_state(np.stack([orc.chain_initial_bed(prob, c) for c in range(3)]))
    return eng, rfp


def _assert_strip_equals_flux_tile(a, b):
    assert a["strip"] == 1 and b["strip"] == 0          # the paths under test really ran
    for k in ("acc", "blk", "beds", "energy", "res"):
        assert np.array_equal(a[k], b[k]), k
    np.testing.assert_allclose(a["loss"], b["loss"], rtol=1e-12)


@pytest.mark.parametrize("H,n,state", [(64, 80, "f64"), (256, 60, "f64"), (64, 40, "f32")])
def test_strip_kernels_equal_flux_tile_kernels(H, n, state):
    """256: blocks 50-80 (16-, 32- and 64-lane strips, windows clipped on every side of the grid since centres may lie anywhere)."""
    ea, rfp = _standard(H, state, strip=1, split2=0)     # equal fields for both families: the flux-tile fused kernel has no split stage 2
    eb, _ = _standard(H, state, strip=0, split2=0)
    a, b = _run(ea, n, 5, [11, 12, 13], rfp), _run(eb, n, 5, [11, 12, 13], rfp)
    ea.close(); eb.close()
    _assert_strip_equals_flux_tile(a, b)
    assert 0.2 < a["acc"].mean() < 1.0


def test_standard_tables_run_the_strip_kernels():
    for H in (64, 256):
        eng, *_ = make_engine(H, 2)
        assert eng.strip_active()
        eng.close()


def _wide(H, W, bw0, bw1, bh0, bh1, **options):
    from mcmc_gpu_amd.engine import GsmEngine
    prob = orc.synthetic_problem(H, W)
    res = prob["resolution"]
    pairs = orc.block_pairs(bw0, bw1, bh0, bh1)          # (bw, bh) columns, MCMC.py:576-579
    lp = [2, 0, 6, 1]
    masks = orc.edge_masks(pairs, lp, 49900.0, res)
    w = orc.crf_weight(prob["xx"], prob["yy"], prob["data_mask"], lp, 49900.0)
    ones = np.full(prob["region_mask"].shape, 1)
    eng = GsmEngine(H, W, 3)
    for name, value in options.items():
        eng.set_option(name, value)
    eng.set_static(prob["surf"], prob["velx"], prob["vely"], prob["dhdt"], prob["smb"], w, ones, ones, res, 5.0)
    eng.set_blocks(pairs, masks)
    eng.set_centres(ones)                                          # whole-map updates: windows clipped on every side
    rfp = orc.standard_rf_params(); rfp.resolution = res
    eng.set_state(np.stack([orc.chain_initial_bed(prob, c) for c in range(3)]))
    return eng, rfp


def test_strip_kernels_equal_flux_tile_kernels_wide_blocks_on_an_oblong_grid():
    """Blocks 20 - 110 cells wide and 20 - 50 tall on a 128 x 192 grid, whole-map updates: every strip decomposition up to two
    64-lane column groups (strip::config: 64-, 16-, 32- and 2 x 64-lane strips), H != W, most windows clipped."""
    outs = {}
    engines = []
    for strip, split2 in ((1, 0), (0, 0), (1, 1)):
        eng, rfp = _wide(128, 192, 20, 110, 20, 50, strip=strip, split2=split2)
        engines.append(eng)
        outs[(strip, split2)] = _run(eng, 80, 3, [21, 22, 23], rfp)
    for eng in engines:
        eng.close()
    a, b, c = outs[(1, 0)], outs[(0, 0)], outs[(1, 1)]
    # stage 2 split by the parity of kx (the default on strip handles) against the direct sums: the same chain to rounding
    assert np.array_equal(c["acc"], a["acc"]) and np.array_equal(c["blk"], a["blk"])
    np.testing.assert_allclose(c["beds"], a["beds"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(c["loss"], a["loss"], rtol=1e-10)
    widths = set(int(x) for x in a["blk"][..., 3].ravel())
    assert max(widths) > 90 and min(widths) <= 62                 # the two-group 64-lane strips and the one-group ones both ran
    _assert_strip_equals_flux_tile(a, b)


def test_options_are_the_handles_and_checked():
    """gsm_set_option: strip_active follows the option from the next call on; an unknown option or a value outside its range is
    GSM_E_ARG and leaves the handle usable."""
    eng, prob, cfg, pairs, masks, rfp = make_engine(64, 2)
    assert eng.strip_active()
    eng.set_option("strip", 0)
    assert not eng.strip_active()
    eng.set_option("strip", 1)
    assert eng.strip_active()
    for call in (lambda: eng._check(eng.lib.gsm_set_option(eng.h, 99, 0)), lambda: eng.set_option("strip", 2),
                 lambda: eng.set_option("fused_segment", 0)):
        with pytest.raises(GsmError) as e:
            call()
        assert e.value.code == GSM_E_ARG
    assert eng.strip_active()
    rfp = orc.standard_rf_params(); rfp.resolution = prob["resolution"]
    eng.set_state(np.stack([orc.chain_initial_bed(prob, c) for c in range(2)]))
    loss, acc, blk = eng.run_philox(8, 0, [1, 2], rfp, batch=8)
    assert loss.shape == (2, 8) and np.isfinite(loss).all()
    eng.close()


def test_environment_is_read_per_handle_and_does_not_stick(monkeypatch):
    """GSM_STRIP is read when an engine is made, for that engine: one made under GSM_STRIP=0 stays on the flux-tile kernels after
    the variable is gone, one made afterwards beside it runs the strip kernels, and the two agree as the two families must."""
    monkeypatch.setenv("GSM_STRIP", "0")
    ea, rfp = _standard(64, "f64", split2=0)
    assert not ea.strip_active()
    monkeypatch.delenv("GSM_STRIP")
    eb, _ = _standard(64, "f64", split2=0)
    assert eb.strip_active() and not ea.strip_active()
    a, b = _run(ea, 8, 5, [11, 12, 13], rfp), _run(eb, 8, 5, [11, 12, 13], rfp)
    ea.close(); eb.close()
    _assert_strip_equals_flux_tile(b, a)
