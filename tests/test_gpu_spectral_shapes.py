"""-m gpu: the device spectral synthesis (proposal_device.h through gsm_spectral_from_noise) at every even block shape from 2 x 2
to 128 x 128, three covariance models each, against mcmc_oracle.spectral_from_draws -- tests/spectral_shape_cases.py has the
tables, the never-zero edge masks, the draws and the restatement of the device's geometry; tests/test_spectral_shape_cases.py
shows on the CPU that the flat bar is a fair one.

Two handle forms.  'bare': no gsm_set_static, so strip_for is 0 and split2 = parseval = 0 -- direct stage-2 sums, the variance from
the field.  'static': the fields of the standard 128 x 128 setup; tables that strip_table_ok admits run the parity-split stage 2
and the Parseval variance, the others run as in 'bare'.  The test asserts the handle's own decisions against the restatement:
strip_active() per table, and that exactly the tables the restatement refuses are refused.

Bar, per field: max |device - oracle x mask| <= 1e-12 x scale, flat; the doubles of a record beyond bh x bw stay 0 (the output is
zero-filled: anything else is a write out of range).  Every admissible shape, every model, both forms."""
import ctypes as C

import numpy as np
import pytest
import torch

import mcmc_oracle as orc
import spectral_shape_cases as sc

pytestmark = pytest.mark.gpu


def _static(eng, H, W):
    prob, cfg, _, _, _ = orc.standard_setup(H, W)
    eng.set_static(cfg.surf, cfg.velx, cfg.vely, cfg.dhdt, cfg.smb, cfg.crf_data_weight, cfg.region_mask, cfg.mc_region_mask,
                   cfg.resolution, cfg.sigma_mc)


def _run_table(eng, key, form, tally):
    """One table on `eng`: the decisions against the restatement, then 64 shapes x 3 models.  Returns (worst err / scale, where)."""
    from mcmc_gpu_amd._lib import GsmError
    plan = sc.table_plan(key)
    shapes = plan["shapes"]
    n = len(shapes)
    try:
        eng.set_blocks(sc.pairs_of(shapes), [sc.mask1d(bh, bw) for bh, bw in shapes])
    except GsmError as e:
        assert not plan["admissible"] and "LDS" in str(e), (key, str(e))
        tally["refused"].append(key)
        return 0.0, None
    if form == "static":
        assert eng.strip_active() == plan["strip"], f"table {key}: strip_active() {eng.strip_active()}, restated {plan['strip']}"
    stride = eng.field_stride
    ds = [sc.draws(bh, bw) for bh, bw in shapes]

    def pack(name):
        out = np.zeros((n, stride))
        for r, d in enumerate(ds):
            out[r, :d[name].size] = d[name].ravel()
        return eng._f64(out)

    d_re, d_im, d_ng = pack("n_re"), pack("n_im"), pack("n_nug")          # packed once per table, shared by the three models
    d_si = torch.arange(n, dtype=torch.int32, device=eng.dev)
    d_sc = eng._f64(np.array([[d["scale"], d["nug"], d["range_x"], d["range_y"]] for d in ds]))
    worst = (0.0, None)
    for model, nugget in sc.MODELS:
        p = eng.rf_struct(sc.rf_params(model, nugget))
        out = torch.zeros((n, stride), dtype=torch.float64, device=eng.dev)
        try:
            eng.call(eng.lib.gsm_spectral_from_noise, n, d_si, d_sc, C.byref(p), d_re, d_im, d_ng if nugget else None, out, stride)
        except GsmError as e:
            assert not plan["admissible"] and "too large" in str(e), (key, str(e))
            tally["refused"].append(key)
            return 0.0, None
        assert plan["admissible"], f"table {key} ran, the restatement refuses it"
        torch.cuda.synchronize(eng.dev)
        h = out.cpu().numpy()
        for r, ((bh, bw), d) in enumerate(zip(shapes, ds)):
            exp = sc.expected(d, model, nugget, (bh, bw)) * sc.mask1d(bh, bw)
            err = np.abs(h[r, :bh * bw].reshape(bh, bw) - exp).max() / d["scale"]
            if not err <= worst[0]:                        # NaN counts as worst
                worst = (err, (bh, bw, model))
            assert err <= sc.BAR, (f"{form} table {key} {model} {bh} x {bw}: max error {err:.3e} x scale; geometry "
                                   f"{sc.prop_geom(bh, bw, plan['split2'][r] and form == 'static')}, classes "
                                   f"{sorted(sc.classes(bh, bw, plan if form == 'static' else None, r))}")
            assert np.abs(exp).max() > 0.5 * d["scale"]
            assert not h[r, bh * bw:].any(), f"{form} table {key} {model} {bh} x {bw}: non-zero beyond the record"
    tally["tables"].append(key)
    tally["wide"] += plan["wide"]
    tally["strip"] += bool(plan["strip"] and form == "static")
    return worst


def _report(label, form, tally, worst):
    keys = tally["tables"]
    cnt = sc.count_classes(keys, form == "static")
    print(f"\n    {label} {form}: {len(keys)} tables ({tally['wide']} wide, {tally['strip']} on the strip kernels), refused {tally['refused']}; "
          f"worst err / scale {worst[0]:.2e} at {worst[1]}\n    classes: " + ", ".join(f"{c} {cnt[c]}" for c in sorted(cnt)), flush=True)


@pytest.mark.parametrize("form", ["bare", "static"])
@pytest.mark.parametrize("i", range(8))
def test_every_even_shape_of_a_height_band(i, form):
    from mcmc_gpu_amd.engine import GsmEngine
    eng = GsmEngine(sc.GRID, sc.GRID, 1)
    if form == "static":
        _static(eng, sc.GRID, sc.GRID)
    tally = dict(tables=[], refused=[], wide=0, strip=0)
    worst = (0.0, None)
    for j in range(8):
        w = _run_table(eng, (i, j), form, tally)
        if not w[0] <= worst[0]:
            worst = w
    eng.close()
    _report(f"band {i}", form, tally, worst)
    expect_refused = [k for k in [(i, j) for j in range(8)] if not sc.table_plan(k)["admissible"]]
    assert tally["refused"] == expect_refused
    assert tally["wide"] == sum(sc.table_plan((i, j))["wide"] for j in range(8))
    assert len(tally["tables"]) + len(expect_refused) == 8


@pytest.mark.parametrize("form", ["bare", "static"])
def test_more_than_eight_tiles_along_a_side(form):
    """Lengths beyond 128 (spectral_shape_cases.EXTRA): 9 tile rows in stage 2 ('tall') and 9 tile columns in stage 1 ('long'), the
    division branch of tile_magic.  Neither table goes to the strip kernels, so both forms run the direct stage 2."""
    from mcmc_gpu_amd.engine import GsmEngine
    for name in sc.EXTRA:
        H, W = sc.EXTRA_GRID[name]
        eng = GsmEngine(H, W, 1)
        if form == "static":
            _static(eng, H, W)
        tally = dict(tables=[], refused=[], wide=0, strip=0)
        worst = _run_table(eng, name, form, tally)
        eng.close()
        _report(name, form, tally, worst)
        assert tally["tables"] == [name] and tally["strip"] == 0
