"""-m gpu: chain groups of the small-scale chain -- gsm_sgs_set_groups at the C ABI, run_many_sgs(groups=), sgs.handoff
(set-up: tests/sgs_groups_common.py).

Kernel level: with groups set, gsm_sgs_loss, gsm_sgs_state_init and gsm_qt_transform (both directions) give every chain, bit for bit,
what the same call gives on a handle that holds only that group's chains and is handed that group's plane or tables.
Run level: run_many_sgs(groups=) equals one run_many_sgs call per group on a template set up with that group's trend and transformer
and the same generators or seeds per chain: beds, accept masks, blocks, counts, generator states bit for bit, losses bit for bit
with device draws and to 1e-12 relative with host draws."""
import ctypes as C

import numpy as np
import pytest

import posterior_common as pc
import sgs_groups_common as gc

pytestmark = pytest.mark.gpu
GSM_E_ARG = -1
N_ITER = 16


def _engine(ch, n):
    from mcmc_gpu_amd.engine import GsmEngine
    eng = GsmEngine(gc.H, gc.H, n)
    eng.set_static(ch.surf, ch.velx, ch.vely, ch.dhdt, ch.smb, None, ch.grounded_ice_mask, ch.mc_region_mask, ch.resolution, ch.sigma_mc)
    return eng


def _set_groups(eng, of, n_groups):
    of = np.ascontiguousarray(of, dtype=np.int32)
    return eng.lib.gsm_sgs_set_groups(eng.h, of.ctypes.data_as(C.POINTER(C.c_int32)), n_groups)


def _loss_and_state(eng, beds, trend):
    import torch
    n = beds.shape[0]
    d_beds, d_trend = eng._f64(beds), eng._f64(trend)
    loss = torch.empty(n, dtype=torch.float64, device=eng.dev); bad = torch.empty(n, dtype=torch.int32, device=eng.dev)
    energy = torch.empty((n, gc.H, gc.H), dtype=torch.float64, device=eng.dev); state = torch.empty((n, 4), dtype=torch.float64, device=eng.dev)
    eng.call(eng.lib.gsm_sgs_loss, d_beds, d_trend, loss, bad)
    eng.call(eng.lib.gsm_sgs_state_init, d_beds, d_trend, energy, state)
    return loss.cpu().numpy(), bad.cpu().numpy(), energy.cpu().numpy(), state.cpu().numpy()


def _qt(eng, q, ref, x, inverse):
    import torch
    d_q, d_ref, d_x = eng._f64(q), eng._f64(ref), eng._f64(x)
    out = torch.empty_like(d_x)
    eng.call(eng.lib.gsm_qt_transform, d_q, d_ref, int(q.shape[-1]), d_x, out, int(d_x.numel()), int(inverse))
    return out.cpu().numpy()


def test_kernels_read_the_group_of_the_chain():
    prob, trends, nst = gc.tables("qt")
    ch = gc.template(prob, trends[0], nst[0])
    of = gc.OF
    beds = np.stack(gc.beds_of(prob, of.size))
    beds[1, 10, 12] = prob["surf"][10, 12] + 30.0                                      # a bad cell (thickness < 0) in one chain
    detr = beds - trends[of]
    q = np.stack([t.quantiles_[:, 0] for t in nst]); ref = np.stack([t.references_ for t in nst])
    eng = _engine(ch, of.size)
    try:
        assert _set_groups(eng, of, gc.G) == 0
        got = _loss_and_state(eng, detr, trends)
        fwd = _qt(eng, q, ref, detr, 0)
        inv = _qt(eng, q, ref, fwd, 1)
        # with groups the transform takes whole maps of all chains only
        import torch
        d = eng._f64(detr)
        with torch.cuda.device(eng.dev):
            rc = eng.lib.gsm_qt_transform(eng.h, C.c_void_p(d.data_ptr()), C.c_void_p(d.data_ptr()), 200, C.c_void_p(d.data_ptr()),
                                          C.c_void_p(d.data_ptr()), int(d.numel()) - 1, 0, eng._stream())
        assert rc == GSM_E_ARG
        # refusals of the setter leave the groups as they were
        assert _set_groups(eng, [0, 1, 2, 3, 4, 0], gc.G) == GSM_E_ARG and _set_groups(eng, [0, -1, 0, 0, 0, 0], gc.G) == GSM_E_ARG
        assert _set_groups(eng, of, 0) == GSM_E_ARG
        again = _loss_and_state(eng, detr, trends)
        for a, b in zip(got, again):
            assert np.array_equal(a, b)
        # NULL and one group remove them: the calls read plane 0 for every chain again
        assert eng.lib.gsm_sgs_set_groups(eng.h, None, 0) == 0
        plain = _loss_and_state(eng, detr, trends)
        assert _set_groups(eng, of, gc.G) == 0 and _set_groups(eng, np.zeros(of.size), 1) == 0
        for a, b in zip(plain, _loss_and_state(eng, detr, trends)):
            assert np.array_equal(a, b)
    finally:
        eng.close()
    assert got[1][1] > 0 and (got[1][[0, 2, 3, 4, 5]] == 0).all()
    assert not np.array_equal(got[0], plain[0])                                        # the groups' trends do differ
    assert np.array_equal(got[0][of == 0], plain[0][of == 0])                          # ... and group 0 is plane 0
    for g in np.unique(of):
        idx = np.flatnonzero(of == g)
        e1 = _engine(ch, idx.size)
        try:
            want = _loss_and_state(e1, detr[idx], trends[g])
            wf = _qt(e1, q[g], ref[g], detr[idx], 0)
            wi = _qt(e1, q[g], ref[g], wf, 1)
        finally:
            e1.close()
        for a, b in zip(got, want):
            assert np.array_equal(a[idx], b, equal_nan=True), g
        assert np.array_equal(fwd[idx], wf) and np.array_equal(inv[idx], wi)


@pytest.mark.parametrize("source", gc.SOURCES)
@pytest.mark.parametrize("cfg", gc.CFGS)
def test_grouped_run_equals_separate_runs(monkeypatch, cfg, source):
    monkeypatch.setenv("GSM_SGS_TAIL_QT", "1")                  # with a transformer: both transforms in the tail launch, at any chain count
    res, states, sep, sep_states = gc.grouped_and_separate(cfg, source, N_ITER)
    gc.assert_same_chains(res, states, sep, sep_states, source)
    rate = gc.acceptance(res)
    print(f"{cfg} {source}: acceptance rate {rate:.3f}")
    assert 0.05 < rate < 0.95
    assert not np.array_equal(res[0][0], res[1][0])


def test_stand_alone_transforms(monkeypatch):
    """trend + transformer with GSM_SGS_TAIL_QT=0 (the transforms as launches of their own)"""
    monkeypatch.setenv("GSM_SGS_TAIL_QT", "0")
    for source in ("pcg64", "replay"):
        out = gc.grouped_and_separate("qt", source, N_ITER)
        gc.assert_same_chains(*out, source)
        assert 0.05 < gc.acceptance(out[0]) < 0.95


@pytest.mark.parametrize("cfg", ("qt", "trend"))
def test_every_bed_kept(cfg):
    res, states, sep, sep_states = gc.grouped_and_separate(cfg, "pcg64", 12, only_save_last_bed=False)
    gc.assert_same_chains(res, states, sep, sep_states, "pcg64")
    assert res[0][0].shape == (12, gc.H, gc.H)


def test_above_the_batch_switch():
    """70 chains (more than 64: batches of 32, no draw-ahead, the tail launch's transforms by default) in 5 groups"""
    of = (np.arange(70) * 3) % 5
    res, states, sep, sep_states = gc.grouped_and_separate("qt", "pcg64", 8, of=of, n_groups=5)
    gc.assert_same_chains(res, states, sep, sep_states, "pcg64")


def test_posterior_over_grouped_chains():
    import test_gpu_sgs_posterior as tp
    from mcmc_gpu_amd import posterior
    n_iter, burn_in, thin = 25, 1, 3
    its = posterior.snapshot_iterations(n_iter, burn_in, thin)
    prob, trends, nst = gc.tables("qt")
    beds = gc.beds_of(prob, gc.OF.size)
    tmpl = gc.template(prob, trends[0], nst[0])
    groups = gc.groups_dict(gc.OF, trends, nst)
    idx = np.arange(gc.OF.size)
    for source in ("pcg64", "replay"):
        full = gc.run(tmpl, beds, idx, source, n_iter, groups=groups, only_save_last_bed=False)
        x = np.stack([r[0] for r in full[0]])[:, its]
        plain = gc.run(tmpl, beds, idx, source, n_iter, groups=groups)
        out = gc.run(tmpl, beds, idx, source, n_iter, groups=groups, posterior=dict(burn_in=burn_in, thin=thin))
        pc.check_maps(out[2], tp._reference(x, True), label=f"sgs groups {source}")
        gc.assert_same_chains(out[0], out[1], plain[0], plain[1], source)
        for c in idx:                                           # the kept beds carry the chain's own trend
            assert np.array_equal(full[0][c][0][-1], plain[0][c][0])


@pytest.mark.parametrize("cfg", gc.CFGS)
def test_one_group_is_no_groups(cfg):
    prob, trends, nst = gc.tables(cfg, 1)
    beds = gc.beds_of(prob, 3)
    tmpl = gc.template(prob, None if trends is None else trends[0], None if nst is None else nst[0])
    a = gc.run(tmpl, beds, np.arange(3), "pcg64", 12, groups=gc.groups_dict(np.zeros(3, dtype=int), trends, nst))
    b = gc.run(tmpl, beds, np.arange(3), "pcg64", 12)
    gc.assert_same_chains(a[0], a[1], b[0], b[1], "pcg64")


def test_handoff():
    from sklearn.preprocessing import QuantileTransformer
    from mcmc_gpu_amd import sgs
    prob, trends, nst = gc.tables("qt")
    tmpl = gc.template(prob, trends[0], nst[0])
    rng = np.random.default_rng(5)
    lsc = np.stack([prob["bed"] + rng.normal(0, 20.0, prob["bed"].shape) for _ in range(3)])
    lsc[1, 4:7, 5:9] = prob["surf"][4:7, 5:9] + 12.0                                   # above the surface: clamped
    of = np.array([1, 2, 2, 0])
    beds, groups = sgs.handoff(tmpl, lsc, of, sigma=3, n_quantiles=150, random_state=3)
    clamped = np.where((prob["surf"][None] - lsc) <= 0, prob["surf"][None] - 1, lsc)
    assert (clamped[1, 4:7, 5:9] == prob["surf"][4:7, 5:9] - 1).all() and set(groups) == {"of", "trend", "nst_trans"}
    for c, g in enumerate(of):
        assert np.array_equal(beds[c], clamped[g])
    assert np.array_equal(groups["of"], of) and np.array_equal(groups["trend"], sgs.trend_of(clamped, sigma=3))
    for g in range(3):
        fit = QuantileTransformer(n_quantiles=150, output_distribution="normal", subsample=None,
                                  random_state=3).fit((clamped[g] - groups["trend"][g]).reshape(-1, 1))
        assert np.array_equal(groups["nst_trans"][g].quantiles_, fit.quantiles_)
    rngs = [np.random.default_rng(70 + c) for c in range(4)]
    res, _ = sgs.run_many_sgs(tmpl, beds, rngs, 6, pcg64=True, groups=groups)
    assert len(res) == 4 and all(np.isfinite(r[0]).all() and np.isfinite(r[3]).all() for r in res)
    tmpl.set_normal_transformation(None, do_transform=False)                           # a template without a transformer gets no such key
    assert set(sgs.handoff(tmpl, lsc, of, sigma=3)[1]) == {"of", "trend"}
