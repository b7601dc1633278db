"""GPU: gsm_qt_fit (csrc/qt_fit_kernel.hip) through the C ABI, sgs.fit_normal_scores(device=True) and sgs.handoff(fit='device').
Every check is an equality (tests/qt_fit_common.py: the cases and the NumPy restatement, shown equal to scikit-learn bit for bit by
tests/test_qt_fit_host.py).

Per case, a batch of 3 or 4 fields in one call and every table length of the case: n_valid and n_inf are NumPy's counts; `sorted` is
np.sort of the values that are not NaN, then NaN; `quantiles` is the restatement's table and scikit-learn's quantiles_; each field of
the batch equals the one-field call bit for bit; the same call twice gives the same bits; x is unchanged; a handle made for another grid
gives the same bits.  The refusals return GSM_E_ARG and launch nothing."""
import ctypes as C

import numpy as np
import pytest

import qt_fit_common as qc
import sgs_groups_common as gc

pytestmark = pytest.mark.gpu
GSM_E_ARG = -1


def _engine(H=1, W=1):
    from mcmc_gpu_amd.engine import GsmEngine
    return GsmEngine(H, W, 1)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _fit(eng, d_x, nq, want_sorted=True):
    """(quantiles, n_valid, n_inf, sorted) of one call as arrays"""
    import torch
    out = eng.qt_fit(d_x, qc.probabilities(nq), want_sorted=want_sorted)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in out)


@pytest.mark.parametrize("cells", qc.SIZES, ids=qc.case_id)
def test_tables_counts_and_sort_equal_numpy_and_scikit_learn(cells):
    import torch
    x = qc.fields(cells)
    eng, other = _engine(), _engine(7, 45)
    try:
        d_x = torch.as_tensor(x.copy()).to(eng.dev)
        for nq in qc.nqs(cells):
            quant, n_valid, n_inf, srt = _fit(eng, d_x, nq)
            assert np.array_equal(d_x.cpu().numpy().view(np.uint64), _bits(x))                     # the input is only read
            assert np.array_equal(n_valid, np.count_nonzero(~np.isnan(x), axis=1)) and np.array_equal(n_inf, np.isinf(x).sum(axis=1))
            for r, (f, (want, sk)) in enumerate(zip(x, qc.reference(cells, nq))):
                m = int(n_valid[r])
                assert np.array_equal(srt[r, :m], np.sort(f[~np.isnan(f)])) and np.isnan(srt[r, m:]).all(), (nq, r)
                assert np.array_equal(quant[r], want, equal_nan=m == 0), (nq, r)
                if m == 0:
                    assert np.isnan(quant[r]).all()
                if sk is not None:
                    assert np.array_equal(quant[r], sk), (nq, r)
                one = _fit(eng, d_x[r:r + 1], nq)                                                   # the one-field call: the same bits
                assert np.array_equal(_bits(one[0][0]), _bits(quant[r])) and np.array_equal(_bits(one[3][0]), _bits(srt[r]))
                assert one[1][0] == n_valid[r] and one[2][0] == n_inf[r]
            again = _fit(eng, d_x, nq)
            assert all(np.array_equal(_bits(a) if a.dtype == np.float64 else a, _bits(b) if b.dtype == np.float64 else b)
                       for a, b in zip(again, (quant, n_valid, n_inf, srt)))
            elsewhere = _fit(other, d_x, nq, want_sorted=False)                                     # `cells` is the call's own
            assert np.array_equal(_bits(elsewhere[0]), _bits(quant)) and np.array_equal(elsewhere[1], n_valid) and elsewhere[3] is None
    finally:
        eng.close()
        other.close()


def test_infinities_are_counted_and_sorted_to_the_ends():
    import torch
    x = np.random.default_rng(8).normal(0, 1, (2, 5000))
    x[0, [3, 4097, 4999]] = [np.inf, -np.inf, np.inf]
    x[0, 17] = np.nan
    eng = _engine()
    try:
        quant, n_valid, n_inf, srt = _fit(eng, torch.as_tensor(x).to(eng.dev), 3)
    finally:
        eng.close()
    assert n_valid.tolist() == [4999, 5000] and n_inf.tolist() == [3, 0]
    assert srt[0, 0] == -np.inf and (srt[0, 4997:4999] == np.inf).all() and np.isnan(srt[0, 4999])
    assert np.array_equal(srt[0, :4999], np.sort(x[0][~np.isnan(x[0])]))
    # NumPy's arithmetic on infinities (inf * 0, inf - inf), NaN included, and np.maximum.accumulate's NaN that stays
    assert np.array_equal(quant[0], qc.restate(x[0], 3), equal_nan=True) and np.array_equal(quant[1], qc.restate(x[1], 3))


def _raw(eng, x, n, cells, q, nq, quantiles, n_valid, n_inf, srt):
    import torch
    vp = lambda t: C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr())
    qp = C.POINTER(C.c_double)() if q is None else q.ctypes.data_as(C.POINTER(C.c_double))
    with torch.cuda.device(eng.dev):
        return eng.lib.gsm_qt_fit(eng.h, vp(x), n, cells, qp, nq, vp(quantiles), vp(n_valid), vp(n_inf), vp(srt), eng._stream())


def test_refusals():
    import torch
    n, cells, nq = 2, 300, 10
    eng = _engine()
    try:
        x = torch.zeros((n, cells), dtype=torch.float64, device=eng.dev)
        qt = torch.full((n, nq), 7.0, dtype=torch.float64, device=eng.dev)
        srt = torch.full((n, cells), 7.0, dtype=torch.float64, device=eng.dev)
        nv = torch.full((n,), 7, dtype=torch.int64, device=eng.dev)
        ni = torch.full((n,), 7, dtype=torch.int64, device=eng.dev)
        q = qc.probabilities(nq)
        down, above, below, nan = q[::-1].copy(), q.copy(), q.copy(), q.copy()
        above[-1], below[0], nan[4] = 1.0 + 2.0 ** -52, -5e-324, np.nan
        bad = [
            _raw(eng, None, n, cells, q, nq, qt, nv, ni, srt),
            _raw(eng, x, n, cells, None, nq, qt, nv, ni, srt),
            _raw(eng, x, n, cells, q, nq, None, nv, ni, srt),
            _raw(eng, x, n, cells, q, nq, qt, None, ni, srt),
            _raw(eng, x, n, cells, q, nq, qt, nv, None, srt),
            _raw(eng, x, n, cells, q, nq, x, nv, ni, srt),                      # quantiles aliases x
            _raw(eng, x, n, cells, q, nq, qt, nv, ni, x),                       # sorted aliases x
            _raw(eng, x, 0, cells, q, nq, qt, nv, ni, srt),
            _raw(eng, x, -1, cells, q, nq, qt, nv, ni, srt),
            _raw(eng, x, n, 0, q, nq, qt, nv, ni, srt),
            _raw(eng, x, n, (1 << 24) + 1, q, nq, qt, nv, ni, srt),
            _raw(eng, x, n, cells, q, 1, qt, nv, ni, srt),
            _raw(eng, x, n, cells, q, (1 << 20) + 1, qt, nv, ni, srt),
            _raw(eng, x, n, cells, down, nq, qt, nv, ni, srt),
            _raw(eng, x, n, cells, above, nq, qt, nv, ni, srt),
            _raw(eng, x, n, cells, below, nq, qt, nv, ni, srt),
            _raw(eng, x, n, cells, nan, nq, qt, nv, ni, srt),
        ]
        assert bad == [GSM_E_ARG] * len(bad)
        assert b"gsm_qt_fit" in eng.lib.gsm_last_error(eng.h)
        torch.cuda.synchronize()
        assert bool((qt == 7.0).all()) and bool((srt == 7.0).all()) and bool((nv == 7).all()) and bool((ni == 7).all())      # nothing was launched
        assert _raw(eng, x, n, cells, q, nq, qt, nv, ni, None) == 0                                                           # sorted may be NULL
        torch.cuda.synchronize()
        assert bool((qt == 0.0).all()) and nv.tolist() == [cells] * n and ni.tolist() == [0] * n and bool((srt == 7.0).all())
    finally:
        eng.close()


def test_fit_normal_scores_on_the_device():
    import torch
    from mcmc_gpu_amd import sgs
    x = np.random.default_rng(12).normal(-200.0, 35.0, (3, 64, 64))
    x[1, 5, 7:30] = np.nan
    host = sgs.fit_normal_scores(x, n_quantiles=1000, random_state=6, device=False)
    for given in (x, torch.as_tensor(x).to("cuda")):
        got = sgs.fit_normal_scores(given, n_quantiles=1000, random_state=6, device=True)
        assert len(got) == 3
        for t, ref in zip(got, host):
            assert sgs._is_device_qt(t) and t.n_quantiles_ == ref.n_quantiles_ == 1000 and t.n_features_in_ == ref.n_features_in_ == 1
            assert t.get_params() == ref.get_params()
            assert np.array_equal(t.quantiles_, ref.quantiles_) and t.quantiles_.shape == (1000, 1) and np.array_equal(t.references_, ref.references_)
            probe = np.linspace(-400.0, 0.0, 777).reshape(-1, 1)
            assert np.array_equal(t.transform(probe), ref.transform(probe))
    auto = sgs.fit_normal_scores(x[0], n_quantiles=150)                             # device=None with a GPU: the kernels
    assert len(auto) == 1 and np.array_equal(auto[0].quantiles_[:, 0], qc.restate(x[0], 150))
    y = x.copy()
    y[2, 1, 1] = -np.inf
    with pytest.raises(ValueError, match="infinity"):
        sgs.fit_normal_scores(y, n_quantiles=150, device=True)
    with pytest.raises(ValueError, match="above the 4096 cells"):
        sgs.fit_normal_scores(x, n_quantiles=4097, device=True)


def test_handoff_with_the_fit_on_the_device():
    """the set-up of tests/test_gpu_sgs_groups.py::test_handoff"""
    from mcmc_gpu_amd import sgs
    prob, trends, nst = gc.tables("qt")
    tmpl = gc.template(prob, trends[0], nst[0])
    rng = np.random.default_rng(5)
    lsc = np.stack([prob["bed"] + rng.normal(0, 20.0, prob["bed"].shape) for _ in range(3)])
    lsc[1, 4:7, 5:9] = prob["surf"][4:7, 5:9] + 12.0
    of = np.array([1, 2, 2, 0])
    kw = dict(sigma=3, n_quantiles=150, random_state=3)
    beds_h, groups_h = sgs.handoff(tmpl, lsc, of, fit="host", **kw)
    beds_d, groups_d = sgs.handoff(tmpl, lsc, of, fit="device", **kw)
    assert set(groups_d) == set(groups_h) == {"of", "trend", "nst_trans"}
    assert all(np.array_equal(a, b) for a, b in zip(beds_h, beds_d))
    assert np.array_equal(groups_d["of"], groups_h["of"]) and np.array_equal(groups_d["trend"], groups_h["trend"])
    for g in range(3):
        assert np.array_equal(groups_d["nst_trans"][g].quantiles_, groups_h["nst_trans"][g].quantiles_)
        assert np.array_equal(groups_d["nst_trans"][g].references_, groups_h["nst_trans"][g].references_)
    runs = []
    for beds, groups in ((beds_h, groups_h), (beds_d, groups_d)):
        rngs = [np.random.default_rng(70 + c) for c in range(4)]
        res, _ = sgs.run_many_sgs(tmpl, beds, rngs, 6, pcg64=True, groups=groups)
        runs.append((res, [r.bit_generator.state for r in rngs]))
    gc.assert_same_chains(runs[0][0], runs[0][1], runs[1][0], runs[1][1], "pcg64")
    assert all(np.isfinite(r[0]).all() for r in runs[1][0])
    with pytest.raises(ValueError, match="device"):
        sgs.handoff(tmpl, lsc, of, fit="device", device=False, **kw)
    tmpl.set_normal_transformation(None, do_transform=False)                        # a template without a transformer gets no such key
    assert set(sgs.handoff(tmpl, lsc, of, sigma=3, fit="device")[1]) == {"of", "trend"}
