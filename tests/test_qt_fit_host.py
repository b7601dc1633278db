"""CPU: what the device fit of the normal-score transformers (gsm_qt_fit, sgs.fit_normal_scores, sgs.handoff(fit=)) is held to, and
the parts of it that run without a GPU.

  * tests/qt_fit_common.restate -- the NumPy form of the arithmetic include/gsm.h states for gsm_qt_fit -- equals scikit-learn's
    QuantileTransformer.fit on every case with at least nq values: quantiles_, references_ and n_quantiles_ by np.array_equal;
  * a transformer assembled from the tables transforms and inverts with the bits of the fitted one;
  * sgs.fit_normal_scores(device=False) is the per-field fit, and its refusals; sgs.handoff(fit='host') is sgs.handoff();
  * mcmc_gpu_amd/csrc/sort_device.h on the host (tests/native/sort_device_check.cpp, a stand-alone g++ program; it also builds
    and passes with -fsanitize=address,undefined): the key mapping, the merge-path partition and the sort's geometry."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import qt_fit_common as qc
import sgs_groups_common as gc

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("cells", qc.SIZES, ids=qc.case_id)
def test_restatement_equals_scikit_learn(cells):
    compared = 0
    for nq in qc.nqs(cells):
        for r, f in enumerate(qc.fields(cells)):
            if np.count_nonzero(~np.isnan(f)) < nq:
                continue
            fit = qc.sklearn_fit(f, nq)
            assert fit.n_quantiles_ == nq
            assert np.array_equal(fit.references_, np.linspace(0, 1, nq, endpoint=True))
            assert fit.quantiles_.shape == (nq, 1)
            assert np.array_equal(qc.restate(f, nq), fit.quantiles_[:, 0]), (cells, nq, r)
            compared += 1
    assert compared >= (1 if cells >= 2 else 0)


def test_cases_are_what_they_claim():
    assert len(set(qc.SIZES)) == len(qc.SIZES) and all(t + d in qc.SIZES for t in (qc.TILE,) for d in (-1, 0, 1)) and 2 * qc.TILE + 1 in qc.SIZES
    kinds = {qc.case_id(c).split("-", 1)[1] for c in qc.SIZES}
    assert kinds == set(qc.CONTENTS)
    for cells in qc.SIZES:
        f = qc.fields(cells)
        nan = np.isnan(f).sum(axis=1)
        assert nan[0] == 0 and nan[2] == cells and not np.isinf(f).any()
        if cells >= 2:
            assert f.shape[0] == 4 and 0 < nan[1] < cells and nan[3] == cells - 1
    z = qc.fields(qc.SIZES[8 + 12 * 3])
    assert qc.case_id(z.shape[1]).endswith("zeros_subnormals") and np.signbit(z[0][z[0] == 0]).any() and not np.signbit(z[0][z[0] == 0]).all()
    assert (np.abs(z[0][z[0] != 0]) < 2.3e-308).any()
    # a row of NaN for a field without values, and ties give a table with equal entries
    assert np.isnan(qc.restate(np.full(5, np.nan), 3)).all()
    assert np.array_equal(qc.restate(np.array([2.0, 2.0, np.nan, 2.0]), 3), [2.0, 2.0, 2.0])


@pytest.mark.parametrize("cells", [37, 1025, 100 * 130])
def test_assembled_transformer_has_the_bits_of_the_fitted_one(cells):
    rng = np.random.default_rng(cells)
    for nq in qc.nqs(cells):
        for f in qc.fields(cells)[:2]:
            if np.count_nonzero(~np.isnan(f)) < nq:
                continue
            fit = qc.sklearn_fit(f, nq, random_state=4)
            made = qc.assembled(qc.restate(f, nq), nq, random_state=4)
            lo, hi = np.nanmin(f), np.nanmax(f)
            x = np.concatenate([f[~np.isnan(f)][:500], rng.uniform(lo - 1.0, hi + 1.0, 200), [lo, hi, np.nan]]).reshape(-1, 1)
            z = fit.transform(x)
            assert np.array_equal(made.transform(x), z, equal_nan=True)
            s = np.concatenate([z[:, 0], rng.normal(0, 2, 200), [-9.0, 9.0]]).reshape(-1, 1)
            assert np.array_equal(made.inverse_transform(s), fit.inverse_transform(s), equal_nan=True)


def test_fit_normal_scores_on_the_host():
    from mcmc_gpu_amd import sgs
    x = np.random.default_rng(3).normal(5.0, 40.0, (3, 20, 31))
    x[1, 3, 4:9] = np.nan
    got = sgs.fit_normal_scores(x, n_quantiles=150, random_state=2, device=False)
    assert len(got) == 3
    for t, f in zip(got, x):
        fit = qc.sklearn_fit(f, 150, random_state=2)
        assert sgs._is_device_qt(t) and t.n_quantiles_ == 150 and t.random_state == 2
        assert np.array_equal(t.quantiles_, fit.quantiles_) and np.array_equal(t.references_, fit.references_)
    one = sgs.fit_normal_scores(x[2], n_quantiles=150, device=False)                       # [H, W]: one field
    assert len(one) == 1 and np.array_equal(one[0].quantiles_, got[2].quantiles_)
    flat = sgs.fit_normal_scores(x.reshape(3, -1), n_quantiles=150, device=False, stack=True)      # [n, cells]
    assert len(flat) == 3 and all(np.array_equal(a.quantiles_, b.quantiles_) for a, b in zip(flat, got))
    assert np.array_equal(sgs.quantile_probabilities(1000), qc.probabilities(1000))
    with pytest.raises(ValueError, match="above the 620 cells"):
        sgs.fit_normal_scores(x, n_quantiles=621, device=False)
    with pytest.raises(ValueError, match="at least 2"):
        sgs.fit_normal_scores(x, n_quantiles=1, device=False)
    for bad in (np.inf, -np.inf):
        y = x.copy()
        y[2, 0, 0] = bad
        with pytest.raises(ValueError, match="infinity"):
            sgs.fit_normal_scores(y, n_quantiles=150, device=False)
    with pytest.raises(ValueError, match="fields must be"):
        sgs.fit_normal_scores(x[0, 0], device=False)
    with pytest.raises(ValueError, match="fields must be"):
        sgs.fit_normal_scores(x, device=False, stack=True)
    import torch
    with pytest.raises(ValueError, match="tensor"):
        sgs.fit_normal_scores(torch.zeros((2, 8, 8), dtype=torch.float64), n_quantiles=10, device=False)


def test_handoff_fit_keyword_on_the_host():
    from mcmc_gpu_amd import sgs
    prob, trends, nst = gc.tables("qt")
    tmpl = gc.template(prob, trends[0], nst[0])
    lsc = np.stack([prob["bed"] + 10.0 * g for g in range(2)])
    kw = dict(sigma=2, n_quantiles=100, random_state=1, device=False)
    beds, groups = sgs.handoff(tmpl, lsc, [1, 0, 1], **kw)
    beds_h, groups_h = sgs.handoff(tmpl, lsc, [1, 0, 1], fit="host", **kw)
    assert set(groups) == set(groups_h) == {"of", "trend", "nst_trans"}
    assert all(np.array_equal(a, b) for a, b in zip(beds, beds_h))
    assert np.array_equal(groups["of"], groups_h["of"]) and np.array_equal(groups["trend"], groups_h["trend"])
    for a, b in zip(groups["nst_trans"], groups_h["nst_trans"]):
        assert np.array_equal(a.quantiles_, b.quantiles_) and np.array_equal(a.references_, b.references_) and a.get_params() == b.get_params()
    with pytest.raises(ValueError, match="device"):
        sgs.handoff(tmpl, lsc, [1, 0, 1], fit="device", **kw)
    with pytest.raises(ValueError, match="'host' or 'device'"):
        sgs.handoff(tmpl, lsc, [1, 0, 1], fit="gpu", **kw)


def test_c_abi_declares_the_fit():
    from mcmc_gpu_amd import _lib
    assert "gsm_qt_fit" in _lib.declared_symbols()
    assert "qt_fit_kernel.hip" in _lib.SOURCES and "gsm_api_qt.hip" in _lib.SOURCES


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_sort_header_on_the_host(tmp_path):
    exe = tmp_path / "sort_device_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", str(ROOT / "mcmc_gpu_amd" / "csrc"), "-o", str(exe),
                    str(ROOT / "tests" / "native" / "sort_device_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sort device ok" in r.stdout
