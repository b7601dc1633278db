"""CPU-only: the bars of tests/krige_exact_common.py are fair -- a NumPy fp64 restatement of krige_solve's elimination order
(host_solve) stays within them on every case that tests/test_gpu_krige_exact.py holds the device to -- the cases reach the
regimes they are there for, and the extended-precision truth solves its own systems.  numpy.linalg.lstsq, the reference of the
standing comparisons, is measured against the same bars and printed, not asserted: it misses them at small n."""
import numpy as np
import pytest

import krige_exact_common as kx


def _worst(recs, pick):
    """Largest error / bar of the (est, var) `pick` takes from a Rec, over the cells below the refusal threshold."""
    e = v = 0.0
    for r in recs:
        if r.kappa > kx.KAPPA_REFUSE:
            continue
        got = pick(r)
        assert got is not None, f"the restatement refuses a system of condition number {r.kappa:.2e}"
        e = max(e, float(abs(kx.LD(got[0]) - r.est) / r.b_est))
        v = max(v, float(abs(kx.LD(got[1]) - r.var) / r.b_var))
    return e, v


def _hold(what, recs):
    (he, hv), (le, lv) = _worst(recs, lambda r: r.host), _worst(recs, lambda r: r.lstsq)
    ks = [r.kappa for r in recs]
    print(f"\n{what}: cond {min(ks):.1e} .. {max(ks):.1e}: restatement est {he:.3f} var {hv:.3f} of the bar; lstsq est {le:.2f} var {lv:.2f}")
    assert he <= 1.0 and hv <= 1.0, (what, he, hv)
    return he, hv, le, lv


@pytest.mark.parametrize("mid", sorted(kx.MODELS))
def test_restatement_meets_the_bars_with_one_lag_table(mid):
    worst = [_hold(f"{mid} layout {lid} {kt}", kx.truth(lid, mid, kt)) for lid in kx.LAYOUTS for kt in kx.KTYPES]
    print(f"{mid}: largest ratio, restatement {max(max(w[:2]) for w in worst):.3f}, lstsq {max(max(w[2:]) for w in worst):.2f}")


@pytest.mark.parametrize("maps", ["constant", "smooth"])
@pytest.mark.parametrize("vtype", kx.LOCAL_VTYPES)
def test_restatement_meets_the_bars_with_a_variogram_per_cell(vtype, maps):
    """The restatement forms its entries in fp64 in krige_fill_local's expression order, the truth in long double."""
    worst = [_hold(f"{vtype} {maps} maps layout {lid} {kt}", kx.truth_local(lid, vtype, maps, kt)) for lid in kx.LAYOUTS for kt in kx.KTYPES]
    print(f"{vtype} {maps}: largest ratio, restatement {max(max(w[:2]) for w in worst):.3f}, lstsq {max(max(w[2:]) for w in worst):.2f}")


@pytest.mark.parametrize("kt", kx.KTYPES)
def test_restatement_meets_the_bars_in_cross_validation(kt):
    for name, recs in zip(kx.CV_MODELS, kx.cv_truth(kt)):
        _hold(f"leave-one-out {name} {kt}", recs)
    for (vtype, maps), recs in zip(kx.CV_LOCAL, kx.cv_truth_local(kt)):
        _hold(f"leave-one-out {vtype} {maps} maps {kt}", recs)


def test_cases_reach_their_regimes():
    ns, kappas, wide = set(), [], 0
    for lid in kx.LAYOUTS:
        L = kx.layout(lid)
        assert L["cells"].size <= kx.MAX_CELLS and np.isnan(L["grid"].ravel()[L["cells"]]).all()
        wide += sum(w > 0 for _, _, w in L["nb"])
        for kt in kx.KTYPES:
            for mid in kx.MODELS:
                recs = kx.truth(lid, mid, kt)
                assert len(recs) == L["cells"].size and all(np.isfinite(r.kappa) for r in recs)
                ns |= {r.n for r in recs}
                kappas += [r.kappa for r in recs]
    assert ns >= {1, 2, 3, 4, 5, 6, 7, 8, 16, 48}, sorted(ns)
    assert min(kappas) < 10 and max(kappas) > 1e10 and wide >= 1
    assert any(kx.KAPPA_REFUSE < k < kx.KAPPA_FINITE for k in kappas)           # the refused-or-finite clause is exercised
    yy = kx.layout("d")["yy"]
    assert yy[1, 0] < yy[0, 0] and kx.layout("c")["num_points"] == 20
    # cross-validation: one search for eight models whose systems differ by ten orders of conditioning
    cv = [[r.kappa for r in recs] for recs in kx.cv_truth("ok")]
    print(f"\nleave-one-out: cond per model {[f'{max(k):.1e}' for k in cv]}")
    assert len(cv) == 8 and max(map(max, cv)) / min(map(max, cv)) > 1e10


def test_truth_solves_its_own_systems():
    """The long-double residual of every truth is at most 2^-60 ||A|| ||w*||."""
    worst = 0.0
    for kt in kx.KTYPES:
        groups = [kx.truth(lid, mid, kt) for lid in kx.LAYOUTS for mid in kx.MODELS]
        groups += [kx.truth_local(lid, vt, maps, kt) for lid in kx.LAYOUTS for vt in kx.LOCAL_VTYPES for maps in ("constant", "smooth")]
        groups += kx.cv_truth(kt) + kx.cv_truth_local(kt)
        worst = max([worst] + [r.resid for g in groups for r in g])
    print(f"\nlargest residual of the truth: {worst / 2.0 ** -60:.3f} x 2^-60 ||A|| ||w*||")
    assert worst <= 2.0 ** -60
