"""Host suite of the posterior region functionals (mcmc_gpu_amd/posterior.py `regions`): the option check, the bit plane, the
summary's region_values / region_stats / hypsometry on a synthetic stack against direct NumPy, save / load, and the rank merge.
No GPU."""
import numpy as np
import pytest

import posterior_regions_common as rg
from mcmc_gpu_amd import _lib, posterior

H, W, C, T = 12, 17, 3, 9
RES = 500.0


def _masks():
    m = np.zeros((3, H, W), dtype=bool)
    m[0] = True
    m[1, 2:9, 3:11] = True
    m[2, 5:, 8:] = True
    return m


def test_option_and_symbol():
    assert "regions" in posterior.POSTERIOR_KEYS
    assert "gsm_posterior_regions" in _lib.declared_symbols()
    ok = dict(burn_in=0, thin=10)
    assert posterior.check_options(ok, 100)["regions"] is None
    opt = posterior.check_options(dict(ok, regions=dict(masks=_masks())), 100)["regions"]
    assert opt["masks"].shape == (3, H, W) and opt["masks"].dtype == bool and opt["names"] == ("region0", "region1", "region2")
    assert (opt["sea_level"], opt["rho_ice"], opt["rho_water"], opt["hyps"]) == (0.0, 917.0, 1028.0, None)
    again = posterior.check_regions(opt, H, W)                                   # what check_options returns is accepted again
    assert np.array_equal(again["masks"], opt["masks"]) and again["names"] == opt["names"]
    for rhat in (True, False):                                                   # beside rhat on or off and every other option
        full = posterior.check_options(dict(ok, rhat=rhat, hist=dict(half_width=10.0), local=True, residual=True,
                                            regions=dict(masks=_masks(), hyps=dict(lo=-100, hi=100, bins=8))), 100)
        assert full["regions"]["hyps"] == dict(lo=-100.0, hi=100.0, bins=8) and full["local"] == dict(reach=1)
    with pytest.raises(ValueError, match="unknown posterior option"):
        posterior.check_options(dict(ok, region=dict(masks=_masks())), 100)


def test_check_regions_accepts_masks_and_labels():
    m = _masks()
    assert np.array_equal(posterior.check_regions(dict(masks=m))["masks"], m)
    assert posterior.check_regions(dict(masks=m[1]))["masks"].shape == (1, H, W)           # one bool mask
    assert np.array_equal(posterior.check_regions(dict(masks=m.astype(np.float64) * 3.0))["masks"], m)   # non-zero = inside
    labels = np.zeros((H, W), dtype=np.int32)
    labels[2:5] = 1
    labels[7:9, 3:] = 3                                                                     # label 2 is unused: an empty region
    got = posterior.check_regions(dict(masks=labels, names=("a", "b", "c")), H, W)
    assert got["names"] == ("a", "b", "c") and got["masks"].shape == (3, H, W)
    assert np.array_equal(got["masks"][0], labels == 1) and not got["masks"][1].any() and np.array_equal(got["masks"][2], labels == 3)
    r = posterior.check_regions(dict(masks=m, sea_level=-2, rho_ice=900, rho_water=1000.0, hyps=dict(lo=0, hi=64, bins=np.int64(64))))
    assert (r["sea_level"], r["rho_ice"], r["rho_water"]) == (-2.0, 900.0, 1000.0) and r["hyps"] == dict(lo=0.0, hi=64.0, bins=64)
    assert posterior.check_regions(None) is None
    bits = posterior.region_bits(m)
    assert bits.dtype == np.uint8 and bits.shape == (H, W)
    for k in range(3):
        assert np.array_equal((bits >> k) & 1, m[k])
    assert np.array_equal(posterior.region_bits(np.ones((8, 2, 2), dtype=bool)), np.full((2, 2), 255, dtype=np.uint8))


@pytest.mark.parametrize("bad,match", [
    (dict(masks=np.ones((9, H, W), dtype=bool)), "at most 8"),
    (dict(masks=np.full((H, W), 9, dtype=np.int64)), "at most 8"),
    (dict(masks=np.ones((2, H + 1, W), dtype=bool)), "the grid is"),
    (dict(masks=np.ones((H, W + 1), dtype=np.int32)), "the grid is"),
    (dict(masks=np.ones((2, 2, H, W), dtype=bool)), "shape"),
    (dict(masks=np.zeros((H, W), dtype=np.int32)), "shape"),                                 # no label above 0: no region
    (dict(masks=-np.ones((H, W), dtype=np.int32)), ">= 0"),
    (dict(masks=_masks(), hyps=dict(lo=0, hi=10, bins=7)), "even"),
    (dict(masks=_masks(), hyps=dict(lo=0, hi=10, bins=66)), "even"),
    (dict(masks=_masks(), hyps=dict(lo=0, hi=10, bins=0)), "even"),
    (dict(masks=_masks(), hyps=dict(lo=10, hi=10, bins=8)), "lo < hi"),
    (dict(masks=_masks(), hyps=dict(lo=10, hi=-10, bins=8)), "lo < hi"),
    (dict(masks=_masks(), hyps=dict(lo=0, hi=np.inf, bins=8)), "lo < hi"),
    (dict(masks=_masks(), hyps=dict(lo=0, hi=10)), "keys"),
    (dict(masks=_masks(), rho_ice=0.0), "rho_ice"),
    (dict(masks=_masks(), rho_water=-1028.0), "rho_water"),
    (dict(masks=_masks(), rho_ice=np.nan), "rho_ice"),
    (dict(masks=_masks(), sea_level=np.inf), "sea_level"),
    (dict(masks=_masks(), names=("a", "b")), "names"),
    (dict(masks=_masks(), level=0.0), "unknown regions option"),
    (dict(names=("a",)), "needs masks"),
    (True, "regions must be"),
])
def test_check_regions_refuses(bad, match):
    with pytest.raises(ValueError, match=match):
        posterior.check_regions(bad, H, W)


def test_hypsometry_count_limit():
    posterior.check_region_count(1024, 1024, 2000, 0, 1, split=False)          # 2^20 cells x 2000 snapshots < 2^31
    with pytest.raises(ValueError, match="int32"):
        posterior.check_region_count(1024, 1024, 2049, 0, 1, split=False)


def _stack(split, with_hyps=True):
    """A summary built by hand from a synthetic stack x [C, T, H, W] through the restatement: (summary, x, surf, masks)."""
    rng = np.random.default_rng(3)
    surf = 300.0 + rng.normal(0, 80, (H, W))
    x = rng.normal(0, 150, (C, T, H, W)) + np.linspace(-100, 100, C)[:, None, None, None]
    x[1, 4, 3, 4] = np.nan
    m = np.concatenate([_masks(), np.zeros((1, H, W), dtype=bool)])             # the last region is empty
    K = m.shape[0]
    func = np.stack([rg.reference(x[:, t], surf, m, 0.0, rg.RATIO)[0].astype(np.float64) for t in range(T)], axis=2)
    assert func.shape == (C, K, T, 8)
    N = T // 2 if split else T
    used = x[:, T - (2 * N if split else N):]
    hy = sum(rg.hyps_reference(used[:, t], surf, m, -256.0, 8 / 512.0, 8) for t in range(used.shape[1]))
    z = np.zeros((H, W))
    s = posterior.PosteriorSummary(mean=z, sd=z, rhat=None, within_var=None, between_var_over_n=None, n_chains=C, n_sequences=C * (2 if split else 1),
                                   n_per_sequence=N, snapshot_iterations=np.arange(T), burn_in=0, thin=1, split=split, region_func=func,
                                   region_masks=m, region_names=("all", "a", "b", "none"), region_sea_level=0.0,
                                   region_density_ratio=rg.RATIO, region_resolution=RES,
                                   region_hyps=hy if with_hyps else None,
                                   region_hyps_range=np.array([-256.0, 256.0]) if with_hyps else None)
    return s, x, surf, m


@pytest.mark.parametrize("split", [True, False])
def test_summary_against_numpy(split):
    s, x, surf, m = _stack(split)
    K = m.shape[0]
    thick = np.maximum(surf - x, 0.0)
    haf = np.maximum((surf - x) + rg.RATIO * np.minimum(x - 0.0, 0.0), 0.0)
    valid = np.isfinite(x)
    direct = dict(count=lambda k: (valid & m[k]).sum(axis=(2, 3)).astype(float),
                  volume=lambda k: np.where(valid & m[k], thick, 0.0).sum(axis=(2, 3)) * RES ** 2,
                  volume_above_flotation=lambda k: np.where(valid & m[k], haf, 0.0).sum(axis=(2, 3)) * RES ** 2,
                  area_below_sea_level=lambda k: (valid & m[k] & (x < 0)).sum(axis=(2, 3)) * RES ** 2,
                  area_marine_grounded=lambda k: (valid & m[k] & (x < 0) & (haf > 0)).sum(axis=(2, 3)) * RES ** 2)
    for what, fn in direct.items():
        got = s.region_values(what)
        assert got.shape == (C, K, T)
        for k in range(K):
            np.testing.assert_allclose(got[:, k], fn(k), rtol=1e-13, atol=0, err_msg=f"{what} region {k}")
    with np.errstate(invalid="ignore"):
        for k in range(K - 1):
            xm = np.where(valid & m[k], x, np.nan)
            assert np.array_equal(s.region_values("min_bed")[:, k], np.nanmin(xm, axis=(2, 3)))
            assert np.array_equal(s.region_values("max_bed")[:, k], np.nanmax(xm, axis=(2, 3)))
            np.testing.assert_allclose(s.region_values("mean_bed")[:, k], np.nanmean(xm, axis=(2, 3)), rtol=1e-12)
    for what in ("min_bed", "max_bed", "mean_bed"):                              # an empty region has no extreme and no mean
        assert np.isnan(s.region_values(what)[:, K - 1]).all()
    assert (s.region_values("count")[:, K - 1] == 0).all() and (s.region_values("volume")[:, K - 1] == 0).all()
    with pytest.raises(KeyError):
        s.region_values("area")
    # the statistics over the M N values: the snapshots a split drops are left out, every chain cut into its sequences
    N = s.n_per_sequence
    first = T - N * (2 if split else 1)
    st = s.region_stats()
    assert set(st) == set(posterior.REGION_QUANTITIES)
    for what in ("volume", "volume_above_flotation", "area_marine_grounded", "min_bed"):
        v = s.region_values(what)[:, :, first:]                                  # [C, K, used]
        for k in range(K - 1):
            flat = v[:, k].ravel()
            got = st[what]
            np.testing.assert_allclose(got["mean"][k], flat.mean(), rtol=1e-13)
            np.testing.assert_allclose(got["sd"][k], flat.std(ddof=1), rtol=1e-10)
            np.testing.assert_allclose([got["q025"][k], got["q50"][k], got["q975"][k]], np.quantile(flat, [0.025, 0.5, 0.975]), rtol=1e-13)
            seq = v[:, k].reshape(-1, N)                                          # a chain's halves are consecutive sequences
            Wv, Bn = seq.var(axis=1, ddof=1).mean(), seq.mean(axis=1).var(ddof=1)
            np.testing.assert_allclose(got["rhat"][k], np.sqrt(((N - 1) / N * Wv + Bn) / Wv), rtol=1e-10)
    assert np.isnan(st["min_bed"]["mean"][K - 1]) and st["count"]["mean"][K - 1] == 0 and np.isnan(st["count"]["rhat"][K - 1])
    # hypsometry: bin edges, per-chain mean area per slot, pooled mean curve
    hy = s.hypsometry()
    assert np.array_equal(hy["edges"], np.linspace(-256.0, 256.0, 9)) and hy["area"].shape == (C, K, 10) and hy["mean"].shape == (K, 10)
    used = x[:, first:]
    for k in range(K):
        sel = valid[:, first:] & m[k]
        for c in range(C):
            xs = used[c][sel[c]]
            cnt = np.concatenate([[(xs < -256).sum()], np.histogram(xs, bins=hy["edges"][:-1].tolist() + [256.0 - 1e-9])[0], [(xs >= 256).sum()]])
            np.testing.assert_allclose(hy["area"][c, k], cnt / used.shape[1] * RES ** 2, rtol=1e-13, err_msg=f"hypsometry chain {c} region {k}")
        np.testing.assert_allclose(hy["area"][:, k].sum(axis=1), sel.sum(axis=(1, 2, 3)) / used.shape[1] * RES ** 2, rtol=1e-13)
    np.testing.assert_allclose(hy["mean"], hy["area"].mean(axis=0), rtol=1e-15)


def test_summary_without_regions_or_hypsometry():
    z = np.zeros((2, 2))
    bare = posterior.PosteriorSummary(mean=z, sd=z, rhat=None, within_var=None, between_var_over_n=None, n_chains=1, n_sequences=1, n_per_sequence=2,
                                      snapshot_iterations=np.arange(2), burn_in=0, thin=1, split=False)
    for call in (lambda: bare.region_values("volume"), bare.region_stats, bare.hypsometry):
        with pytest.raises(ValueError, match="regions"):
            call()
    s = _stack(True, with_hyps=False)[0]
    with pytest.raises(ValueError, match="hyps"):
        s.hypsometry()


def test_save_load_round_trip(tmp_path):
    s = _stack(True)[0]
    s.save(tmp_path / "s.npz")
    b = posterior.PosteriorSummary.load(tmp_path / "s.npz")
    for name in ("region_func", "region_masks", "region_hyps", "region_hyps_range"):
        assert np.array_equal(getattr(b, name), getattr(s, name), equal_nan=True), name
    assert b.region_names == s.region_names and isinstance(b.region_names, tuple)
    assert (b.region_sea_level, b.region_density_ratio, b.region_resolution) == (s.region_sea_level, s.region_density_ratio, s.region_resolution)
    assert isinstance(b.region_resolution, float)
    for what in posterior.REGION_QUANTITIES:
        assert np.array_equal(b.region_values(what), s.region_values(what), equal_nan=True)
        for key, v in s.region_stats()[what].items():
            assert np.array_equal(b.region_stats()[what][key], v, equal_nan=True)
    assert all(np.array_equal(b.hypsometry()[k], v) for k, v in s.hypsometry().items())


def test_rank_merge_concatenates_in_rank_order():
    K, Tn, B = 2, 4, 6
    func = np.arange(5 * K * Tn * 8, dtype=np.float64).reshape(5, K, Tn, 8)
    hyps = np.arange(5 * K * (B + 2), dtype=np.int32).reshape(5, K, B + 2)
    parts = [(func[:3], hyps[:3]), (func[3:], hyps[3:])]                        # ragged shards of 3 and 2 chains
    f, h = posterior.merge_regions(parts)
    assert np.array_equal(f, func) and np.array_equal(h, hyps) and h.dtype == np.int64 and f.dtype == np.float64
    f, h = posterior.merge_regions(parts[::-1])                                 # the order of the ranks is the order of the chains
    assert np.array_equal(f, np.concatenate([func[3:], func[:3]])) and np.array_equal(h, np.concatenate([hyps[3:], hyps[:3]]))
    f, h = posterior.merge_regions([(func[:3], None), (func[3:], None)])
    assert np.array_equal(f, func) and h is None
    f, h = posterior.merge_regions([(func, hyps)])                              # one rank: its own arrays
    assert np.array_equal(f, func) and np.array_equal(h, hyps)
    with pytest.raises(ValueError, match="some ranks"):
        posterior.merge_regions([(func[:3], hyps[:3]), (func[3:], None)])
    with pytest.raises(ValueError, match="same K and T"):
        posterior.merge_regions([(func[:3], None), (func[3:, :, :2], None)])
    with pytest.raises(ValueError, match="beside their func"):
        posterior.merge_regions([(func[:3], hyps[:2]), (func[3:], hyps[3:])])
    with pytest.raises(ValueError, match="no rank"):
        posterior.merge_regions([])
