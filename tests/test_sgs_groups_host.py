"""CPU: the host side of chain groups -- every refusal of run_many_sgs(groups=) / smallScaleChain_mp(groups=) is raised before a handle
exists or a generator is touched (this file runs without a GPU: reaching the device would raise RuntimeError instead), and
sgs.slice_groups hands every rank its chains' groups, renumbered."""
import numpy as np
import pytest

import sgs_groups_common as gc
from mcmc_gpu_amd import driver, sgs


class _Wrapped:
    def __init__(self, inner):
        self.inner = inner

    def transform(self, x):
        return self.inner.transform(x)

    def inverse_transform(self, x):
        return self.inner.inverse_transform(x)


def _refused(exc, match, ch, groups, n=6):
    prob = gc.sc.problem(gc.H)
    beds = gc.beds_of(prob, n)
    rngs = [np.random.default_rng(i) for i in range(n)]
    states = [r.bit_generator.state for r in rngs]
    with pytest.raises(exc, match=match):
        sgs.run_many_sgs(ch, beds, rngs, 5, groups=groups)
    with pytest.raises(exc, match=match):
        sgs.run_many_sgs(ch, beds, rngs, 5, pcg64=True, groups=groups)
    assert [r.bit_generator.state for r in rngs] == states


def test_refusals(tmp_path):
    from sklearn.preprocessing import QuantileTransformer
    prob, trends, nst = gc.tables("qt")
    qt = gc.template(prob, trends[0], nst[0])
    only_trend = gc.template(prob, trends[0], None)
    only_nst = gc.template(prob, None, nst[0])
    plain = gc.template(prob, None, None)
    ok = gc.groups_dict(gc.OF, trends, nst)
    assert sgs.check_groups(qt, None, 6) is None
    of, t, q = sgs.check_groups(qt, ok, 6)
    assert of.dtype == np.int32 and np.array_equal(of, gc.OF) and t.shape == (gc.G, gc.H, gc.H) and len(q) == gc.G
    _refused(ValueError, "'of'", qt, dict(trend=trends, nst_trans=nst))
    _refused(ValueError, "'of'", qt, [0, 1])
    _refused(ValueError, "unknown keys", qt, dict(ok, vario=1))
    _refused(ValueError, "one integer per chain", qt, dict(ok, of=gc.OF[:5]))
    _refused(ValueError, "one integer per chain", qt, dict(ok, of=gc.OF.astype(float)))
    _refused(ValueError, "one integer per chain", qt, dict(ok, of=gc.OF[None]))
    _refused(ValueError, r"must lie in \[0, 4\)", qt, dict(ok, of=np.array([0, 1, 2, 3, 4, 0])))
    _refused(ValueError, r"must lie in \[0, 4\)", qt, dict(ok, of=np.array([0, -1, 2, 3, 1, 0])))
    _refused(ValueError, "shape", qt, dict(ok, trend=trends[:, :-1]))
    _refused(ValueError, "shape", qt, dict(ok, trend=trends[0]))
    bad = trends.copy(); bad[2, 3, 3] = np.nan
    _refused(ValueError, "finite", qt, dict(ok, trend=bad))
    bad[2, 3, 3] = np.inf
    _refused(ValueError, "finite", qt, dict(ok, trend=bad))
    _refused(ValueError, "one transformer per group", qt, dict(ok, nst_trans=nst[:3]))
    other = QuantileTransformer(n_quantiles=150, output_distribution="normal", subsample=None, random_state=7).fit((prob["bed"] - trends[1]).reshape(-1, 1))
    _refused(ValueError, "n_quantiles_ differ", qt, dict(ok, nst_trans=[nst[0], other, nst[2], nst[3]]))
    _refused(NotImplementedError, "host", qt, dict(ok, nst_trans=[nst[0], _Wrapped(nst[1]), nst[2], nst[3]]))
    uniform = QuantileTransformer(n_quantiles=200, subsample=None, random_state=7).fit((prob["bed"] - trends[1]).reshape(-1, 1))
    _refused(NotImplementedError, "host", qt, dict(ok, nst_trans=[nst[0], uniform, nst[2], nst[3]]))
    # a key the template's flags do not call for, and a key they call for that is missing
    _refused(ValueError, "nst_trans'\\] is given", only_trend, ok)
    _refused(ValueError, "trend'\\] is given", only_nst, ok)
    _refused(ValueError, "trend'\\] is needed", qt, dict(of=gc.OF, nst_trans=nst))
    _refused(ValueError, "nst_trans'\\] is needed", qt, dict(of=gc.OF, trend=trends))
    _refused(ValueError, "given", plain, ok)
    _refused(ValueError, "neither", plain, dict(of=gc.OF))
    # the driver refuses the same before it writes or starts anything
    beds = gc.beds_of(prob, 6)
    call = lambda n_iters, g: driver.smallScaleChain_mp(6, 1, qt, beds, [1, 2, 3, 4, 5, 6], 5, n_iters, output_path=str(tmp_path), n_gpus=1, groups=g)
    with pytest.raises(ValueError, match="same n_iter"):
        call([5, 5, 5, 5, 5, 6], ok)
    with pytest.raises(ValueError, match="must lie in"):
        call([5] * 6, dict(ok, of=gc.OF + 2))
    assert not (tmp_path / "LargeScaleChain").exists()


def test_slices_cover_all_chains_and_renumber_densely():
    from mcmc_gpu_amd import parallel
    prob, trends, nst = gc.tables("qt", 7)
    of = np.array([5, 2, 2, 6, 0, 5, 5, 2, 6, 6, 0])                         # groups 1, 3, 4 unused
    groups = gc.groups_dict(of, trends, nst)
    for world in (1, 2, 3, 4, 11):
        seen = []
        for rank in range(world):
            lo, hi = parallel.shard_bounds(of.size, world, rank)
            part = sgs.slice_groups(groups, lo, hi)
            k = len(part["nst_trans"])
            assert part["trend"].shape == (k, gc.H, gc.H) and part["of"].dtype == np.int32 and part["of"].shape == (hi - lo,)
            assert sorted(set(part["of"].tolist())) == list(range(k))         # dense: every local group is used, none is missing
            for c in range(lo, hi):                                          # the chain keeps its own trend and transformer
                assert np.array_equal(part["trend"][part["of"][c - lo]], trends[of[c]])
                assert part["nst_trans"][part["of"][c - lo]] is nst[of[c]]
            sgs.check_groups(gc.template(prob, trends[0], nst[0]), part, hi - lo)
            seen += list(range(lo, hi))
        assert seen == list(range(of.size))
    assert sgs.slice_groups(None, 0, 3) is None
    only_t = sgs.slice_groups(dict(of=of, trend=trends), 3, 6)
    assert set(only_t) == {"of", "trend"} and np.array_equal(only_t["of"], [2, 0, 1]) and np.array_equal(only_t["trend"], trends[[0, 5, 6]])


def test_handoff_on_the_host():
    prob, trends, nst = gc.tables("qt")
    tmpl = gc.template(prob, trends[0], nst[0])
    lsc = np.stack([prob["bed"] + 10.0 * g for g in range(2)])
    lsc[0, 2, 2] = prob["surf"][2, 2]                                        # thickness exactly 0: clamped (<=)
    beds, groups = sgs.handoff(tmpl, lsc, [1, 0, 1], sigma=2, n_quantiles=100, random_state=1, device=False)
    assert beds[1][2, 2] == prob["surf"][2, 2] - 1 and np.array_equal(beds[0], lsc[1]) and np.array_equal(beds[0], beds[2])
    from scipy.ndimage import gaussian_filter
    assert np.array_equal(groups["trend"][1], gaussian_filter(lsc[1], sigma=2))
    assert sgs.check_groups(tmpl, groups, 3)[0].tolist() == [1, 0, 1]
    with pytest.raises(ValueError, match="lsc_beds"):
        sgs.handoff(tmpl, lsc[0], [0])
    with pytest.raises(ValueError, match="`of`"):
        sgs.handoff(tmpl, lsc, [0, 2])
