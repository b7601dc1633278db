"""Shared by tests/test_gpu_sgs_groups.py and tests/test_sgs_groups_host.py: the small-scale chain with chain groups
(run_many_sgs(groups=), gsm_sgs_set_groups) on the 32 x 32 problem of tests/sgs_common.problem with blocks 3-8.

G = 4 groups whose trends and transformers really differ: trend_g = the problem's trend + g * (a smooth field of some metres), the
transformer of group g fitted on the bed minus that trend (or, without a trend, on the bed stretched by a factor of g's own).
OF = [2, 0, 1, 1, 2, 1]: interleaved, unequal group sizes, group 3 unused."""
import numpy as np

import sgs_common as sc

H = 32
G = 4
OF = np.array([2, 0, 1, 1, 2, 1])
CFGS = ("trend", "qt", "nst")          # trend only (windowed finish); trend + transformer; transformer only (whole-map paths)
SOURCES = ("replay", "pcg64", "philox")


def smooth(prob):
    return 6.0 * np.sin(2 * np.pi * prob["xx"] / (H * 500.0)) * np.cos(np.pi * prob["yy"] / (H * 500.0)) + 2.0


def tables(cfg, n_groups=G):
    """(problem, trends [n_groups, H, H] or None, transformers or None) of a configuration"""
    prob = sc.problem(H)
    trends = nst = None
    if cfg in ("trend", "qt"):
        trends = np.stack([prob["trend"] + g * smooth(prob) for g in range(n_groups)])
    if cfg in ("qt", "nst"):
        from sklearn.preprocessing import QuantileTransformer
        nst = []
        for g in range(n_groups):
            data = prob["bed"] - trends[g] if trends is not None else prob["bed"] * (1.0 + 0.03 * g) - 5.0 * g
            nst.append(QuantileTransformer(n_quantiles=200, output_distribution="normal", subsample=None, random_state=7).fit(data.reshape(-1, 1)))
    return prob, trends, nst


def template(prob, trend, nst):
    """The product chain on `prob` with this trend and transformer (either may be None), light settings as synthetic.sgs_template"""
    from mcmc_gpu_amd import sgs
    ch = sgs.chain_sgs_gpu(prob["xx"], prob["yy"], prob["bed"], prob["surf"], prob["velx"], prob["vely"], prob["dhdt"], prob["smb"],
                           prob["cond_bed"], prob["data_mask"], np.ones((H, H), dtype=int), prob["resolution"])
    ch.set_update_region(True, prob["region_mask"])
    ch.set_loss_type(sigma_mc=60.0, massConvInRegion=True)
    ch.set_normal_transformation(nst, do_transform=nst is not None)
    ch.set_trend(trend, detrend_map=trend is not None)
    # one variogram for every group (the reference asks for one consistent V1_p): the sill does not follow the group's trend
    sill = 1.0 if nst is not None else float(np.var(prob["bed"] - prob["trend"]))
    ch.set_variogram("Exponential", 6000.0, sill, 0.0, isotropic=True)
    ch.set_sgs_param(16, 4000.0)
    ch.set_block_sizes(3, 8, 3, 8)
    return ch


def groups_dict(of, trends, nst):
    d = dict(of=np.asarray(of))
    if trends is not None:
        d["trend"] = trends
    if nst is not None:
        d["nst_trans"] = nst
    return d


def beds_of(prob, n):
    return [prob["bed"] + np.random.default_rng(40 + i).normal(0, 3, prob["bed"].shape) for i in range(n)]


def run(ch, beds, idx, source, n_iter, **kw):
    """run_many_sgs of the chains `idx` (their own generators / seeds by chain number); returns (results, generator states, extra)"""
    from mcmc_gpu_amd import sgs
    rngs = [np.random.default_rng(900 + int(i)) for i in idx]
    out = sgs.run_many_sgs(ch, [beds[int(i)] for i in idx], rngs, n_iter, pcg64=source == "pcg64",
                           philox_seeds=[300 + int(i) for i in idx] if source == "philox" else None, **kw)
    return out[0], [r.bit_generator.state for r in rngs], out[2] if len(out) == 3 else None


def grouped_and_separate(cfg, source, n_iter, of=OF, n_groups=G, **kw):
    """(grouped results, grouped states, per-chain results of the separate runs, their states): one run with groups against one run per
    group on a template that holds the group's trend and transformer"""
    prob, trends, nst = tables(cfg, n_groups)
    of = np.asarray(of)
    beds = beds_of(prob, of.size)
    tmpl = template(prob, None if trends is None else trends[0], None if nst is None else nst[0])
    res, states, _ = run(tmpl, beds, np.arange(of.size), source, n_iter, groups=groups_dict(of, trends, nst), **kw)
    sep, sep_states = [None] * of.size, [None] * of.size
    for g in np.unique(of):
        idx = np.flatnonzero(of == g)
        r, s, _ = run(template(prob, None if trends is None else trends[g], None if nst is None else nst[g]), beds, idx, source, n_iter, **kw)
        for k, c in enumerate(idx):
            sep[c], sep_states[c] = r[k], s[k]
    return res, states, sep, sep_states


def assert_same_chains(res, states, sep, sep_states, source):
    """beds, accept masks, counts, blocks and generator states bit for bit; losses bit for bit with device draws and to the 1e-12
    relative agreement run_many_sgs documents with host draws"""
    assert states == sep_states
    for c, (x, y) in enumerate(zip(res, sep)):
        assert len(x) == len(y)
        for k in (0, 4, 5, 6):
            assert np.array_equal(x[k], y[k], equal_nan=True), (c, k)
        if source == "replay":
            np.testing.assert_allclose(x[3], y[3], rtol=1e-12)
        else:
            assert np.array_equal(x[3], y[3]), c


def acceptance(res):
    return float(np.mean([r[4].mean() for r in res]))
