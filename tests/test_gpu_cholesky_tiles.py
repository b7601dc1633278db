"""-m gpu: the precomputed-factor ("L z") proposal generator record by record at its tile edges, the chain path with groups of
more than one record tile, and gsm_cholesky_upper / gsm_cov_assemble at their block-count and leading-dimension edges.

Part 1 runs the launches of cholesky_cases.LAUNCHES, in order, on ONE engine whose block table is cholesky_cases.TILE_TABLE and
compares every record of every launch with cholesky_oracle.proposal (cz_scalars / cz_bucket / cz_zgen / cz_gemm_dma kernels).
The measured condition numbers and error maxima are in DESIGN.md, section 4.2b."""
import numpy as np
import pytest
import torch

import cholesky_cases as cc
import cholesky_oracle as co
import mcmc_oracle as orc
from gpu_common import make_engine
from mcmc_gpu_amd import cholesky as chol
from mcmc_gpu_amd._lib import GsmError

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------------
# 1. every record of a launch
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tile_run():
    """The device side of part 1, run once: the launch sequence on one engine, everything copied to the host."""
    rfp = cc.rf_params()
    eng, prob, cfg, _, _, _ = make_engine(64, len(cc.SEEDS), rf_params=rfp)
    rfp.resolution = prob["resolution"]
    rfp.generator = "cholesky"
    pairs, masks = cc.tile_pairs(), cc.tile_masks()
    eng.set_blocks(pairs, masks)
    run = dict(rfp=rfp, pairs=pairs, masks=masks, resolution=prob["resolution"], W=eng.W,
               centres=np.flatnonzero(cfg.region_mask.ravel() == 1), factors={}, sigmas={}, out={}, oracle={}, cache={})
    for launch in cc.LAUNCHES:
        ncls = launch["n_classes"]
        if getattr(eng, "n_classes", None) != ncls:
            factors = chol.build_factors(eng, rfp, n_classes=ncls, jitter=cc.JITTER)
            run["factors"][ncls] = [f.cpu().numpy() for f in factors]
            run["sigmas"][ncls] = [chol.cov_assemble(eng, bh, bw, rfp.resolution, v).cpu().numpy()
                                   for bh, bw in cc.TILE_TABLE for v in chol.class_varios(rfp, ncls)]
        out = eng.propose_philox(launch["n_steps"], launch["step0"], cc.SEEDS, rfp)
        run["out"][launch["name"]] = {k: v.cpu().numpy() for k, v in out.items()}
    eng.close()
    return run


def _oracle(run, launch):
    """The oracle side of a launch, computed once; the oracle's factors are shared by the launches of one class count."""
    if launch["name"] not in run["oracle"]:
        ncls = launch["n_classes"]
        run["oracle"][launch["name"]] = cc.OracleLaunch(launch, run["rfp"], run["pairs"], run["masks"], run["centres"], run["W"],
                                                        run["resolution"], chol.class_varios(run["rfp"], ncls),
                                                        run["cache"].setdefault(ncls, {}))
    return run["oracle"][launch["name"]]


def _oracle_allowance(run, ncls):
    """First-order sensitivity of a Cholesky factor to the rounding of the assembly, cond * eps, times 10 for the product with z;
    cond of the table's largest block in the class of the longest range (the worst conditioned).  In units of the scale."""
    conds = [np.linalg.cond(orc.cov_matrix(co.block_coords(*cc.TILE_TABLE[-1], run["resolution"]), v) + cc.JITTER * v["sill"] * np.eye(520))
             for v in chol.class_varios(run["rfp"], ncls)]
    return max(conds), 10.0 * max(conds) * cc.EPS


@pytest.mark.parametrize("launch", cc.LAUNCHES, ids=[l["name"] for l in cc.LAUNCHES])
def test_every_record_of_a_launch_matches_the_oracle(tile_run, launch):
    ora = _oracle(tile_run, launch)
    counts = ora.counts
    print(f"\n{launch['name']}: records per group {counts.tolist()}")
    # the geometry this launch is here for
    if launch["name"] == "big":
        assert (counts > 192).any() and ((counts >= 129) & (counts <= 192)).any()
    elif launch["name"] == "tiny":
        assert (counts == 0).any() and (counts == 1).any()
    elif launch["name"] == "at64":
        assert (counts == 64).any() and (counts < 64).any() and (counts > 64).any()
    else:
        assert len(counts) == 3 * len(cc.TILE_TABLE) and counts.min() >= 1
    cond, allow = _oracle_allowance(tile_run, launch["n_classes"])
    assert allow <= 1e-8                                   # no looser than the sampled test's 1e-8 of the scale
    out = tile_run["out"][launch["name"]]
    dev_counts = np.bincount((out["size_idx"] * launch["n_classes"] + out["rf_scalars"][..., 2].astype(np.int64)).ravel(),
                             minlength=len(counts))
    print(f"{launch['name']}: records per group on the device {dev_counts.tolist()}")
    worst_exact, worst_oracle = cc.compare_launch(out, ora, tile_run["factors"][launch["n_classes"]], tile_run["masks"], allow)
    print(f"{launch['name']}: cond {cond:.4e}, largest error / scale: {worst_exact:.3e} against U_dev^T z (bound 1e-12), "
          f"{worst_oracle:.3e} against the oracle's factor (bound {allow:.3e})")


@pytest.mark.parametrize("ncls", [1, 3])
def test_factors_of_the_tile_table(tile_run, ncls):
    """U^T U == Sigma + jitter I to 1e-12 (sill 1) for every (size, class) of the table, U upper triangular with zero padding;
    the device covariance equals the oracle's to the tolerance of the F6 fixture test."""
    varios = chol.class_varios(tile_run["rfp"], ncls)
    worst = 0.0
    for g, (U, sigma) in enumerate(zip(tile_run["factors"][ncls], tile_run["sigmas"][ncls])):
        bh, bw = cc.TILE_TABLE[g // ncls]
        N, Np = bh * bw, (bh * bw + 63) // 64 * 64
        v = varios[g % ncls]
        assert U.shape == (Np, Np) and sigma.shape == (N, N)
        assert not U[N:, :].any() and not U[:, N:].any() and not np.tril(U, -1).any()
        np.testing.assert_allclose(sigma, orc.cov_matrix(co.block_coords(bh, bw, tile_run["resolution"]), v), rtol=0, atol=1e-12)
        err = np.abs(U[:N, :N].T @ U[:N, :N] - (sigma + cc.JITTER * v["sill"] * np.eye(N))).max()
        assert err <= 1e-12, f"group {g} (N = {N}): |U^T U - (Sigma + jitter I)| = {err:.3e}"
        worst = max(worst, err)
    print(f"\n{ncls} classes: largest |U^T U - (Sigma + jitter I)| = {worst:.3e}")


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the chain path with groups of more than one record tile
# ---------------------------------------------------------------------------------------------------------------------------
def test_chain_path_with_multi_tile_groups():
    """run_philox in two launches of 2048 records (25 groups of ~82: two record tiles, the two scratch slots alternating) ==
    one propose_philox of 4096 records (~164 per group: three tiles) + run_replay, bit for bit."""
    n_chains, n_steps, step0 = 32, 128, 4000
    rfp = orc.standard_rf_params(model="Exponential")
    eng, prob, cfg, pairs, masks, _ = make_engine(64, n_chains, rf_params=rfp)
    rfp.resolution = prob["resolution"]
    rfp.generator = "cholesky"
    chol.build_factors(eng, rfp, n_classes=1)
    beds0 = np.stack([orc.chain_initial_bed(prob, c) for c in range(n_chains)])
    seeds = [4100 + 3 * c for c in range(n_chains)]
    eng.set_state(beds0)
    loss, acc, blk = eng.run_philox(n_steps, step0, seeds, rfp, batch=64)
    assert eng.last_run_fused() == 0
    beds = eng.beds.cpu().numpy().copy()
    eng.set_state(beds0)
    p = eng.propose_philox(n_steps, step0, seeds, rfp)
    si, ce = p["size_idx"].cpu().numpy(), p["centre"].cpu().numpy()
    for half in (si[:, :64], si[:, 64:]):
        assert np.bincount(half.ravel(), minlength=25).max() > 64          # a batch has groups of more than one record tile
    assert np.bincount(si.ravel(), minlength=25).max() > 128
    loss_r, acc_r = eng.run_replay(si, ce, p["u"].cpu().numpy(), p["fields"])
    assert np.array_equal(acc, acc_r) and np.array_equal(loss, loss_r)
    assert np.array_equal(beds, eng.beds.cpu().numpy())
    assert np.array_equal(blk[..., :2], ce) and np.array_equal(blk[..., 2], pairs[1][si]) and np.array_equal(blk[..., 3], pairs[0][si])
    assert 0.2 < acc.mean() <= 1.0
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. gsm_cholesky_upper at its block-count edges, gsm_cov_assemble with a padded leading dimension
# ---------------------------------------------------------------------------------------------------------------------------
SENTINEL = -7.25e77


@pytest.fixture(scope="module")
def eng1():
    eng, *_ = make_engine(64, 1)
    yield eng
    eng.close()


def _factor(eng, S, ld, jitter=0.0):
    """gsm_cholesky_upper on a copy of S in an [n][ld] device array whose columns past n hold SENTINEL; the whole array back."""
    n = S.shape[0]
    A = torch.full((n, ld), SENTINEL, dtype=torch.float64, device=eng.dev)
    A[:, :n] = torch.as_tensor(S, device=eng.dev)
    eng.call(eng.lib.gsm_cholesky_upper, A, n, ld, float(jitter))
    return A.cpu().numpy()


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("n", [64, 128, 192])          # diagonal kernel only; one panel and one update tile; two panels, 3 + 1 update tiles
def test_cholesky_upper_sizes_and_leading_dimension(eng1, n, pad):
    S = cc.spd(n, 100 + n)
    A = _factor(eng1, S, n + pad)
    np.testing.assert_allclose(A[:, :n], np.linalg.cholesky(S).T, rtol=0, atol=1e-12)
    assert not np.tril(A[:, :n], -1).any()
    assert np.array_equal(A[:, n:], np.full((n, pad), SENTINEL))       # the padding columns come back bit-unchanged


def test_cholesky_upper_jitter(eng1):
    S = cc.spd(192, 7)
    A = _factor(eng1, S, 192, jitter=0.5)
    np.testing.assert_allclose(A, np.linalg.cholesky(S + 0.5 * np.eye(192)).T, rtol=0, atol=1e-12)


@pytest.mark.parametrize("case", ["pivot64", "pivot65", "pivot131", "nan71"])
def test_cholesky_upper_reports_the_first_failing_pivot(eng1, case):
    """The pivot an unblocked NumPy loop fails at first: the last of the first diagonal block, the first of the second (after
    one panel and update), one inside the third, and a NaN on the diagonal.  After the failure the host still launches the
    remaining panels on the abandoned matrix; the first index must survive them.  The next good call on the handle succeeds."""
    S = cc.spd(192, 11)
    if case == "nan71":
        bad, pivot = S.copy(), 71
        bad[70, 70] = np.nan
    else:
        pivot = int(case[5:])
        bad = cc.fail_at(S, pivot)
    assert cc.unblocked_cholesky_first_failure(S) == 0
    assert cc.unblocked_cholesky_first_failure(bad) == pivot
    with pytest.raises(GsmError, match=rf"not positive definite at pivot {pivot} \(") as ei:
        _factor(eng1, bad, 192)
    assert ei.value.code == -1
    good = cc.spd(128, 13)
    np.testing.assert_allclose(_factor(eng1, good, 128), np.linalg.cholesky(good).T, rtol=0, atol=1e-12)


@pytest.mark.parametrize("vt", ["Exponential", "Matern"])          # closed form; lag table
def test_cov_assemble_with_a_padded_leading_dimension(eng1, vt):
    v = chol.make_vario(vt, 4000.0, 2500.0, azimuth=30.0, s=0.9125 if vt == "Matern" else None)
    bh, bw = 10, 14
    N = bh * bw
    tight = chol.cov_assemble(eng1, bh, bw, 500.0, v).cpu().numpy()
    padded = chol.cov_assemble(eng1, bh, bw, 500.0, v, ld=N + 8).cpu().numpy()
    assert padded.shape == (N, N + 8)
    assert np.array_equal(padded[:, :N], tight) and not padded[:, N:].any()
    np.testing.assert_allclose(tight, orc.cov_matrix(co.block_coords(bh, bw, 500.0), v), rtol=0, atol=1e-12)
