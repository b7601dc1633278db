"""GPU: the kriging solve of every kernel that has one -- gsm_krige_grid, gsm_krige_cv, gsm_sgs_blocks, gsm_sgs_grid and their
_local twins, all through krige_solve (csrc/sgs_search.h) -- against the extended-precision truth of tests/krige_exact_common.py
at its per-cell bars (a small multiple of 2^-53 cond ||w*||_1 max|v|; tests/test_krige_exact_host.py holds a NumPy restatement
of the device's elimination order to the same bars).  Neighbours come from the CPU oracle's search, never from the device; the
device's neighbour counts (and the block kernel's neighbour trace) are asserted equal before any number is compared.  Every
test prints its largest error / bar ratio per entry point and model."""
import warnings

import numpy as np
import pytest

import krige_exact_common as kx
import nonstationary_common as nc
import sgs_common as sc
import sgs_oracle as so

pytestmark = pytest.mark.gpu


@pytest.fixture
def refusals(monkeypatch):
    """Lets a call that flags 'singular kriging system' return what it computed (NaN at the refused cells, the others complete)
    and lists the refusals; every other device error still raises."""
    from mcmc_gpu_amd import _lib, engine
    seen = []
    check = engine.GsmEngine._check

    def tolerant(self, rc):
        try:
            check(self, rc)
        except _lib.GsmError as e:
            if "singular kriging system" not in str(e):
                raise
            seen.append(str(e))
    monkeypatch.setattr(engine.GsmEngine, "_check", tolerant)
    return seen


@pytest.fixture
def handed_tables(monkeypatch):
    """Records every lag table interpolate hands to the device: [(table, mi, mj)]."""
    from mcmc_gpu_amd import interpolate
    seen = []
    make = interpolate.lag_cov_table

    def spy(vario, hw, dx, dy, mi=None, mj=None):
        t = make(vario, hw, dx, dy, mi, mj)
        seen.append((t, (t.shape[0] - 1) // 2, (t.shape[1] - 1) // 2))
        return t
    monkeypatch.setattr(interpolate, "lag_cov_table", spy)
    return seen


def _same_entries(cov, handed):
    """The table the device got holds the truth's entries at every lag it spans."""
    t, mi, mj = handed
    assert mi <= cov.mi and mj <= cov.mj
    assert np.array_equal(t, cov.table[cov.mi - mi:cov.mi + mi + 1, cov.mj - mj:cov.mj + mj + 1])


def _report(what, r_est, r_var):
    print(f"\n{what}: largest error / bar: est {r_est:.3f} var {r_var:.3f}")
    assert r_est < 1.0 and r_var < 1.0, (what, r_est, r_var)


@pytest.mark.parametrize("kt", kx.KTYPES)
@pytest.mark.parametrize("mid", sorted(kx.MODELS))
def test_krige_grid(mid, kt, refusals, handed_tables):
    from mcmc_gpu_amd import interpolate
    worst = (0.0, 0.0)
    for lid in kx.LAYOUTS:
        recs = kx.truth(lid, mid, kt)
        plan = kx.plan_of(lid, kx.MODELS[mid], kt)
        est, var, n = interpolate._krige_run(plan, kx.layout(lid)["cells"])
        _same_entries(kx.table_cov(plan, plan.vario), handed_tables[-1])
        worst = np.maximum(worst, kx.ratios(recs, est, var, n, f"gsm_krige_grid {mid} {kt} layout {lid}"))
        assert refusals or not np.isnan(est).any()
    _report(f"gsm_krige_grid {mid} {kt}", *worst)


@pytest.mark.parametrize("kt", kx.KTYPES)
@pytest.mark.parametrize("maps", ["constant", "smooth"])
@pytest.mark.parametrize("vtype", kx.LOCAL_VTYPES)
def test_krige_grid_local(vtype, maps, kt, refusals):
    from mcmc_gpu_amd import interpolate
    worst = (0.0, 0.0)
    for lid in kx.LAYOUTS:
        recs = kx.truth_local(lid, vtype, maps, kt)
        plan = kx.plan_of(lid, kx.local_vario(lid, vtype, maps), kt)
        assert plan.local is not None
        est, var, n = interpolate._krige_run(plan, kx.layout(lid)["cells"])
        worst = np.maximum(worst, kx.ratios(recs, est, var, n, f"gsm_krige_grid_local {vtype} {maps} maps {kt} layout {lid}"))
    _report(f"gsm_krige_grid_local {vtype} {maps} maps {kt}", *worst)


@pytest.mark.parametrize("kt", kx.KTYPES)
def test_krige_cv_eight_models_in_one_call(kt, refusals, handed_tables):
    """Leave-one-out with the Gaussian series and three other models in ONE gsm_krige_cv call: one search per target, eight
    solves that rewrite the same LDS, conditioning from ~1e1 to ~1e12.  Each model's results against its own truth."""
    from mcmc_gpu_amd import interpolate
    targets, _ = kx.cv_targets()
    models = [kx.MODELS[m] for m in kx.CV_MODELS]
    assert len(models) == interpolate.CV_MAX_MODELS == 8
    plan = kx.plan_of(kx.CV_LAYOUT, models[0], kt)
    est, var, n = interpolate._cv_run(plan, models, targets, None, 0.0)
    assert len(handed_tables) == 8
    for m, (name, recs) in enumerate(zip(kx.CV_MODELS, kx.cv_truth(kt))):
        _same_entries(kx.table_cov(plan, models[m]), handed_tables[m])
        # the neighbour count is the call's, one for all models: a model's refusal does not clear it
        _report(f"gsm_krige_cv {name} {kt}", *kx.ratios(recs, est[m], var[m], n, f"gsm_krige_cv {name} {kt}"))


@pytest.mark.parametrize("kt", kx.KTYPES)
def test_krige_cv_local_three_models_in_one_call(kt, refusals):
    from mcmc_gpu_amd import interpolate
    targets, _ = kx.cv_targets()
    varios = kx.cv_local_varios()
    plan = kx.plan_of(kx.CV_LAYOUT, varios[0], kt)
    est, var, n = interpolate._cv_run(plan, varios, targets, None, 0.0)
    for m, ((vtype, maps), recs) in enumerate(zip(kx.CV_LOCAL, kx.cv_truth_local(kt))):
        what = f"gsm_krige_cv_local {vtype} {maps} maps {kt}"
        _report(what, *kx.ratios(recs, est[m], var[m], n, what))


# ---- sequential simulation: one step at a time ----------------------------------------------------------------------------------------
def _one_step(what, cov, kt, gmean, out, nbrs, tr, z):
    """Every simulated cell of a finished run as one kriging step: its neighbours (the oracle's) hold their final values in the
    returned grid `out` by the time the cell is visited -- inputs of the cell, not its output.  tr [cells, (n, est, var)] and
    out[cell] = est + sqrt(|var|) z against the truth of that one system.  nbrs: [(i, j, [(ni, nj), ...])] in path order."""
    recs = []
    for i, j, nb in nbrs:
        ni, nj = np.array([p[0] for p in nb]), np.array([p[1] for p in nb])
        recs.append(kx.solve_cell(cov, i, j, ni, nj, out[ni, nj], kt, gmean))
    assert all(r.kappa <= kx.KAPPA_REFUSE for r in recs), f"{what}: the case is meant to stay well conditioned"
    r_est, r_var = kx.ratios(recs, tr[:, 1], np.abs(tr[:, 2]), tr[:, 0].astype(int), what)
    r_val = 0.0
    for k, ((i, j, _), rec) in enumerate(zip(nbrs, recs)):
        sd = np.sqrt(abs(rec.var))
        want = rec.est + sd * kx.LD(z[k])
        bar = rec.b_est + abs(z[k]) * rec.b_var / (2.0 * float(sd)) + 4 * kx.U * abs(out[i, j])
        r_val = max(r_val, float(abs(kx.LD(out[i, j]) - want) / bar))
    print(f"\n{what}: {len(recs)} cells, n {min(r.n for r in recs)} .. {max(r.n for r in recs)}, cond up to {max(r.kappa for r in recs):.1e}: "
          f"largest error / bar: est {r_est:.3f} var {r_var:.3f} value {r_val:.3f}")
    assert r_est < 1.0 and r_var < 1.0 and r_val < 1.0, (what, r_est, r_var, r_val)


BLOCK_MODELS = ("exp9k", "matern", "sph9k", "exp_aniso")
BLOCK_WIN = (9, 23, 17, 29)            # 14 x 12 cells, row 16 of them conditioning data: 156 simulated cells, three chunks of 64


@pytest.mark.parametrize("kt", kx.KTYPES)
@pytest.mark.parametrize("whole_grid_table", [True, False])
def test_sgs_blocks(whole_grid_table, kt):
    """gsm_sgs_blocks on one chain whose window lists 168 cells: neighbours from the cell's own chunk of 64, from earlier chunks
    and from outside the block (sgs_sequence_kernel), at both ways krige_solve loads its rows (a table over every lag of the
    grid, a table of the search window's lags with a range test).  48 neighbours within 4 km on a grid full of values."""
    import torch
    from mcmc_gpu_amd import sgs
    from mcmc_gpu_amd.engine import GsmEngine, _ptr
    H, npts, rad, seed = 48, 48, 4000.0, 77
    prob = sc.driver_problem(H, dy=sc.TIE_FREE_DY)
    xx, yy = np.ascontiguousarray(prob["xx"], dtype=np.float64), np.ascontiguousarray(prob["yy"], dtype=np.float64)
    bed = (prob["bed"] - prob["bed"].mean()) / prob["bed"].std()
    is_data = prob["data_mask"]
    r0, r1, c0, c1 = BLOCK_WIN
    xs, ys, dx, dy = sgs._axes(xx, yy)
    hw = int(np.ceil(rad / abs(dx)))
    mi, mj = (H - 1, H - 1) if whole_grid_table else (2 * hw, 2 * hw)
    assert mi <= H - 1
    start = bed.copy()                                                     # what the oracle sees: the block emptied but for its data
    start[r0:r1, c0:c1] = np.where(is_data[r0:r1, c0:c1], bed[r0:r1, c0:c1], np.nan)
    sim_mask = np.zeros((H, H), bool)
    sim_mask[r0:r1, c0:c1] = True
    gmean = float(np.mean(start[~np.isnan(start)]))
    # the reference's draws (MCMC.py:128, :165): one shuffle of the window's cells, one normal per simulated cell
    rng = np.random.default_rng(seed)
    ii, jj = np.meshgrid(np.arange(H), np.arange(H), indexing="ij")
    inds = np.array([ii[sim_mask].flatten(), jj[sim_mask].flatten()]).T
    rng.shuffle(inds)
    simulated = ~is_data[inds[:, 0], inds[:, 1]]
    z = np.zeros(inds.shape[0])
    z[simulated] = rng.standard_normal(int(simulated.sum()))
    assert inds.shape[0] == 168 and simulated.sum() == 156
    eng = GsmEngine(H, H, 1)
    dev = eng.dev
    f64 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    try:
        d_gm = f64([gmean])
        eng._check(eng.lib.gsm_sgs_set_kriging(eng.h, 1 if kt == "sk" else 0, _ptr(d_gm)))
        for mid in BLOCK_MODELS:
            vario = kx.MODELS[mid]
            so.STABLE_TIES, so.NBR_LOG = True, []
            try:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    so.sgs(xx, yy, start, dict(vario), rad, npts, kt, sim_mask=sim_mask, rng=np.random.default_rng(seed))
                nbrs = [e for e in so.NBR_LOG if e[2]]                                       # an empty search widens and logs again
            finally:
                so.STABLE_TIES, so.NBR_LOG = False, None
            assert [(i, j) for i, j, _ in nbrs] == [tuple(c) for c in inds[simulated]]
            cov = kx.TableCov(vario, hw, dx, dy, H, H)
            table = sgs.lag_cov_table(vario, hw, dx, dy, mi, mj)
            _same_entries(cov, (table, mi, mj))
            grid = f64(bed[None])
            keep = (f64(np.where(is_data, bed, np.nan)), i32([BLOCK_WIN]), f64(xs), f64(ys), f64(table), i32([0, inds.shape[0]]), i32(inds), f64(z))
            tr = torch.zeros((inds.shape[0], 3), dtype=torch.float64, device=dev)
            nbr = torch.full((inds.shape[0], 48), -2, dtype=torch.int32, device=dev)
            eng._check(eng.lib.gsm_sgs_blocks(eng.h, _ptr(grid), _ptr(keep[0]), _ptr(keep[1]), _ptr(keep[2]), _ptr(keep[3]), _ptr(keep[4]), mi, mj,
                                              hw, rad, npts, float(vario["sill"]), _ptr(keep[5]), _ptr(keep[6]), _ptr(keep[7]), int(inds.shape[0]),
                                              _ptr(tr), _ptr(nbr), eng._stream()))
            out, t, nb = grid.cpu().numpy()[0], tr.cpu().numpy(), nbr.cpu().numpy()
            assert np.array_equal(t[:, 0] < 0, ~simulated)
            outside = ~sim_mask | is_data
            assert np.array_equal(out[outside], bed[outside])
            for k, (i, j, lst) in zip(np.flatnonzero(simulated), nbrs):                     # the neighbour trace, entry by entry
                want = np.full(48, -1, dtype=np.int32)
                want[:len(lst)] = [a * H + b for a, b in lst]
                assert np.array_equal(nb[k], want), (mid, k)
            origin = {tuple(c): k for k, c in enumerate(inds)}                               # where each neighbour's value came from
            kinds = set()
            for i, j, lst in nbrs:
                for p in lst:
                    kinds.add("outside" if (p not in origin or is_data[p]) else "same chunk" if origin[p] // 64 == origin[(i, j)] // 64 else "earlier chunk")
            assert kinds == {"outside", "same chunk", "earlier chunk"}
            _one_step(f"gsm_sgs_blocks {mid} {kt} table extents ({mi}, {mj})", cov, kt, gmean, out, nbrs, t[simulated], z[simulated])
    finally:
        eng.close()


def _grid_case():
    """24 x 24 tie-free cells, conditioning lines every 6 rows and 8 columns, 16 neighbours within 3 km (interp_sgs_common.regimes'
    layout): the smallest grid on which a path fills more than six chunks of 64 cells."""
    import interp_sgs_common as ic
    H = W = 24
    xx, yy = np.meshgrid(np.arange(W) * 500.0, np.arange(H) * sc.TIE_FREE_DY)
    return xx, yy, np.where(ic._lines(H, W, 6, 8), ic.field(H, W, 31), np.nan), dict(radius=3000.0, num_points=16)


@pytest.mark.parametrize("kt", kx.KTYPES)
@pytest.mark.parametrize("mid", ["exp9k", "matern", "gau1500", "local Exponential", "local Gaussian", "local Spherical"])
def test_sgs_grid(mid, kt):
    """gsm_sgs_grid / gsm_sgs_grid_local with unbounded draws, two realisations in one call: every path cell as one step."""
    from mcmc_gpu_amd import interpolate
    xx, yy, grid, kw = _grid_case()
    H, W = grid.shape
    local = mid.startswith("local ")
    vario = nc.vario_of(H, W, mid.split()[1], 0.25 if mid.endswith("Gaussian") else 1.0) if local else kx.MODELS[mid]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plan = interpolate._Plan(xx, yy, grid, vario, kw["radius"], kw["num_points"], kt, None, None, None, None)
    seeds = [5, 6]
    ns, (paths, tr) = interpolate._run(plan, [np.random.default_rng(s) for s in seeds], trace=True)
    if local:
        cov = kx.LocalCov(plan.local, vario["vtype"], plan.xs, plan.ys)
    else:
        cov = kx.table_cov(plan, plan.vario)
    off = 0
    for r, s in enumerate(seeds):
        path, z = plan.draws(np.random.default_rng(s))
        assert np.array_equal(path, paths[r])
        so.NBR_LOG = []
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                if local:
                    nc.sgs_local(xx, yy, plan.grid_ns, vario, kw["radius"], kw["num_points"], kt, rng=np.random.default_rng(s), stable_ties=True)
                else:
                    so.STABLE_TIES = True
                    so.sgs(xx, yy, plan.grid_ns, dict(vario), kw["radius"], kw["num_points"], kt, rng=np.random.default_rng(s))
            nbrs = [e for e in so.NBR_LOG if e[2]]
        finally:
            so.STABLE_TIES, so.NBR_LOG = False, None
        assert np.array_equal([i * W + j for i, j, _ in nbrs], path)
        entry = "gsm_sgs_grid_local" if local else "gsm_sgs_grid"
        _one_step(f"{entry} {mid} {kt} seed {s}", cov, kt, plan.global_mean, ns[r], nbrs, tr[off:off + path.size], z)
        off += path.size
