"""-m gpu: the end of a small-scale iteration (mcmc_gpu_amd/csrc/sgs_iter_kernel.hip) kernel by kernel through the C ABI, against the
long-double reference and the derived bounds of tests/sgs_iter_common.py (tests/test_sgs_iter_host.py shows that an fp64 restatement
meets them): gsm_sgs_loss, gsm_sgs_state_init, gsm_sgs_finish (single calls on every window kind, and a sequence of 200),
gsm_sgs_decide, gsm_sgs_commit, gsm_sgs_commit_map, the one-launch tail of gsm_sgs_iterate without a transformer (mode 2) and with
one (mode 1, with and without the transforms inside the tail launch), and what the six stand-alone entry points refuse.

Every tolerance is a derived bound of sgs_iter_common (LOSS_BOUND, ENERGY_BOUND, the compensated sum's 2 u sum e) or an exact
equality; every u of an acceptance test sits at p_ref (1 -/+ m), m = max(1e-9, 8 x the bound on lp - ln), so no row is undecidable.

Mode 1 bound.  The transforms agree with scikit-learn's to QT_INV_ATOL = 1e-9 m per inverse transform (tests/test_gpu_sgs.py); the
round trip inverse(transform(.)) is the identity up to that, so after k round trips a bed is within k x 1e-9 m =: d of the
reference's.  A bed error d on every cell moves a residual by at most dv = d AV, AV = (|velx_r| + |velx_l|) / den_x +
(|vely_d| + |vely_u|) / den_y, and the loss by sum over the cells that enter of (2 |v| dv + dv^2) / (2 sigma^2): that is added to
LOSS_BOUND of the reference's plane."""
import numpy as np
import pytest

import sgs_iter_common as ic

pytestmark = pytest.mark.gpu
LD = ic.LD
E_ARG, E_STATE, E_UNSUPPORTED, E_DEVICE_DATA = -1, -2, -4, -5
NAN = float("nan")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


class World:
    """One handle on an H x W grid with the static fields of sgs_iter_common.make_case."""

    def __init__(self, H, W, n, state_dtype="f64", static=True):
        import torch
        from mcmc_gpu_amd.engine import GsmEngine
        self.torch, self.H, self.W, self.n = torch, H, W, n
        self.case = ic.make_case(H, W, n)
        self.eng = GsmEngine(H, W, n, state_dtype=state_dtype)
        self.lib, self.dev = self.eng.lib, self.eng.dev
        if static:
            c = self.case
            self.eng.set_static(c["surf"], c["velx"], c["vely"], c["dhdt"], c["smb"], None, c["upd"], c["mc"], ic.RES, ic.SIGMA)

    def to(self, a, dtype):
        return self.torch.as_tensor(np.ascontiguousarray(a, dtype=dtype)).to(self.dev)

    def f64(self, a):
        return None if a is None else self.to(a, np.float64)

    def i32(self, a):
        return self.to(a, np.int32)

    def u8(self, a):
        return self.to(a, np.uint8)

    def call(self, name, *args):
        self.eng.call(getattr(self.lib, name), *args)

    def refused(self, name, *args):
        """(code, text) of a call: (0, '') when it was taken."""
        from mcmc_gpu_amd._lib import GsmError
        try:
            self.call(name, *args)
        except GsmError as e:
            return e.code, str(e)
        return 0, ""

    def state_init(self, beds, trend):
        """(energy [n, H, W], state [n, 4]) of gsm_sgs_state_init, as device tensors."""
        t = self.torch
        energy = t.full((self.n, self.H, self.W), NAN, dtype=t.float64, device=self.dev)
        state = t.full((self.n, 4), NAN, dtype=t.float64, device=self.dev)
        self.call("gsm_sgs_state_init", beds, trend, energy, state)
        return energy, state

    def close(self):
        self.eng.close()


def chains_of(H, W):
    return [n for n in ic.CHAINS if n != 70 or (H, W) in ic.SMALL_GRIDS]


def trend_case(case, use_trend):
    """(beds as the chain holds them, trend or None)."""
    return (ic.detrended(case), case["trend"]) if use_trend else (case["beds"], None)


def comp_bound_ok(state, energy_plane):
    """state[0] + state[1] against the long-double sum of the device's own energy plane: (difference, 2 u sum e)."""
    s = energy_plane.astype(LD).sum()
    return abs(LD(state[0]) + LD(state[1]) - s), LD(2.0) * LD(ic.U) * s


# ---- gsm_sgs_loss ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_trend", [False, True])
@pytest.mark.parametrize("H,W", ic.GPU_GRIDS)
def test_loss_and_guard_against_the_long_double_reference(H, W, use_trend):
    got = {}
    for n in chains_of(H, W):
        w = World(H, W, n)
        try:
            beds, trend = trend_case(w.case, use_trend)
            loss_ref, bound, bad_ref, _ = ic.score(w.case, beds, trend)
            d_loss = w.f64(np.full(n, NAN))
            d_bad = w.i32(np.full(n, -1))
            w.call("gsm_sgs_loss", w.f64(beds), w.f64(trend), d_loss, d_bad)
            loss, bad = d_loss.cpu().numpy(), d_bad.cpu().numpy()
        finally:
            w.close()
        ratio = np.abs(loss.astype(LD) - loss_ref) / bound
        print(f"{H}x{W} n={n} trend={use_trend}: worst loss ratio {float(ratio.max()):.3f}, bound {float((bound / loss_ref).max()):.2e} relative")
        assert (ratio <= 1).all(), ratio
        assert np.array_equal(bad, bad_ref)
        if n >= 3:
            assert bad[0] == 0 and bad[1] > 0                                   # the guard fires on some beds and not on others
        got[n] = loss
    for n, loss in got.items():                                                 # chain c's loss whatever shares the handle
        assert same_bits(loss[:1], got[1])
        if n == 70:
            assert same_bits(loss[:3], got[3])


# ---- gsm_sgs_state_init ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_trend", [False, True])
@pytest.mark.parametrize("H,W", ic.GPU_GRIDS)
def test_state_init(H, W, use_trend):
    n = 3
    w = World(H, W, n)
    try:
        case = w.case
        beds, trend = trend_case(case, use_trend)
        energy, state = w.state_init(w.f64(beds), w.f64(trend))
        energy, state = energy.cpu().numpy(), state.cpu().numpy()
    finally:
        w.close()
    v, A = ic.residual_ld(ic.with_trend(beds, trend), case["surf"], case["velx"], case["vely"], case["dhdt"], case["smb"], ic.RES)
    e_ref, enters = ic.energy_ld(v, case["mc"])
    eb = ic.energy_bound(v, A, enters)
    assert (energy[~enters] == 0).all()                                         # exactly 0 off the mask and where the residual is NaN
    assert (np.abs(energy.astype(LD) - e_ref) <= eb).all()
    _, _, bad_ref, _ = ic.score(case, beds, trend)
    for c in range(n):
        diff, bound = comp_bound_ok(state[c], energy[c])
        print(f"{H}x{W} chain {c}: compensated sum off by {float(diff / bound):.3f} of its bound")
        assert diff <= bound
        assert state[c, 2] == (state[c, 0] + state[c, 1]) / ic.TWO_SIGMA2
        assert state[c, 3] == bad_ref[c]


# ---- gsm_sgs_finish, single calls ------------------------------------------------------------------------------------------------
ROLES = ("uphill_below", "uphill_above", "downhill", "grounds", "ring_grounded", "ungrounds")
REC_STRIDE = 3


def _pick(mask, inside, rng):
    """A cell (r, c) of the boolean map `inside` where mask holds, or None."""
    cells = np.argwhere(inside & mask)
    return None if len(cells) == 0 else tuple(cells[rng.integers(len(cells))])


def finish_case(H, W, win, use_trend):
    """cur, next [6, H, W] of the six ROLES on one window, and the static case: next == cur outside the window."""
    case = ic.make_case(H, W, 1)
    base, trend = trend_case(case, use_trend)
    base = base[0]
    lift = (lambda g: case["surf"][g] + 1.0 - (trend[g] if use_trend else 0.0))   # a bed a metre above the surface
    r0, r1, c0, c1 = win
    inwin = np.zeros((H, W), bool)
    inwin[r0:r1, c0:c1] = True
    h = ic.halo(win, H, W)
    ring = np.zeros((H, W), bool)
    ring[h[0]:h[1], h[2]:h[3]] = True
    ring &= ~inwin
    guarded = (case["upd"] == 1) & ~np.isnan(base)
    rng = np.random.default_rng([H, W, r0, r1, c0, c1])
    cells = max(1, (r1 - r0) * (c1 - c0))
    cur, nxt = np.tile(base, (6, 1, 1)), np.tile(base, (6, 1, 1))
    for c, role in enumerate(ROLES):
        nxt[c][inwin] += rng.standard_normal(int(inwin.sum())) / np.sqrt(cells)
        if role == "grounds" and (g := _pick(guarded, inwin, rng)) is not None:
            nxt[c][g] = lift(g)
        if role == "ring_grounded" and (g := _pick(guarded, ring, rng)) is not None:
            cur[c][g] = nxt[c][g] = lift(g)
        if role == "ungrounds" and (g := _pick(guarded, inwin, rng)) is not None:
            cur[c][g] = lift(g)
    # orientation by the reference's losses: the first two chains go uphill, the third downhill
    lc, _, _, _ = ic.score(case, cur, trend)
    ln, _, _, _ = ic.score(case, nxt, trend)
    for c, want_up in ((0, True), (1, True), (2, False)):
        if (ln[c] > lc[c]) != want_up:
            cur[c], nxt[c] = nxt[c].copy(), cur[c].copy()
    return case, cur, nxt, trend


def finish_expect(case, cur, nxt, trend, roles=ROLES):
    """Per chain: lp, ln (inf where the proposal is grounded), their bounds, bad counts, u and the reference's decision."""
    lp, bp, bad_c, _ = ic.score(case, cur, trend)
    ln, bn, bad_n, _ = ic.score(case, nxt, trend)
    out = []
    for c, role in enumerate(roles):
        ln_c = float("inf") if bad_n[c] > 0 else ln[c]
        if bad_n[c] > 0:
            u = 0.0 if role == "ring_grounded" else 0.5
        else:
            u = ic.u_at_margin(lp[c], ln_c, bp[c] + bn[c], below=role != "uphill_above")
        out.append(dict(lp=lp[c], ln=ln_c, bp=bp[c], bn=bn[c], bad_c=int(bad_c[c]), bad_n=int(bad_n[c]), u=u,
                        acc=ic.decide_ref(lp[c], ln_c, u)))
    return out


def run_finish(w, cur, nxt, trend, wins, u, energy, state, resampled):
    t = w.torch
    n = w.n
    accept = t.full((n,), 9, dtype=t.uint8, device=w.dev)
    loss_rec = t.full((n * REC_STRIDE,), -7.5, dtype=t.float64, device=w.dev)
    acc_rec = t.full((n * REC_STRIDE,), 9, dtype=t.uint8, device=w.dev)
    w.call("gsm_sgs_finish", cur, nxt, trend, energy, state, w.i32(wins), w.f64(u), resampled, accept, loss_rec, acc_rec, REC_STRIDE)
    return accept.cpu().numpy(), loss_rec.cpu().numpy().reshape(n, REC_STRIDE), acc_rec.cpu().numpy().reshape(n, REC_STRIDE)


@pytest.fixture(scope="module")
def finish_worlds():
    made = {}

    def get(H, W):
        if (H, W) not in made:
            made[(H, W)] = World(H, W, len(ROLES))
        return made[(H, W)]
    yield get
    for w in made.values():
        w.close()


IN_LIMIT = [k for k, v in ic.finish_windows().items() if not v[2]]


@pytest.mark.parametrize("use_trend", [False, True])
@pytest.mark.parametrize("name", IN_LIMIT)
def test_finish_single_call(finish_worlds, name, use_trend):
    (H, W), win, _ = ic.finish_windows()[name]
    w = finish_worlds(H, W)
    n = w.n
    case, cur, nxt, trend = finish_case(H, W, win, use_trend)
    exp = finish_expect(case, cur, nxt, trend)
    if (win[1] - win[0]) * (win[3] - win[2]) > 0:
        assert {e["acc"] for e in exp} == {True, False}
        assert exp[3]["bad_n"] > 0 and exp[0]["bad_n"] == 0                         # a guarded and an unguarded proposal
    d_cur, d_nxt, d_trend = w.f64(cur), w.f64(nxt), w.f64(trend)
    energy, state = w.state_init(d_cur, d_trend)
    energy0, state0 = energy.cpu().numpy(), state.cpu().numpy()
    res0 = np.arange(n * H * W, dtype=np.int32).reshape(n, H, W) % 11
    resampled = w.i32(res0)
    accept, loss_rec, acc_rec = run_finish(w, d_cur, d_nxt, d_trend, np.tile(win, (n, 1)), [e["u"] for e in exp], energy, state, resampled)
    rc, msg = w.refused("gsm_sgs_check")
    assert rc == 0, msg
    assert np.array_equal(accept, [e["acc"] for e in exp]), (accept, exp)
    assert np.array_equal(acc_rec[:, 0], accept) and (acc_rec[:, 1:] == 9).all() and (loss_rec[:, 1:] == -7.5).all()
    cur1, nxt1, energy1, state1, res1 = (x.cpu().numpy() for x in (d_cur, d_nxt, energy, state, resampled))
    fresh_e, fresh_s = w.state_init(d_cur, d_trend)
    fresh_e, fresh_s = fresh_e.cpu().numpy(), fresh_s.cpu().numpy()
    r0, r1, c0, c1 = win
    for c, e in enumerate(exp):
        want, bound = (e["ln"], e["bn"]) if e["acc"] else (e["lp"], e["bp"])
        if np.isinf(want):
            assert loss_rec[c, 0] == want
        else:
            assert abs(LD(loss_rec[c, 0]) - want) <= bound, (name, ROLES[c], float(abs(LD(loss_rec[c, 0]) - want) / bound))
        if e["acc"]:
            assert same_bits(cur1[c], nxt[c]) and same_bits(nxt1[c], nxt[c])
            bumped = res0[c].copy()
            bumped[r0:r1, c0:c1] += 1
            assert np.array_equal(res1[c], bumped)
            assert same_bits(energy1[c], fresh_e[c])
            assert state1[c, 3] == e["bad_n"] == fresh_s[c, 3]
            assert same_bits(state1[c, 2], np.float64(loss_rec[c, 0]))
            diff, cb = comp_bound_ok(state1[c], energy1[c])
            print(f"{name} {ROLES[c]}: carried sum off by {float(diff / cb):.3f} of its bound")
            assert diff <= cb
        else:
            assert same_bits(cur1[c], cur[c]) and same_bits(nxt1[c], cur[c])
            assert same_bits(energy1[c], energy0[c]) and same_bits(state1[c], state0[c]) and same_bits(res1[c], res0[c])


@pytest.mark.parametrize("use_trend", [False, True])
def test_finish_refuses_a_halo_over_the_limit(finish_worlds, use_trend):
    (H, W), win, over = ic.finish_windows()["35x34_over"]
    assert over
    w = finish_worlds(H, W)
    n = w.n
    case, cur, nxt, trend = finish_case(H, W, win, use_trend)
    d_cur, d_nxt, d_trend = w.f64(cur), w.f64(nxt), w.f64(trend)
    energy, state = w.state_init(d_cur, d_trend)
    energy0, state0 = energy.cpu().numpy(), state.cpu().numpy()
    resampled = w.i32(np.zeros((n, H, W)))
    accept, loss_rec, acc_rec = run_finish(w, d_cur, d_nxt, d_trend, np.tile(win, (n, 1)), np.zeros(n), energy, state, resampled)
    rc, msg = w.refused("gsm_sgs_check")
    assert rc == E_DEVICE_DATA and "gsm_sgs_check: window outside the grid / larger than 1024 cells" in msg, (rc, msg)
    assert (accept == 0).all() and (acc_rec[:, 0] == 0).all()
    assert same_bits(d_cur.cpu().numpy(), cur) and same_bits(energy.cpu().numpy(), energy0) and same_bits(state.cpu().numpy(), state0)
    assert (resampled.cpu().numpy() == 0).all() and same_bits(loss_rec[:, 0], state0[:, 2])
    assert w.refused("gsm_sgs_check") == (0, "")                                    # the flag was cleared


# ---- gsm_sgs_finish, a sequence --------------------------------------------------------------------------------------------------
def test_finish_sequence_of_200_calls():
    H, W, n, calls = 41, 50, 3, 200
    w = World(H, W, n)
    try:
        case = ic.make_case(H, W, 1)
        trend = case["trend"]
        cur = np.tile(ic.detrended(case)[0], (n, 1, 1))
        guarded = (case["upd"] == 1) & ~np.isnan(cur[0])
        rng = np.random.default_rng(2050)
        d_cur, d_trend = w.f64(cur), w.f64(trend)
        d_nxt = d_cur.clone()
        energy, state = w.state_init(d_cur, d_trend)
        resampled = w.i32(np.zeros((n, H, W)))
        res = np.zeros((n, H, W), np.int32)
        lp, bp, _, _ = ic.score(case, cur, trend)
        lp, bp = list(lp), list(bp)
        n_acc = n_rej = n_inf_inf = 0
        for k in range(calls):
            wins, nxt = [], cur.copy()
            for c in range(n):
                hh, ww = rng.integers(1, 35, 2)
                hh, ww = min(hh, H), min(ww, W)
                r0, c0 = rng.integers(0, H - hh + 1), rng.integers(0, W - ww + 1)
                wins.append((r0, r0 + hh, c0, c0 + ww))
                nxt[c, r0:r0 + hh, c0:c0 + ww] += rng.standard_normal((hh, ww)) / np.sqrt(hh * ww)
                inwin = np.zeros((H, W), bool)
                inwin[r0:r0 + hh, c0:c0 + ww] = True
                if rng.random() < 0.2 and (g := _pick(guarded, inwin, rng)) is not None:
                    nxt[c][g] = case["surf"][g] + 1.0 - trend[g]
                elif rng.random() < 0.5:                                            # a proposal that un-grounds what an earlier one grounded
                    lifted = inwin & guarded & (case["surf"] - (nxt[c] + trend) <= 0)
                    nxt[c][lifted] = (case["surf"] - trend - 700.0)[lifted]
            ln, bn, bad_n, _ = ic.score(case, nxt, trend)
            us, accs = [], []
            for c in range(n):
                ln_c = float("inf") if bad_n[c] > 0 else ln[c]
                if np.isinf(ln_c) or np.isinf(lp[c]):
                    u = float(rng.choice([0.0, 0.3, 0.9]))
                    n_inf_inf += bool(np.isinf(ln_c) and np.isinf(lp[c]))
                else:
                    u = ic.u_at_margin(lp[c], ln_c, bp[c] + bn[c], below=rng.random() < 0.5)
                us.append(u)
                accs.append(ic.decide_ref(lp[c], ln_c, u))
                if accs[-1]:
                    lp[c], bp[c] = ln_c, bn[c]
            d_nxt.copy_(w.f64(nxt))
            accept, _, _ = run_finish(w, d_cur, d_nxt, d_trend, wins, us, energy, state, resampled)
            assert np.array_equal(accept, accs), (k, accept, accs)
            for c in range(n):
                if accs[c]:
                    cur[c] = nxt[c]
                    r0, r1, c0, c1 = wins[c]
                    res[c, r0:r1, c0:c1] += 1
            n_acc += sum(accs)
            n_rej += n - sum(accs)
        assert n_acc >= 20 and n_rej >= 20 and n_inf_inf >= 1, (n_acc, n_rej, n_inf_inf)
        assert same_bits(d_cur.cpu().numpy(), cur) and same_bits(d_nxt.cpu().numpy(), cur)
        assert np.array_equal(resampled.cpu().numpy(), res)
        fresh_e, fresh_s = w.state_init(d_cur, d_trend)
        energy, state, fresh_s = energy.cpu().numpy(), state.cpu().numpy(), fresh_s.cpu().numpy()
        assert same_bits(energy, fresh_e.cpu().numpy())
        _, _, bad_ref, _ = ic.score(case, cur, trend)
        for c in range(n):
            diff, cb = comp_bound_ok(state[c], energy[c])
            print(f"chain {c}: after {calls} calls the carried sum is off by {float(diff / cb):.3f} of 2 u sum e")
            assert diff <= cb
            assert state[c, 3] == bad_ref[c] == fresh_s[c, 3]
        assert w.refused("gsm_sgs_check") == (0, "")
    finally:
        w.close()


# ---- gsm_sgs_decide --------------------------------------------------------------------------------------------------------------
def test_decide_table_at_70_chains():
    rows = ic.decision_rows()
    n = 70
    table = [rows[i % len(rows)] for i in range(n)]
    assert len(rows) < 35                                                       # every row also lands in the second block of 64
    lp = np.array([r[0] for r in table]); ln = np.array([r[1] for r in table])
    bad = np.array([r[2] for r in table], np.int32); u = np.array([r[3] for r in table])
    w = World(5, 7, n, static=False)
    try:
        t = w.torch
        d_lp = w.f64(lp)
        accept = t.full((n,), 9, dtype=t.uint8, device=w.dev)
        loss_rec = t.full((n * REC_STRIDE,), -7.5, dtype=t.float64, device=w.dev)
        acc_rec = t.full((n * REC_STRIDE,), 9, dtype=t.uint8, device=w.dev)
        w.call("gsm_sgs_decide", w.f64(ln), w.i32(bad), w.f64(u), d_lp, accept, loss_rec, acc_rec, REC_STRIDE)
        accept, lp1 = accept.cpu().numpy(), d_lp.cpu().numpy()
        loss_rec, acc_rec = loss_rec.cpu().numpy().reshape(n, REC_STRIDE), acc_rec.cpu().numpy().reshape(n, REC_STRIDE)
    finally:
        w.close()
    ln_eff = np.where(bad > 0, np.inf, ln)
    want = np.array([ic.decide_ref(a, b, c) for a, b, c in zip(lp, ln_eff, u)])
    assert np.array_equal(accept, want), [(i, table[i]) for i in np.flatnonzero(accept != want)]
    assert want.any() and not want.all()
    assert same_bits(lp1, np.where(want, ln_eff, lp))
    assert same_bits(loss_rec[:, 0], lp1) and np.array_equal(acc_rec[:, 0], accept)
    assert (loss_rec[:, 1:] == -7.5).all() and (acc_rec[:, 1:] == 9).all()


# ---- gsm_sgs_commit / gsm_sgs_commit_map -----------------------------------------------------------------------------------------
COMMIT_WINS = [(0, 4, 0, 5), (0, 3, 44, 50), (36, 41, 0, 2), (39, 41, 47, 50), (14, 14, 9, 15), (8, 11, 30, 33), (0, 41, 0, 50), (5, 5, 7, 7)]
COMMIT_ACC = [1, 0, 1, 0, 1, 0, 1, 3]                                           # any non-zero accepts


@pytest.mark.parametrize("whole_map", [False, True])
def test_commit_and_commit_map(whole_map):
    H, W, n = 41, 50, len(COMMIT_WINS)
    rng = np.random.default_rng(77)
    cur, other = rng.standard_normal((n, H, W)), rng.standard_normal((n, H, W))
    cur[:, 3, 3], other[:, 4, 4] = np.nan, np.nan
    res = rng.integers(0, 2 ** 31 - 2, (n, H, W)).astype(np.int32)
    w = World(H, W, n, static=False)
    try:
        d_cur, d_other, d_res = w.f64(cur), w.f64(other), w.i32(res)
        w.call("gsm_sgs_commit_map" if whole_map else "gsm_sgs_commit", d_cur, d_other, d_res, w.i32(COMMIT_WINS), w.u8(COMMIT_ACC))
        got = [x.cpu().numpy() for x in (d_cur, d_other, d_res)]
    finally:
        w.close()
    want_cur, want_other, want_res = cur.copy(), other.copy(), res.copy()
    for c, ((r0, r1, c0, c1), a) in enumerate(zip(COMMIT_WINS, COMMIT_ACC)):
        if a:
            if whole_map:
                want_cur[c] = other[c]
            else:
                want_cur[c, r0:r1, c0:c1] = other[c, r0:r1, c0:c1]
            want_res[c, r0:r1, c0:c1] += 1
        elif not whole_map:
            want_other[c, r0:r1, c0:c1] = cur[c, r0:r1, c0:c1]
    assert same_bits(got[0], want_cur) and same_bits(got[1], want_other) and np.array_equal(got[2], want_res)


# ---- the tail launch through gsm_sgs_iterate -------------------------------------------------------------------------------------
N_ITERS = 3


def iterate(w, fields, n_iters):
    import ctypes as C
    from mcmc_gpu_amd._lib import SgsBatch
    b = SgsBatch()
    for k, v in fields.items():
        setattr(b, k, v.data_ptr() if isinstance(v, w.torch.Tensor) else v)
    w.call("gsm_sgs_iterate", C.byref(b), n_iters)


def empty_lists(w, n_iters):
    """The search operands of gsm_sgs_blocks_batch / gsm_sgs_iterate with an empty cell list for every chain: nothing is simulated."""
    n = w.n
    return dict(zcond=None, x_axis=w.f64(np.arange(w.W) * ic.RES), y_axis=w.f64(np.arange(w.H) * ic.RES), lag_cov=w.f64(np.ones(16)),
                cell_off=w.i32(np.zeros(n_iters * n + 1)), cell_cnt=w.i32(np.zeros(n_iters * n)), cells=w.i32(np.zeros(8)), z=w.f64(np.zeros(4)),
                radius=3.0 * ic.RES, sill=1.0, lag_mi=0, lag_mj=0, hw=3, num_points=8, max_cells=64)


def test_blocks_batch_with_empty_cell_lists_leaves_the_grid_alone():
    """sgs_kernel.hip: sgs_rank_kernel lists no cell, sgs_weights_kernel returns at slot >= cnt, and sgs_sequence_kernel stages the
    window in LDS, skips its chunk loop and stores the window back as it read it: the iterations of the tail tests below score the
    caller's `next`."""
    H, W, n = 41, 50, 3
    w = World(H, W, n)
    try:
        grid = ic.detrended(w.case)
        d_grid = w.f64(grid)
        e = empty_lists(w, 1)
        w.call("gsm_sgs_blocks_batch", d_grid, None, w.i32(ic.tail_windows(H, W)), e["x_axis"], e["y_axis"], e["lag_cov"], 0, 0, e["hw"], e["radius"],
               e["num_points"], e["sill"], e["cell_off"], e["cell_cnt"], e["cells"], e["z"], e["max_cells"])
        assert w.refused("gsm_sgs_check") == (0, "")
        assert same_bits(d_grid.cpu().numpy(), grid) and np.isnan(grid).any()
    finally:
        w.close()


# per role and iteration: the side of p_ref that u takes (True: below), or the u itself where a loss is infinite
TAIL_SIDES = [(True, False, True), (0.0, 0.7, 0.7), (0.5, False, True), (False, True, False), (True, True, True)]


def tail_case(H, W, n, use_trend):
    """cur, next [n, H, W]: next differs from cur inside the three windows of the three iterations; chain c plays role c % 5
    (1: grounded in the second window, 2: grounded in the first)."""
    case = ic.make_case(H, W, n)
    cur, trend = trend_case(case, use_trend)
    cur = cur.copy()
    nxt = cur.copy()
    wins = ic.tail_windows(H, W)
    for c in range(n):
        rng = np.random.default_rng([H, W, c, 5])
        guarded = (case["upd"] == 1) & ~np.isnan(cur[c])
        for j, (r0, r1, c0, c1) in enumerate(wins):
            nxt[c, r0:r1, c0:c1] += rng.standard_normal((r1 - r0, c1 - c0)) / np.sqrt(max(1, (r1 - r0) * (c1 - c0)))
            inwin = np.zeros((H, W), bool)
            inwin[r0:r1, c0:c1] = True
            if (c % 5, j) in ((1, 1), (2, 0)) and (g := _pick(guarded, inwin, rng)) is not None:
                nxt[c][g] = case["surf"][g] + 1.0 - (trend[g] if use_trend else 0.0)
    return case, cur, nxt, trend, wins


def tail_reference(case, cur, nxt, trend, wins, n_iters):
    """The reference's iterations on the caller's planes: per iteration the full-grid loss of `next`, the decision, the commit of
    that iteration's window.  u at the margin on the side TAIL_SIDES names; with an infinite loss there is no margin to keep and u is
    the role's number (0.7 where the role names a side)."""
    n = cur.shape[0]
    cur, nxt = cur.copy(), nxt.copy()
    lp0, _, _, _ = ic.score(case, cur, trend)
    lp0 = np.array(lp0, dtype=np.float64)                                       # the caller's loss_prev: an input, exact for both sides
    lp, bp = [LD(x) for x in lp0], [LD(0.0)] * n
    res = np.zeros(cur.shape, np.int32)
    u = np.zeros((n_iters, n)); acc = np.zeros((n_iters, n), bool)
    rec, rec_b = np.zeros((n_iters, n), dtype=LD), np.zeros((n_iters, n), dtype=LD)
    last = None
    for j in range(n_iters):
        ln, bn, bad, _ = ic.score(case, nxt, trend)
        last = (ln, bn, bad)
        r0, r1, c0, c1 = wins[j]
        for c in range(n):
            ln_c = LD(np.inf) if bad[c] > 0 else ln[c]
            side = TAIL_SIDES[c % 5][j]
            if np.isinf(ln_c) or np.isinf(lp[c]):
                u[j, c] = side if isinstance(side, float) else 0.7
            else:
                u[j, c] = ic.u_at_margin(lp[c], ln_c, bp[c] + bn[c], below=side if isinstance(side, bool) else True)
            acc[j, c] = ic.decide_ref(lp[c], ln_c, u[j, c])
            if acc[j, c]:
                lp[c], bp[c] = ln_c, bn[c]
                cur[c, r0:r1, c0:c1] = nxt[c, r0:r1, c0:c1]
                res[c, r0:r1, c0:c1] += 1
            else:
                nxt[c, r0:r1, c0:c1] = cur[c, r0:r1, c0:c1]
            rec[j, c], rec_b[j, c] = lp[c], bp[c]
    return dict(lp0=lp0, u=u, acc=acc, rec=rec, rec_b=rec_b, cur=cur, nxt=nxt, res=res, last=last)


def check_records(loss_rec, ref, label):
    """loss_rec [n, n_iters] of the device against the reference's records: inf is inf, the rest inside the bound."""
    n_iters, n = ref["rec"].shape
    for j in range(n_iters):
        for c in range(n):
            want, got = ref["rec"][j, c], loss_rec[c, j]
            if np.isinf(want) or np.isnan(want):
                assert same_bits(np.float64(got), np.float64(want)), (label, j, c, got, want)
            elif ref["rec_b"][j, c] == 0:
                assert got == np.float64(want), (label, j, c)                   # the caller's own loss_prev, carried through a rejection
            else:
                assert abs(LD(got) - want) <= ref["rec_b"][j, c], (label, j, c, float(abs(LD(got) - want) / ref["rec_b"][j, c]))


@pytest.mark.parametrize("use_trend", [False, True])
@pytest.mark.parametrize("H,W", ic.GPU_GRIDS)
def test_tail_launch_without_a_transformer(H, W, use_trend):
    """Mode 2 of sgs_loss_tail_kernel: three iterations in one call, so the self-resetting ticket is used three times per chain."""
    for n in chains_of(H, W):
        case, cur, nxt, trend, wins = tail_case(H, W, n, use_trend)
        ref = tail_reference(case, cur, nxt, trend, wins, N_ITERS)
        if n >= 3:
            assert ref["acc"].any() and not ref["acc"].all()
            assert (ref["last"][2] > 0).any() and (ref["last"][2] == 0).any()      # guarded and unguarded proposals
            assert np.isinf(ref["rec"][0, 1]) and ref["acc"][1, 1]                  # chain 1 meets (+inf, +inf) and takes it
        w = World(H, W, n)
        try:
            t = w.torch
            d_cur, d_nxt = w.f64(cur), w.f64(nxt)
            out = dict(resampled=w.i32(np.zeros(cur.shape)), loss=w.f64(np.full(n, NAN)), bad=w.i32(np.full(n, -1)), loss_prev=w.f64(ref["lp0"]),
                       accept=t.full((n,), 9, dtype=t.uint8, device=w.dev), loss_rec=w.f64(np.full(n * N_ITERS, NAN)),
                       acc_rec=t.full((n * N_ITERS,), 9, dtype=t.uint8, device=w.dev))
            keep = dict(empty_lists(w, N_ITERS), trend=w.f64(trend), windows=w.i32(np.repeat(np.array(wins), n, axis=0)), u=w.f64(ref["u"]))
            iterate(w, dict(keep, cur=d_cur, next=d_nxt, cell_off_stride=n, qt_n=0, windowed=0, grid_finite=0, **out), N_ITERS)
            assert w.refused("gsm_sgs_check") == (0, "")
            got = {k: v.cpu().numpy() for k, v in out.items()}
            cur1, nxt1 = d_cur.cpu().numpy(), d_nxt.cpu().numpy()
        finally:
            w.close()
        label = f"{H}x{W} n={n} trend={use_trend}"
        acc_rec, loss_rec = got["acc_rec"].reshape(n, N_ITERS), got["loss_rec"].reshape(n, N_ITERS)
        assert np.array_equal(acc_rec.T, ref["acc"]), (label, acc_rec.T, ref["acc"])
        assert np.array_equal(got["accept"], ref["acc"][-1])
        check_records(loss_rec, ref, label)
        assert same_bits(got["loss_prev"], loss_rec[:, -1].copy())
        ln, bn, bad = ref["last"]
        assert (np.abs(got["loss"].astype(LD) - ln) <= bn).all(), label
        assert np.array_equal(got["bad"], bad)
        assert same_bits(cur1, ref["cur"]) and same_bits(nxt1, ref["nxt"]) and np.array_equal(got["resampled"], ref["res"])


# ---- mode 1: a transformer, its two transforms inside the tail launch or not -----------------------------------------------------
QT_GRIDS = [(8, 512), (20, 600)]
QT_NQ = [64, 1024, 1025]
QT_ITERS, QT_CHAINS = 2, 4


def qt_inputs(H, W, nq):
    from sklearn.preprocessing import QuantileTransformer
    case = ic.make_case(H, W, QT_CHAINS)
    cur, trend = trend_case(case, True)
    with np.errstate(invalid="ignore"):
        cur = np.where(np.abs(case["surf"] - (cur + trend)) < 1e-3, cur + 0.4, cur)      # no thickness that the transform's 1e-9 m could flip
    data = cur[0][~np.isnan(cur[0])].reshape(-1, 1)
    qt = QuantileTransformer(n_quantiles=nq, output_distribution="normal", subsample=None).fit(data)
    assert qt.quantiles_.shape[0] == nq
    return case, cur, trend, qt


def qt_reference(case, cur, trend, qt, wins):
    """scikit-learn's transform and inverse transform of the whole map, then the long-double loss, the decision and the commit of the
    whole plane; the bound of iteration j is LOSS_BOUND plus the module docstring's transform term with d = (j + 1) x 1e-9 m."""
    n, H, W = cur.shape
    cur = cur.copy()
    velx, vely = np.abs(case["velx"]).astype(LD), np.abs(case["vely"]).astype(LD)
    AV = ic._grad_ld(velx, -1, ic.RES, True) + ic._grad_ld(vely, -2, ic.RES, True)
    res = np.zeros(cur.shape, np.int32)
    u = np.zeros((QT_ITERS, n)); acc = np.zeros((QT_ITERS, n), bool)
    rec, rec_b = np.zeros((QT_ITERS, n), dtype=LD), np.zeros((QT_ITERS, n), dtype=LD)
    lp = lp0 = bp = None
    for j in range(QT_ITERS):
        scores = qt.transform(cur.reshape(-1, 1))
        prop = qt.inverse_transform(scores).reshape(cur.shape)
        b = ic.with_trend(prop, trend)
        v, A = ic.residual_ld(b, case["surf"], case["velx"], case["vely"], case["dhdt"], case["smb"], ic.RES)
        ln, bn, _ = ic.loss_ld(v, A, case["mc"])
        _, enters = ic.energy_ld(v, case["mc"])
        dv = LD((j + 1) * ic.QT_INV_ATOL) * AV
        bn = bn + np.where(enters, LD(2.0) * np.abs(v) * dv + dv * dv, LD(0.0)).sum(axis=(-2, -1)) / LD(ic.TWO_SIGMA2)
        thick = case["surf"] - b
        with np.errstate(invalid="ignore"):
            assert not (np.abs(thick[:, case["upd"] == 1]) <= QT_ITERS * ic.QT_INV_ATOL).any()      # no thickness the transform's error could flip
        bad = ic.bad_count(b, case["surf"], case["upd"])
        if j == 0:                                                              # the caller's loss_prev: one above, two below the proposal's
            lp0 = np.array([ln[0] - 1, ln[1] - 1, ln[2] + 1, ln[3] - 1], dtype=np.float64)
            lp, bp = [LD(x) for x in lp0], [LD(0.0)] * n
        r0, r1, c0, c1 = wins[j]
        for c in range(n):
            ln_c = LD(np.inf) if bad[c] > 0 else ln[c]
            if np.isinf(ln_c) or np.isinf(lp[c]):
                u[j, c] = 0.5 if c == 1 else 0.0                                 # chain 1 rejects its grounded proposal twice, chain 3 takes it: (+inf, +inf) next
            else:
                u[j, c] = ic.u_at_margin(lp[c], ln_c, bp[c] + bn[c], below=(c + j) % 2 == 0)
            acc[j, c] = ic.decide_ref(lp[c], ln_c, u[j, c])
            if acc[j, c]:
                lp[c], bp[c] = ln_c, bn[c]
                cur[c] = prop[c]
                res[c, r0:r1, c0:c1] += 1
            rec[j, c], rec_b[j, c] = lp[c], bp[c]
    return dict(lp0=lp0, u=u, acc=acc, rec=rec, rec_b=rec_b, cur=cur, res=res, bad=bad)


def qt_child(tail_qt):
    """Every grid and table size through gsm_sgs_iterate with a transformer and the batch's tail_qt (include/gsm.h: GSM_TAIL_QT_ON /
    GSM_TAIL_QT_OFF), every output plane kept."""
    saved = {}
    for H, W in QT_GRIDS:
        for nq in QT_NQ:
            case, cur, trend, qt = qt_inputs(H, W, nq)
            wins = ic.tail_windows(H, W)[:QT_ITERS]
            ref = qt_reference(case, cur, trend, qt, wins)
            n = QT_CHAINS
            w = World(H, W, n)
            try:
                t = w.torch
                d_cur = w.f64(cur)
                d_nxt, d_prop = t.full_like(d_cur, NAN), t.full_like(d_cur, NAN)
                out = dict(cur=d_cur, next=d_nxt, proposed=d_prop, resampled=w.i32(np.zeros(cur.shape)), loss=w.f64(np.full(n, NAN)),
                           bad=w.i32(np.full(n, -1)), loss_prev=w.f64(ref["lp0"]), accept=t.full((n,), 9, dtype=t.uint8, device=w.dev),
                           loss_rec=w.f64(np.full(n * QT_ITERS, NAN)), acc_rec=t.full((n * QT_ITERS,), 9, dtype=t.uint8, device=w.dev))
                keep = dict(empty_lists(w, QT_ITERS), trend=w.f64(trend), windows=w.i32(np.repeat(np.array(wins), n, axis=0)), u=w.f64(ref["u"]),
                            qt_quantiles=w.f64(qt.quantiles_[:, 0]), qt_references=w.f64(qt.references_))
                iterate(w, dict(keep, cell_off_stride=n, qt_n=nq, windowed=0, grid_finite=0, tail_qt=tail_qt, **out), QT_ITERS)
                assert w.refused("gsm_sgs_check") == (0, "")
                for k, v in out.items():
                    saved[f"{H}x{W}_{nq}_{k}"] = v.cpu().numpy()
            finally:
                w.close()
            print(f"CASE {H}x{W} nq={nq}")
    return saved


@pytest.fixture(scope="module")
def qt_runs():
    pytest.importorskip("sklearn.preprocessing")
    from mcmc_gpu_amd._lib import TAIL_QT_OFF, TAIL_QT_ON
    return {"1": qt_child(TAIL_QT_ON), "0": qt_child(TAIL_QT_OFF)}


@pytest.mark.parametrize("nq", QT_NQ)
@pytest.mark.parametrize("H,W", QT_GRIDS)
def test_tail_launch_with_a_transformer(qt_runs, H, W, nq):
    """8 x 512 with nq <= 1024 takes the transforms into the tail launch (per + 2 W = 2048), 20 x 600 and nq = 1025 fall back to the
    stand-alone transforms: either way both settings of the batch's tail_qt give the same bits, and both agree with scikit-learn.  `next`
    is compared where the last iteration was rejected: after an accepted one the tail launch leaves T(proposed) there, ready for the
    next batch, and the stand-alone path T(cur) of before the iteration."""
    case, cur, trend, qt = qt_inputs(H, W, nq)
    wins = ic.tail_windows(H, W)[:QT_ITERS]
    ref = qt_reference(case, cur, trend, qt, wins)
    assert ref["acc"].any() and not ref["acc"].all()
    assert np.isinf(ref["rec"][0, 3]) and ref["acc"][1, 3]                          # chain 3 meets (+inf, +inf) and takes it
    on, off = ({k[len(f"{H}x{W}_{nq}_"):]: v for k, v in qt_runs[f].items() if k.startswith(f"{H}x{W}_{nq}_")} for f in ("1", "0"))
    assert set(on) == set(off) and len(on) == 10
    rejected_last = ~ref["acc"][-1]
    assert rejected_last.any()
    for k in on:
        if k == "next":
            assert same_bits(on[k][rejected_last], off[k][rejected_last]), k
        else:
            assert same_bits(on[k], off[k]), k
    n = QT_CHAINS
    for label, got in (("tail", on), ("stand-alone", off)):
        acc_rec, loss_rec = got["acc_rec"].reshape(n, QT_ITERS), got["loss_rec"].reshape(n, QT_ITERS)
        assert np.array_equal(acc_rec.T, ref["acc"]), (label, acc_rec.T, ref["acc"])
        assert np.array_equal(got["accept"], ref["acc"][-1])
        check_records(loss_rec, ref, label)
        assert np.array_equal(got["bad"], ref["bad"]) and np.array_equal(got["resampled"], ref["res"])
        assert np.array_equal(np.isnan(got["cur"]), np.isnan(ref["cur"]))
        assert np.nanmax(np.abs(got["cur"] - ref["cur"])) <= QT_ITERS * ic.QT_INV_ATOL
        scores = qt.transform(ref["cur"][rejected_last].reshape(-1, 1)).reshape(-1)
        assert np.array_equal(np.isnan(got["next"][rejected_last].reshape(-1)), np.isnan(scores))


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def entry_args(w):
    """Valid argument lists of the six stand-alone entry points (name -> {argument: value}), outputs filled with a sentinel."""
    t = w.torch
    n, HW = w.n, w.H * w.W
    plane = lambda: t.full((n * HW,), -3.25, dtype=t.float64, device=w.dev)
    per = lambda: t.full((n,), -3.25, dtype=t.float64, device=w.dev)
    i32 = lambda k: t.zeros(k, dtype=t.int32, device=w.dev)
    u8 = lambda k: t.zeros(k, dtype=t.uint8, device=w.dev)
    return {
        "gsm_sgs_loss": dict(beds=plane(), trend=None, loss=per(), bad=i32(n)),
        "gsm_sgs_decide": dict(loss_next=per(), bad=i32(n), u=per(), loss_prev=per(), accept=u8(n), loss_rec=per(), acc_rec=u8(n), rec_stride=1),
        "gsm_sgs_state_init": dict(beds=plane(), trend=None, energy=plane(), state=t.zeros(4 * n, dtype=t.float64, device=w.dev)),
        "gsm_sgs_finish": dict(cur=plane(), next=plane(), trend=None, energy=plane(), state=t.zeros(4 * n, dtype=t.float64, device=w.dev),
                               windows=i32(4 * n), u=per(), resampled=i32(n * HW), accept=u8(n), loss_rec=per(), acc_rec=u8(n), rec_stride=1),
        "gsm_sgs_commit_map": dict(cur=plane(), proposed=plane(), resampled=i32(n * HW), windows=i32(4 * n), accept=u8(n)),
        "gsm_sgs_commit": dict(cur=plane(), next=plane(), resampled=i32(n * HW), windows=i32(4 * n), accept=u8(n)),
    }


NULLS = {"gsm_sgs_loss": ("beds", "loss", "bad"), "gsm_sgs_decide": ("loss_next", "bad", "u", "loss_prev", "accept"),
         "gsm_sgs_state_init": ("beds", "energy", "state"),
         "gsm_sgs_finish": ("cur", "next", "energy", "state", "windows", "u", "resampled", "accept"),
         "gsm_sgs_commit_map": ("cur", "proposed", "resampled", "windows", "accept"),
         "gsm_sgs_commit": ("cur", "next", "resampled", "windows", "accept")}
NEEDS_STATIC = ("gsm_sgs_loss", "gsm_sgs_state_init", "gsm_sgs_finish")


def _refusal(w, entry, change, code, text):
    args = {**entry_args(w)[entry], **change}
    before = {k: v.clone() for k, v in args.items() if isinstance(v, w.torch.Tensor)}
    rc, msg = w.refused(entry, *args.values())
    assert rc == code and f"{entry}: {text}" in msg, (entry, change, rc, msg)
    for k, v in before.items():
        assert w.torch.equal(v, args[k]), f"{entry} with {sorted(change)}: {k} was written"


@pytest.mark.parametrize("entry", sorted(NULLS))
def test_refusals_of_the_stand_alone_entry_points(entry):
    w = World(5, 7, 2)
    try:
        for name in NULLS[entry]:
            _refusal(w, entry, {name: None}, E_ARG, "NULL pointer")
        if "rec_stride" in entry_args(w)[entry]:
            _refusal(w, entry, dict(rec_stride=0), E_ARG, "rec_stride must be >= 1")
            _refusal(w, entry, dict(rec_stride=-1, loss_rec=None), E_ARG, "rec_stride must be >= 1")
            rc, msg = w.refused(entry, *{**entry_args(w)[entry], "rec_stride": 0, "loss_rec": None, "acc_rec": None}.values())
            assert rc == 0, msg                                                 # no record pointer: the stride is not read
        rc, msg = w.refused(entry, *entry_args(w)[entry].values())            # and the valid call is taken
        assert rc == 0, msg
        assert w.refused("gsm_sgs_check") == (0, "")
    finally:
        w.close()
    if entry in NEEDS_STATIC:
        w = World(5, 7, 2, static=False)
        try:
            _refusal(w, entry, {}, E_STATE, "call gsm_set_static first")
        finally:
            w.close()
        w = World(5, 7, 2, state_dtype="f32")
        try:
            _refusal(w, entry, {}, E_UNSUPPORTED, "fp64 beds only")
        finally:
            w.close()
