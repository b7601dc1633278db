"""CPU: the bar of tests/test_gpu_sgs_iter.py is fair, and its case lists hit what they claim (tests/sgs_iter_common.py).

The project's own fp64 restatement of the residual (oracle/mcmc_oracle.mc_residual) and numpy's nansum must lie inside the bounds
derived for the device from the operation count, against the long-double reference, on every grid, chain count and trend case;
the worst ratios are printed.  decide_ref is oracle/sgs_oracle.py's inline decision on the finite rows."""
import numpy as np
import pytest

import mcmc_oracle as orc
import sgs_iter_common as ic

LD = ic.LD


def _cases():
    for H, W in ic.GRIDS:
        for n in ic.CHAINS:
            if n == 70 and (H, W) not in ic.SMALL_GRIDS:
                continue
            yield H, W, n


def test_fp64_restatement_lies_inside_the_derived_bounds():
    worst_res, worst_loss, rel = 0.0, 0.0, []
    for H, W, n in _cases():
        case = ic.make_case(H, W, n)
        for trend in (None, case["trend"]):
            beds = case["beds"] if trend is None else ic.detrended(case)
            b = ic.with_trend(beds, trend)
            v, A = ic.residual_ld(b, case["surf"], case["velx"], case["vely"], case["dhdt"], case["smb"], ic.RES)
            loss, bound, bad, s = ic.score(case, beds, trend)
            for c in range(n):
                v64 = orc.mc_residual(b[c], case["surf"], case["velx"], case["vely"], case["dhdt"], case["smb"], ic.RES)
                assert np.array_equal(np.isnan(v64), np.isnan(v[c]))
                ok = ~np.isnan(v64)
                r = np.abs(v64.astype(LD) - v[c])[ok] / (LD(8.0) * LD(ic.U) * A[c][ok])
                worst_res = max(worst_res, float(r.max()))
                loss64 = np.nansum(np.square(v64[case["mc"] == 1])) / (2 * ic.SIGMA ** 2)
                worst_loss = max(worst_loss, float(abs(LD(loss64) - loss[c]) / bound[c]))
                rel.append(float(bound[c] / loss[c]))
                assert int(bad[c]) == int(np.sum((case["surf"] - b[c] <= 0)[case["upd"] == 1]))
    print(f"worst residual ratio {worst_res:.3f}, worst loss ratio {worst_loss:.3f}, loss bound {min(rel):.2e} .. {max(rel):.2e} relative")
    assert worst_res <= 1.0
    assert worst_loss <= 1.0


def test_nan_cells_take_their_neighbours_out_of_the_sum():
    case = ic.make_case(41, 50, 1)
    v, _ = ic.residual_ld(case["beds"], case["surf"], case["velx"], case["vely"], case["dhdt"], case["smb"], ic.RES)
    H, W = 41, 50
    for g in case["nan_cells"]:
        r, c = divmod(int(g), W)
        for rr, cc in ((r, c - 1), (r, c + 1), (r - 1, c), (r + 1, c)):
            if 0 <= rr < H and 0 <= cc < W:
                assert np.isnan(v[0, rr, cc])
        if 0 < r < H - 1 and 0 < c < W - 1:
            assert not np.isnan(v[0, r, c]) or np.isnan(case["beds"][0, r, c - 1:c + 2]).sum() > 1     # its own value is not in its stencil
    e, enters = ic.energy_ld(v, case["mc"])
    assert (e[~enters] == 0).all() and enters.sum() < (case["mc"] == 1).sum()


def test_decide_ref_is_the_oracles_inline_decision():
    """oracle/sgs_oracle.py:278-283 restated on the rows without NaN or inf - inf."""
    rows = [r for r in ic.decision_rows() if not (np.isnan(r[0]) or np.isnan(r[1]) or (np.isinf(r[0]) and (np.isinf(r[1]) or r[2] > 0)))]
    assert len(rows) >= 11
    for lp, ln, bad, u in rows:
        loss_next = np.inf if bad > 0 else ln
        with np.errstate(under="ignore", over="ignore"):
            if lp > loss_next:
                acceptance_rate = 1
            else:
                acceptance_rate = min(1, np.exp(lp - loss_next))
        assert ic.decide_ref(lp, loss_next, u) == bool(u <= acceptance_rate)
    inf, nan = float("inf"), float("nan")
    assert ic.decide_ref(inf, inf, 0.9) and ic.decide_ref(nan, 3.0, 0.5) and ic.decide_ref(3.0, nan, 0.5)      # min(1, nan) == 1
    assert ic.decide_ref(1.0, 2000.0, 0.0) and not ic.decide_ref(1.0, 2000.0, 5e-324)
    assert ic.decide_ref(7.5, 7.5, 1.0) and not ic.decide_ref(3.0, 3.75, np.exp(-0.75) * (1 + 1e-9))


def test_case_lists_hit_what_they_claim():
    parts, per = ic.loss_parts(32, 33)
    assert (parts, per) == (2, 528) and per % 33 == 0                       # two parts, but of 16 whole rows each
    assert ic.loss_parts(33, 32) == (2, 528) and 528 % 32 == 16             # the boundary at cell 528 is mid-row
    assert 684 % 50 != 0 and (2 * 684) % 50 != 0                            # and so are both boundaries of 41 x 50
    assert ic.loss_parts(33, 31)[0] == 1 and ic.loss_parts(41, 50) == (3, 684) and 3 * 684 > 2050 > 2 * 684       # ragged last part
    parts, per = ic.loss_parts(8, 512)
    assert parts == 4 and per + 2 * 512 == ic.KTAIL_TILE                    # the QT tail's limit exactly
    parts, per = ic.loss_parts(20, 600)
    assert per + 2 * 600 == 2200 > ic.KTAIL_TILE
    assert ic.loss_parts(256, 257)[0] == 64 and (256 * 257 + 1023) // 1024 > 64
    wins = ic.finish_windows()
    for name, ((H, W), win, over) in wins.items():
        r0, r1, c0, c1 = win
        assert 0 <= r0 <= r1 <= H and 0 <= c0 <= c1 <= W, name              # inside the grid
        assert (ic.halo_cells(win, H, W) > ic.KSGS_HALO_MAX) == over, name
    assert ic.halo_cells(wins["34x34"][1], 41, 50) == 1296 and ic.halo(wins["34x34"][1], 41, 50) == (2, 38, 4, 40)
    assert ic.halo_cells(wins["16x70"][1], 20, 600) == 18 * 72 == 1296
    assert ic.halo_cells(wins["35x34_over"][1], 41, 50) == 37 * 36
    assert ic.halo(wins["whole_20x20"][1], 20, 20) == (0, 20, 0, 20)
    assert wins["empty"][1][0] == wins["empty"][1][1]
    for H, W in ic.GRIDS:
        ws = ic.tail_windows(H, W)
        rows = np.zeros(H + 1, int)
        for r0, r1, c0, c1 in ws:
            assert 0 <= r0 <= r1 <= H and 0 <= c0 <= c1 <= W and (r1 - r0) * (c1 - c0) <= ic.KSGS_MAX_WIN
            rows[r0:r1] += 1
        assert rows.max() <= 1                                              # disjoint row bands
    assert any((r1 - r0, c1 - c0) == (4, 256) for r0, r1, c0, c1 in ic.tail_windows(8, 512))
    assert any((r1 - r0, c1 - c0) == (32, 32) for r0, r1, c0, c1 in ic.tail_windows(256, 257))


@pytest.mark.parametrize("H,W", ic.GRIDS)
def test_guard_fires_on_some_beds_and_not_on_others(H, W):
    case = ic.make_case(H, W, 3)
    for trend in (None, case["trend"]):
        beds = case["beds"] if trend is None else ic.detrended(case)
        bad = ic.bad_count(ic.with_trend(beds, trend), case["surf"], case["upd"])
        assert bad[0] == 0 and bad[2] == 0 and bad[1] > 0, bad            # even chains afloat, odd chains grounded on the patch
    assert (case["mc"] != case["upd"]).any() and (case["mc"] == 0).any()


def test_proposals_of_the_device_tests_are_what_their_roles_say():
    """The planes that tests/test_gpu_sgs_iter.py sends to gsm_sgs_finish and gsm_sgs_iterate, scored by the reference alone: per
    window a guarded and an unguarded proposal, accepted and rejected chains, every u inside [0, 1)."""
    import test_gpu_sgs_iter as dev
    for name, ((H, W), win, over) in ic.finish_windows().items():
        for use_trend in (False, True):
            case, cur, nxt, trend = dev.finish_case(H, W, win, use_trend)
            exp = dev.finish_expect(case, cur, nxt, trend)
            assert all(0.0 <= e["u"] < 1.0 for e in exp), name
            outside = np.ones((H, W), bool)
            outside[win[0]:win[1], win[2]:win[3]] = False
            assert np.array_equal(cur[:, outside], nxt[:, outside], equal_nan=True)          # next == cur outside the window
            if (win[1] - win[0]) * (win[3] - win[2]) > 0:
                assert exp[3]["bad_n"] > 0 and exp[0]["bad_n"] == 0, name
                assert {e["acc"] for e in exp} == {True, False}, name
                assert exp[0]["ln"] > exp[0]["lp"] and exp[1]["ln"] > exp[1]["lp"] and exp[2]["ln"] < exp[2]["lp"], name
    for H, W in ic.GPU_GRIDS:
        case, cur, nxt, trend, wins = dev.tail_case(H, W, 3, True)
        ref = dev.tail_reference(case, cur, nxt, trend, wins, dev.N_ITERS)
        assert ((ref["u"] >= 0) & (ref["u"] < 1)).all()
        assert ref["acc"].any() and not ref["acc"].all()
        assert (ref["last"][2] > 0).any() and (ref["last"][2] == 0).any()
        assert np.isinf(ref["rec"][0, 1]) and ref["acc"][1, 1]                              # a chain meets (+inf, +inf)
