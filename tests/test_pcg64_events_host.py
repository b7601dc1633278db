"""not gpu: every case of tests/pcg64_event_cases.py reaches the stream event it is there for, shown with NumPy and
oracle/pcg64_oracle.py alone -- the start is a start of NumPy's own ziggurat walk, it sits in the lane and window the case names,
the tail loop runs as often as it says, the Lemire rejection falls on the half it says and leaves has_uint32 as it says.  The
walk that says so is itself pinned against numpy.random.Generator on every case.  tests/test_gpu_pcg64_events.py runs the same
cases on the device."""
import numpy as np
import pytest

import pcg64_event_cases as ec


@pytest.mark.parametrize("case", ec.CASES, ids=lambda c: c.name)
def test_case_reaches_its_event(case):
    ec.check(case)
    if case.event == "lemire":
        return
    # the walk behind the check is NumPy's: same normals bit for bit, same number of draws consumed
    v = ec.view(case)
    g = ec.generator(v.start)
    want = g.standard_normal(v.count)
    assert np.array_equal(v.values.view(np.uint64), want.view(np.uint64))
    behind = ec.generator(v.start)
    behind.bit_generator.advance(v.n_draws)
    assert g.bit_generator.state["state"] == behind.bit_generator.state["state"]
    assert [a[0] for a in v.att] == sorted({a[0] for a in v.att}) and v.att[0][0] == 0


def test_every_listed_event_has_a_case_in_each_decoder():
    """(event, params that matter) per harness: what the decoder's branches need, one-wave through 'grid', four-wave through 'draw'."""
    have = {(c.harness, c.event, tuple(sorted((k, v) for k, v in c.params.items() if k not in ("H", "stream")))) for c in ec.CASES}

    def has(harness, event, **need):
        return any(h == harness and e == event and all((k, v) in p for k, v in need.items()) for h, e, p in have)

    for hn in ("grid", "draw"):
        assert has(hn, "tail", lane=0, runs=1) and has(hn, "tail", lane=0, runs=2) and has(hn, "tail", lane=0, min_runs=3)
        for lane in (1, 31, 63):
            assert has(hn, "tail", lane=lane)
        assert has(hn, "two_tails") and has(hn, "wedge_wedge") and has(hn, "wedge_taillook")
        assert has(hn, "wedge63", accepted=True) and has(hn, "wedge63", accepted=False)
        assert has(hn, "end_fast") and has(hn, "end_wacc", lane=63) and has(hn, "after", what="wedge") and has(hn, "after", what="tail")
        assert any(h == hn and e == "end_wacc" and dict(p)["lane"] < 63 for h, e, p in have)
        assert has(hn, "rej_before_last") and has(hn, "end_tail")
    for w in (1, 2, 3):
        assert has("draw", "tail", window=w, lane=0)
    for w in (1, 3):
        assert any(h == "draw" and e == "tail" and dict(p).get("window") == w and dict(p)["lane"] > 0 for h, e, p in have)
        assert has("draw", "wedge63", window=w)
    for w in range(4):
        assert has("draw", "end_inside", window=w)
    assert has("draw", "cut_before_end") and has("draw", "end_fast", last=255)
    for pl in (1, 2):
        assert has("draw", "tail", plane=pl)
    planes2 = {c.shape[5] > 0 for c in ec.CASES if c.harness == "draw" and c.params.get("plane") == 2}
    assert planes2 == {False, True}                                   # plane 2 consumed unstored, and stored
    assert {c.shape for c in ec.CASES if c.harness == "grid"} >= {1, 63, 64, 65}
    assert {int(np.prod(ec.pairs(c.shape)[:, 0])) for c in ec.CASES if c.harness == "draw"} >= {64, 256}
    pats = {(c.harness, c.params.get("stream", "rf"), c.params["pattern"]) for c in ec.CASES if c.event == "lemire"}
    assert {("draw", "ch", ("lH", "L")), ("draw", "ch", ("L", "hL")), ("draw", "ch", ("lhL", "H")), ("draw", "rf", ("lH",)),
            ("small", "rf", ("lH", "L")), ("small", "rf", ("H", "L", "hL"))} <= pats
    assert has("small", "tail") and has("small", "end_wacc")
    assert len({c.name for c in ec.CASES}) == len(ec.CASES)


def test_states_pack_as_the_engine_packs_them():
    from mcmc_gpu_amd.engine import GsmEngine
    gens = [ec.generator(ec.words(c)) for c in ec.CASES]
    packed = GsmEngine.pack_pcg64_states(gens)
    assert [tuple(int(x) for x in row) for row in packed] == [ec.words(c) for c in ec.CASES]
    assert GsmEngine.unpack_pcg64_states(packed) == [g.bit_generator.state for g in gens]


def test_constructed_draw_has_the_chosen_halves():
    for lo, hi in ((0, 0), (0xFFFFFFFF, 1), (0x12345678, 0x9ABCDEF0)):
        g = ec.generator(ec.constructed(lo, hi, salt=lo & 7))
        assert int(g.bit_generator.random_raw(1)[0]) == (hi << 32) | lo
    for n in (25, 96, 15):
        w = ec.rejected_word(n, 0)
        assert (w * n & ec.M32) < (1 << 32) % n
    assert (1 << 32) % 96 == 64 and (1 << 32) % 25 == 21


def test_the_literal_table_is_what_the_finder_finds():
    assert ec.find_all() == ec.CASES
