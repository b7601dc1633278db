"""CPU: the `mode` keyword of interpolate.sgs / sgs_many / _run -- its argument errors, raised before any device work, and its
default -- and, with NumPy alone, that the cases of tests/interp_sgs_pcg64_common.py reach what the device test needs them
for: the ziggurat's tail path, a generator that enters with a cached 32-bit word, a shuffle that leaves one behind."""
import inspect
import warnings

import numpy as np
import pytest

import interp_sgs_common as ic
import interp_sgs_pcg64_common as pc


def _small():
    xx, yy, grid, cases = ic.small()
    vario, kw, _ = cases["a"]
    return xx, yy, grid, vario, kw


def _many(seeds, **extra):
    from mcmc_gpu_amd import interpolate
    xx, yy, grid, vario, kw = _small()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return interpolate.sgs_many(xx, yy, grid, vario, seeds, **kw, **extra)


def test_unknown_mode_raises_before_device_work():
    from mcmc_gpu_amd import interpolate
    xx, yy, grid, vario, kw = _small()
    with pytest.raises(ValueError, match="mode must be 'replay' or 'pcg64'"):
        _many([1, 2], mode="philox")
    with pytest.raises(ValueError, match="mode must be 'replay' or 'pcg64'"):
        _many([], mode="philox")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(ValueError, match="mode must be 'replay' or 'pcg64'"):
            interpolate.sgs(xx, yy, grid, vario, seed=1, mode="device", **kw)
        plan = interpolate._Plan(xx, yy, grid, vario, kw["radius"], kw["num_points"], kw["ktype"], None, None, None, None)
    g = np.random.default_rng(3)
    before = g.bit_generator.state
    with pytest.raises(ValueError, match="mode must be 'replay' or 'pcg64'"):
        interpolate._run(plan, [g], mode="PCG64")
    assert g.bit_generator.state == before


def test_pcg64_mode_refuses_another_bit_generator():
    mt = np.random.Generator(np.random.MT19937(5))
    before = mt.bit_generator.state["state"]["pos"]
    with pytest.raises(ValueError, match="PCG64"):
        _many([1, mt], mode="pcg64")
    with pytest.raises(ValueError, match="PCG64"):
        _many([np.random.Generator(np.random.PCG64DXSM(5))], mode="pcg64")
    assert mt.bit_generator.state["state"]["pos"] == before


def test_pcg64_mode_refuses_the_same_generator_twice():
    g = np.random.default_rng(9)
    before = g.bit_generator.state
    with pytest.raises(ValueError, match="listed twice"):
        _many([4, g, 5, g], mode="pcg64")
    with pytest.raises(ValueError, match="listed twice"):
        _many([g, np.random.Generator(g.bit_generator)], mode="pcg64")       # two Generators on one bit generator: one stream
    assert g.bit_generator.state == before


def test_replay_is_the_default_and_is_passed_down(monkeypatch):
    """mode='replay' spelled out is the call without the keyword: the default of all three functions, and sgs -> sgs_many ->
    _run hand the same value down (the device result of both spellings: tests/test_gpu_interp_sgs_pcg64.py)."""
    from mcmc_gpu_amd import interpolate
    for fn in (interpolate.sgs, interpolate.sgs_many, interpolate._run):
        assert inspect.signature(fn).parameters["mode"].default == "replay"
    seen = []

    def fake_run(plan, gens, segment_cells=None, device=None, trace=False, mode="replay"):
        seen.append((mode, [g.bit_generator.state for g in gens], segment_cells, device, trace))
        return np.repeat(plan.grid_ns[None], len(gens), axis=0), None

    monkeypatch.setattr(interpolate, "_run", fake_run)
    xx, yy, grid, vario, kw = _small()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = interpolate.sgs_many(xx, yy, grid, vario, [3, 4], **kw)
        b = interpolate.sgs_many(xx, yy, grid, vario, [3, 4], mode="replay", **kw)
        c = interpolate.sgs(xx, yy, grid, vario, seed=3, **kw)
        d = interpolate.sgs(xx, yy, grid, vario, seed=3, mode="replay", **kw)
        interpolate.sgs(xx, yy, grid, vario, seed=3, mode="pcg64", **kw)
    assert seen[0] == seen[1] and seen[2] == seen[3] and seen[0][0] == seen[2][0] == "replay" and seen[4][0] == "pcg64"
    assert np.array_equal(a, b, equal_nan=True) and np.array_equal(c, d, equal_nan=True)


# ---- the device test's cases are fair (NumPy alone) -------------------------------------------------------------------------
def test_the_many_normals_case_draws_from_the_ziggurats_tail():
    n, values, kind, R, pending = pc.cases()[pc.MANY_NORMALS]
    assert kind == "normal"
    draws = [pc.plan(n, values, kind).draws(g)[1] for g in pc.generators(R, pending)]
    assert sum(d.size for d in draws) >= 50_000
    assert any((np.abs(d) > pc.ZIGGURAT_NOR_R).any() for d in draws)


def test_a_pending_generator_enters_with_a_cached_word():
    for cid, (n, values, kind, R, pending) in pc.cases().items():
        has = [g.bit_generator.state["has_uint32"] for g in pc.generators(R, pending)]
        assert sum(has) == (1 if pending else 0), cid
        assert not pending or has[min(1, R - 1)] == 1, cid
    assert sum(c[4] for c in pc.cases().values()) >= 16
    g = np.random.default_rng(1)
    g.integers(0, 10)
    assert g.bit_generator.state["has_uint32"] == 1


def test_a_shuffle_leaves_a_cached_word_behind():
    """The normals and uniforms are 64-bit draws and leave the cached word alone, so the state after _Plan.draws shows what the
    shuffle left: a generator that entered without a cached word and ends with one."""
    n, values, kind, R, pending = pc.cases()[pc.CACHED_AFTER_SHUFFLE]
    gens = pc.generators(R, pending)
    assert gens[0].bit_generator.state["has_uint32"] == 0
    path, _ = pc.plan(n, values, kind).draws(gens[0])
    assert path.size > 0 and gens[0].bit_generator.state["has_uint32"] == 1
    # the 30 x 30 end-to-end check of the device test ends the same way
    from mcmc_gpu_amd import interpolate
    xx, yy, grid, vario, kw = pc.small_30()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plan = interpolate._Plan(xx, yy, grid, vario, kw["radius"], kw["num_points"], kw["ktype"], None, None, None, kw["bounds"])
    g = np.random.default_rng(pc.SEED_30)
    path, d = plan.draws(g)
    assert path.size == int(np.isnan(grid).sum()) and g.bit_generator.state["has_uint32"] == 1


def test_the_cases_cover_every_size_value_pattern_realisation_count_and_draw_kind():
    cs = pc.cases()
    assert {c[0] for c in cs.values()} == set(pc.N_CELLS)
    assert {c[1] for c in cs.values()} == {"none", "all", "some"} and {c[2] for c in cs.values()} == {"normal", "truncated"}
    assert {c[3] for c in cs.values()} == {1, 3, 70}
    n, values, kind, _, _ = cs["129-some-truncated"]
    p = pc.plan(n, values, kind)
    path, d = p.draws(np.random.default_rng(0))
    lo, hi = p.bounds[0].ravel()[path], p.bounds[1].ravel()[path]
    assert (lo == hi).any() and np.isnan(lo).any() and np.isnan(hi).any()
    assert np.all(d[lo == hi] == 0.0) and np.all(d[np.isnan(lo) | np.isnan(hi)] != 0.0)
    assert pc.plan(n, "all", "normal").draws(np.random.default_rng(0))[0].size == 0
