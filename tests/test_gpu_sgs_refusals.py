"""GPU: what the SGS and kriging entry points of libgsm_hip refuse, with which code and which text -- the contract that the
kernels' shared search setup, the named device flags and the flag decoders have to keep.

Part 1: the argument refusals of gsm_sgs_blocks, gsm_sgs_blocks_batch, gsm_sgs_iterate, gsm_sgs_grid, gsm_sgs_grid_local,
gsm_krige_grid and gsm_krige_grid_local, one row per refusal: every other argument is valid, the call launches nothing, and the
output arrays keep the sentinel they were filled with.  "Simple kriging without means" cannot reach those entry points:
gsm_sgs_set_kriging, the only way to select simple kriging, refuses a NULL mean itself; that refusal is the row.

Part 2: the device flags that no other test reaches -- a window outside the grid (1), a listed cell outside its window (2), a
grid without any value (4, through the library directly: the Python layer refuses such a grid before the device sees it) and no
block centre inside the region mask (16) -- on 8 x 8 and 12 x 12 grids of spacing 1.  Each case: code, text, and a correct call
on the same handle afterwards gives what it gave before (the flag was cleared)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E_ARG, E_STATE, E_UNSUPPORTED, E_DEVICE_DATA = -1, -2, -4, -5
SENTINEL, SENTINEL_I = -12345.5, -77
VARIO = dict(azimuth=0.0, nugget=0.0, major_range=4.0, minor_range=4.0, sill=1.0, vtype="exponential")
RADIUS, HW, NPTS, MAX_CELLS = 3.0, 3, 8, 16


class _World:
    """One handle on an H x H grid of spacing 1 with the operands every entry point takes."""

    def __init__(self, H, n_chains):
        import torch
        from mcmc_gpu_amd import sgs
        from mcmc_gpu_amd.engine import GsmEngine
        self.torch, self.H, self.n = torch, H, n_chains
        self.eng = GsmEngine(H, H, n_chains)
        self.dev = self.eng.dev
        self.xs, self.ys = self.f64(np.arange(H)), self.f64(np.arange(H))
        self.lag = self.f64(sgs.lag_cov_table(VARIO, HW, 1.0, 1.0, H - 1, H - 1))
        self.local = self.f64(np.tile([0.25, -0.0, 0.0, 0.25, 1.0, 0.0], (H * H, 1)))       # interpolate._local_table's rows of VARIO
        self.field = np.random.default_rng(11).standard_normal((H, H))

    def f64(self, a):
        return self.torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(self.dev)

    def i32(self, a):
        return self.torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32)).to(self.dev)

    def full(self, n, value, dtype=None):
        return self.torch.full((n,), value, dtype=dtype or self.torch.float64, device=self.dev)

    def zeros(self, n, dtype):
        return self.torch.zeros(n, dtype=dtype, device=self.dev)

    def call(self, name, args):
        """lib.<name>(handle, *args.values(), stream) -> (code, gsm_last_error)."""
        torch = self.torch
        vals = [C.c_void_p(v.data_ptr()) if isinstance(v, torch.Tensor) else v for v in args.values()]
        with torch.cuda.device(self.dev):
            rc = getattr(self.eng.lib, name)(self.eng.h, *vals, self.eng._stream())
        return rc, self.eng.lib.gsm_last_error(self.eng.h).decode()

    def iterate(self, fields, n_iters=1):
        from mcmc_gpu_amd._lib import SgsBatch
        torch = self.torch
        b = SgsBatch()
        for k, v in fields.items():
            setattr(b, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
        with torch.cuda.device(self.dev):
            rc = self.eng.lib.gsm_sgs_iterate(self.eng.h, C.byref(b), n_iters, self.eng._stream())
        return rc, self.eng.lib.gsm_last_error(self.eng.h).decode()


@pytest.fixture(scope="module")
def worlds():
    made = {}

    def get(H, n_chains):
        if (H, n_chains) not in made:
            made[(H, n_chains)] = _World(H, n_chains)
        return made[(H, n_chains)]
    yield get
    for w in made.values():
        w.eng.close()


# ---- part 1: argument refusals ---------------------------------------------------------------------------------------------------
SEARCH = [(dict(hw=0), E_ARG, "search half-width"),
          (dict(num_points=7), E_UNSUPPORTED, "num_points must be in [8, 48]"),
          (dict(num_points=49), E_UNSUPPORTED, "num_points must be in [8, 48]"),
          (dict(radius=0.0), E_ARG, "radius must be > 0"),
          (dict(radius=-1.0), E_ARG, "radius must be > 0")]
LAG = [(dict(lag_mi=-1), E_ARG, "lag table extents must be >= 0"), (dict(lag_mj=-1), E_ARG, "lag table extents must be >= 0")]
MAXC = [(dict(max_cells=0), E_ARG, "max_cells must be in [1, 1024]"), (dict(max_cells=1025), E_ARG, "max_cells must be in [1, 1024]")]
BOUNDS_TEXT = "bounds (lower and upper) go with GSM_DRAW_TRUNCATED and only with it"
VTYPE_TEXT = "vtype must be GSM_VTYPE_EXPONENTIAL, GSM_VTYPE_GAUSSIAN or GSM_VTYPE_SPHERICAL"


class _Refusals:
    """The valid argument lists of the seven entry points on one world, outputs filled with the sentinel."""

    def __init__(self, w):
        t = w.torch
        n, HW_ = w.n, w.H * w.H
        self.w = w
        self.grids, self.grids2 = w.full(n * HW_, SENTINEL), w.full(n * HW_, SENTINEL)
        self.trace = w.full(3 * n * MAX_CELLS, SENTINEL)
        self.est, self.var, self.nn = w.full(4, SENTINEL), w.full(4, SENTINEL), w.full(4, SENTINEL_I, t.int32)
        self.loss, self.loss_prev = w.full(n, SENTINEL), w.full(n, SENTINEL)
        self.outputs = [(self.grids, SENTINEL), (self.grids2, SENTINEL), (self.trace, SENTINEL), (self.est, SENTINEL),
                        (self.var, SENTINEL), (self.nn, SENTINEL_I), (self.loss, SENTINEL), (self.loss_prev, SENTINEL)]
        zc = w.full(HW_, float("nan"))
        self.lo, self.hi = w.full(HW_, -1.0), w.full(HW_, 1.0)
        i32z = lambda k: w.zeros(k, t.int32)
        search = dict(hw=HW, radius=RADIUS, num_points=NPTS)
        blocks_head = dict(grids=self.grids, zcond=zc, windows=i32z(4 * n), x_axis=w.xs, y_axis=w.ys, lag_cov=w.lag, lag_mi=w.H - 1,
                           lag_mj=w.H - 1, **search, sill=1.0, cell_off=i32z(n + 1))
        cells, z = i32z(2 * n * MAX_CELLS), w.zeros(n * MAX_CELLS, t.float64)
        grid_head = dict(grids=self.grids, path=i32z(4 * n), path_off=w.zeros(n + 1, t.int64), max_path=4, draws=w.zeros(4 * n, t.float64),
                         lower=None, upper=None, draw_kind=0, x_axis=w.xs, y_axis=w.ys)
        krige_head = dict(grid=self.grids, cells=i32z(4), n_cells=4, x_axis=w.xs, y_axis=w.ys)
        krige_tail = dict(est=self.est, var=self.var, n_neighbours=self.nn)
        self.base = {
            "gsm_sgs_blocks": dict(**blocks_head, cells=cells, z=z, max_cells=MAX_CELLS, trace=self.trace, nbr_trace=None),
            "gsm_sgs_blocks_batch": dict(**blocks_head, cell_cnt=None, cells=cells, z=z, max_cells=MAX_CELLS),
            "gsm_sgs_iterate": dict(cur=self.grids, next=self.grids2, zcond=zc, x_axis=w.xs, y_axis=w.ys, lag_cov=w.lag, windows=i32z(4 * n),
                                    cell_off=i32z(n + 1), cells=cells, z=z, u=w.zeros(n, t.float64), resampled=i32z(n * HW_),
                                    loss=self.loss, bad=i32z(n), loss_prev=self.loss_prev, accept=w.zeros(n, t.uint8), radius=RADIUS,
                                    sill=1.0, cell_off_stride=n, lag_mi=w.H - 1, lag_mj=w.H - 1, hw=HW, num_points=NPTS,
                                    max_cells=MAX_CELLS),
            "gsm_sgs_grid": dict(**grid_head, lag_cov=w.lag, lag_mi=w.H - 1, lag_mj=w.H - 1, **search, sill=1.0, seg_cells=64,
                                 trace=self.trace),
            "gsm_sgs_grid_local": dict(**grid_head, local=w.local, vtype=0, **search, seg_cells=64, trace=self.trace),
            "gsm_krige_grid": dict(**krige_head, lag_cov=w.lag, lag_mi=w.H - 1, lag_mj=w.H - 1, **search, sill=1.0, **krige_tail),
            "gsm_krige_grid_local": dict(**krige_head, local=w.local, vtype=0, **search, **krige_tail),
        }

    def rows(self, entry):
        null = lambda *names: [({k: None}, E_ARG, "NULL pointer") for k in names]
        HW_ = self.w.H * self.w.H
        bounds = [(dict(lower=self.lo, upper=self.hi), E_ARG, BOUNDS_TEXT), (dict(draw_kind=1), E_ARG, BOUNDS_TEXT),
                  (dict(draw_kind=1, lower=self.lo), E_ARG, BOUNDS_TEXT)]
        path = [(dict(max_path=-1), E_ARG, "max_path must be in [0, H * W]"), (dict(max_path=HW_ + 1), E_ARG, "max_path must be in [0, H * W]"),
                (dict(seg_cells=0), E_ARG, "seg_cells must be >= 1")]
        n_cells = [(dict(n_cells=-1), E_ARG, "n_cells must be in [0, H * W]"), (dict(n_cells=HW_ + 1), E_ARG, "n_cells must be in [0, H * W]")]
        matern = [(dict(vtype=3), E_UNSUPPORTED, VTYPE_TEXT)]
        return {
            "gsm_sgs_blocks": null("grids", "lag_cov", "z") + SEARCH + LAG + MAXC,
            "gsm_sgs_blocks_batch": null("grids", "x_axis", "cell_off") + SEARCH + LAG + MAXC,
            "gsm_sgs_iterate": null("next", "y_axis", "lag_cov") + SEARCH + LAG + MAXC +
                               [(dict(cell_off_stride=self.w.n - 1), E_ARG, "cell_off_stride must be >= n_chains"),
                                (dict(tail_qt=3), E_ARG, "tail_qt must be GSM_TAIL_QT_AUTO, _ON or _OFF"),
                                (dict(tail_qt=-1), E_ARG, "tail_qt must be GSM_TAIL_QT_AUTO, _ON or _OFF")],
            "gsm_sgs_grid": null("grids", "draws", "lag_cov") + bounds + SEARCH + LAG + path,
            "gsm_sgs_grid_local": null("grids", "path_off", "local") + bounds + SEARCH + path + matern,
            "gsm_krige_grid": n_cells + null("grid", "lag_cov", "est") + SEARCH + LAG,
            "gsm_krige_grid_local": n_cells + null("cells", "local", "n_neighbours") + SEARCH + matern,
        }[entry]

    def check(self, entry, rows):
        w = self.w
        for change, code, text in rows:
            args = {**self.base[entry], **change}
            rc, msg = w.iterate(args) if entry == "gsm_sgs_iterate" else w.call(entry, args)
            label = f"{entry} with {sorted(change)}"
            assert rc == code, f"{label}: code {rc}, text {msg!r}"
            assert msg.startswith(entry + ": ") and text in msg, f"{label}: {msg!r}"
            for out, s in self.outputs:
                assert bool((out == s).all()), f"{label}: an output array was written"


ENTRIES = ["gsm_sgs_blocks", "gsm_sgs_blocks_batch", "gsm_sgs_iterate", "gsm_sgs_grid", "gsm_sgs_grid_local", "gsm_krige_grid",
           "gsm_krige_grid_local"]


@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_refusals(worlds, entry):
    r = _Refusals(worlds(8, 1 if "krige" in entry else 2))
    rows = r.rows(entry)
    assert len(rows) >= 9
    r.check(entry, rows)


@pytest.mark.parametrize("entry", ["gsm_krige_grid", "gsm_krige_grid_local"])
def test_krige_refuses_a_handle_of_several_chains(worlds, entry):
    r = _Refusals(worlds(8, 2))
    r.check(entry, [({}, E_ARG, "one grid per handle (create it with n_chains = 1)")])


def test_simple_kriging_without_means_is_refused(worlds):
    w = worlds(8, 1)
    rc = w.eng.lib.gsm_sgs_set_kriging(w.eng.h, 1, None)
    msg = w.eng.lib.gsm_last_error(w.eng.h).decode()
    assert rc == E_ARG and "gsm_sgs_set_kriging: simple kriging needs the global mean of every chain" in msg, (rc, msg)
    rc = w.eng.lib.gsm_sgs_set_kriging(w.eng.h, 2, None)
    msg = w.eng.lib.gsm_last_error(w.eng.h).decode()
    assert rc == E_ARG and "ktype must be GSM_KRIGING_ORDINARY or GSM_KRIGING_SIMPLE" in msg, (rc, msg)


# ---- part 2: device flags --------------------------------------------------------------------------------------------------------
WIN = (2, 6, 2, 6)


def _window_cells():
    r0, r1, c0, c1 = WIN
    cells = np.array([(i, j) for i in range(r0, r1) for j in range(c0, c1)], dtype=np.int32)
    np.random.default_rng(5).shuffle(cells)
    return cells


def _blocks(w, win, cells):
    """gsm_sgs_blocks of one chain: every listed cell of the window is simulated.  Returns (code, text, grid afterwards)."""
    grid = w.f64(w.field[None])
    z = np.random.default_rng(6).standard_normal(cells.shape[0])
    rc, msg = w.call("gsm_sgs_blocks", dict(
        grids=grid, zcond=w.full(w.H * w.H, float("nan")), windows=w.i32(win), x_axis=w.xs, y_axis=w.ys, lag_cov=w.lag, lag_mi=w.H - 1,
        lag_mj=w.H - 1, hw=HW, radius=RADIUS, num_points=NPTS, sill=1.0, cell_off=w.i32([0, cells.shape[0]]), cells=w.i32(cells),
        z=w.f64(z), max_cells=MAX_CELLS, trace=None, nbr_trace=None))
    return rc, msg, grid.cpu().numpy().reshape(w.H, w.H)


@pytest.mark.parametrize("H", [8, 12])
def test_window_outside_the_grid_and_cell_outside_its_window(worlds, H):
    w = worlds(H, 1)
    cells = _window_cells()
    rc, msg, good = _blocks(w, WIN, cells)
    assert rc == 0, msg
    assert np.isfinite(good).all() and not np.array_equal(good, w.field)
    strayed = cells.copy()
    strayed[3] = (0, 0)                                                   # inside the grid, outside the window
    for win, listed in (((0, H + 1, 0, 2), cells), (WIN, strayed)):       # flag 1, then flag 2
        rc, msg, _ = _blocks(w, win, listed)
        assert rc == E_DEVICE_DATA, (rc, msg)
        assert msg.startswith("gsm_sgs_blocks: window outside the grid / larger than 1024 cells, more cells than max_cells, or a listed "
                              "cell outside its window"), msg
        rc, msg, again = _blocks(w, WIN, cells)
        assert rc == 0, msg
        assert np.array_equal(again, good)


def _holes(w):
    """Four cells of the grid without a value, and the grid with NaN there."""
    cells = np.array([3 * w.H + 3, 3 * w.H + 4, 4 * w.H + 3, 1 * w.H + 6], dtype=np.int32)
    grid = w.field.copy()
    grid.ravel()[cells] = np.nan
    return cells, grid


def _krige(w, grid, cells):
    est, var, n = w.full(cells.size, SENTINEL), w.full(cells.size, SENTINEL), w.full(cells.size, SENTINEL_I, w.torch.int32)
    rc, msg = w.call("gsm_krige_grid", dict(grid=w.f64(grid), cells=w.i32(cells), n_cells=int(cells.size), x_axis=w.xs, y_axis=w.ys,
                                            lag_cov=w.lag, lag_mi=w.H - 1, lag_mj=w.H - 1, hw=HW, radius=RADIUS, num_points=NPTS, sill=1.0,
                                            est=est, var=var, n_neighbours=n))
    return rc, msg, (est.cpu().numpy(), var.cpu().numpy(), n.cpu().numpy())


@pytest.mark.parametrize("H", [8, 12])
def test_krige_grid_without_any_value(worlds, H):
    w = worlds(H, 1)
    cells, grid = _holes(w)
    rc, msg, good = _krige(w, grid, cells)
    assert rc == 0, msg
    assert np.isfinite(good[0]).all() and (good[2] >= 1).all()
    rc, msg, bad = _krige(w, np.full((H, H), np.nan), cells)
    assert rc == E_DEVICE_DATA, (rc, msg)
    assert msg.startswith("gsm_krige_grid: a cell to estimate has no value anywhere on the grid"), msg
    assert np.isnan(bad[0]).all() and np.isnan(bad[1]).all() and (bad[2] == 0).all()       # every cell raised the error
    rc, msg, again = _krige(w, grid, cells)
    assert rc == 0, msg
    assert all(np.array_equal(a, b) for a, b in zip(again, good))


def _sgs_grid(w, grid, path):
    grids = w.f64(grid[None])
    draws = np.random.default_rng(7).standard_normal(path.size)
    rc, msg = w.call("gsm_sgs_grid", dict(
        grids=grids, path=w.i32(path), path_off=w.torch.as_tensor(np.array([0, path.size], dtype=np.int64)).to(w.dev),
        max_path=int(path.size), draws=w.f64(draws), lower=None, upper=None, draw_kind=0, x_axis=w.xs, y_axis=w.ys, lag_cov=w.lag,
        lag_mi=w.H - 1, lag_mj=w.H - 1, hw=HW, radius=RADIUS, num_points=NPTS, sill=1.0, seg_cells=64, trace=None))
    return rc, msg, grids.cpu().numpy().reshape(w.H, w.H)


@pytest.mark.parametrize("H", [8, 12])
def test_sgs_grid_without_any_value(worlds, H):
    w = worlds(H, 1)
    path, grid = _holes(w)
    rc, msg, good = _sgs_grid(w, grid, path)
    assert rc == 0, msg
    assert np.isfinite(good).all()
    rc, msg, bad = _sgs_grid(w, np.full((H, H), np.nan), path)
    assert rc == E_DEVICE_DATA, (rc, msg)
    assert msg.startswith("gsm_sgs_grid: a cell to simulate has no value anywhere on the grid"), msg
    assert np.isnan(bad.ravel()[path[0]])                                 # the first path cell had nothing to condition on
    rc, msg, again = _sgs_grid(w, grid, path)
    assert rc == 0, msg
    assert np.array_equal(again, good)


def _draw_philox(w, region):
    t, n_iters = w.torch, 3
    k = n_iters * w.n
    out = dict(windows=w.zeros(4 * k, t.int32), blocks=w.zeros(4 * k, t.int32), cell_off=w.zeros(k, t.int32), cell_cnt=w.zeros(k, t.int32),
               cells=w.zeros(2 * k * MAX_CELLS, t.int32), z=w.zeros(k * MAX_CELLS, t.float64), u=w.zeros(k, t.float64))
    seeds = t.as_tensor(np.arange(1, w.n + 1, dtype=np.int64)).to(w.dev)
    mask = t.as_tensor(np.full(w.H * w.H, region, dtype=np.uint8)).to(w.dev)
    rc, msg = w.call("gsm_sgs_draw_philox", dict(seeds=seeds, iter0=0, n_iters=n_iters, region_mask=mask, is_data=w.zeros(w.H * w.H, t.uint8),
                                                 min_x=2, max_x=4, min_y=2, max_y=4, max_cells=MAX_CELLS, **out))
    assert rc == 0, msg                                                   # asynchronous: gsm_sgs_check reports
    rc, msg = w.call("gsm_sgs_check", {})
    return rc, msg, {k_: v.cpu().numpy() for k_, v in out.items()}


@pytest.mark.parametrize("H", [8, 12])
def test_no_block_centre_inside_the_region_mask(worlds, H):
    w = worlds(H, 1)
    rc, msg, good = _draw_philox(w, 1)
    assert rc == 0, msg
    assert (good["cell_cnt"] >= 1).all()
    rc, msg, _ = _draw_philox(w, 0)
    assert rc == E_DEVICE_DATA, (rc, msg)
    assert msg.startswith("gsm_sgs_check: no block centre inside the region mask after 64 attempts"), msg
    rc, msg, again = _draw_philox(w, 1)
    assert rc == 0, msg
    assert all(np.array_equal(again[k], good[k]) for k in good)
