"""Cases of the 'pcg64' mode of interpolate.sgs (gsm_sgs_grid_draw_pcg64): the device's shuffle, path and draws against
interpolate._Plan.draws, which is NumPy.  tests/test_gpu_interp_sgs_pcg64.py runs them on the device,
tests/test_interp_sgs_pcg64_host.py shows with NumPy alone that they reach what they are here for: the ziggurat's tail, a
generator that enters with a cached 32-bit word, a shuffle that leaves one behind.

A case is (n_cells, values, kind, R, pending) on a 260 x 260 grid whose sim_mask is the first n_cells cells in C order:
    n_cells  the mask edges of random_interval at 2^k - 1 / 2^k, the 64-lane windows of the compaction and of the uniforms, the
             1024 cells the block kernel (sgs_draw_pcg64_kernel) stops at, and sizes far beyond it
    values   which cells of sim_mask hold a value: 'none', 'all' (an empty path) or 'some' (a random 30 %)
    kind     'normal' (no bounds) or 'truncated' (bounds with lower == upper cells and NaN bounds)
    R        realisations, generator r seeded with SEED0 + r
    pending  generator min(1, R - 1) has made one rng.integers(0, 10) before the call: it enters with has_uint32 == 1
The cells behind the mask always hold values (a plan needs conditioning data)."""
import functools
import warnings

import numpy as np

import interp_sgs_common as ic

H = W = 260
N_CELLS = (0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 1024, 1025, 4097, 65535, 65536, 65537)
SEED0 = 4100
VARIO = dict(major_range=6000.0, minor_range=6000.0, azimuth=0.0, sill=1.0, nugget=0.0, vtype="Exponential")
ZIGGURAT_NOR_R = 3.6541528853610088          # numpy/random/src/distributions/ziggurat_constants.h: beyond it only the tail path draws


def cases():
    """id -> (n_cells, values, kind, R, pending)."""
    out = {}
    for n in N_CELLS:
        few = 3 if n <= 4097 else 1                        # a host shuffle of 65 536 rows takes 0.1 s: one realisation there
        out[f"{n}-none-normal"] = (n, "none", "normal", few, True)
        out[f"{n}-some-truncated"] = (n, "some", "truncated", few, n % 2 == 1)
        out[f"{n}-all-normal"] = (n, "all", "normal", 1, n % 2 == 0)
        if n <= 1025:
            out[f"{n}-some-normal-70"] = (n, "some", "normal", 70, True)
    out["129-none-truncated-70"] = (129, "none", "truncated", 70, True)
    return out


MANY_NORMALS = "65537-none-normal"           # R * path_len >= 50 000 normals: wedges (0.7 % of the draws) and tails (1 in 3 700) occur
CACHED_AFTER_SHUFFLE = "127-none-normal"     # its first generator leaves the shuffle with has_uint32 == 1 (asserted by the host test)


@functools.lru_cache(maxsize=None)
def plan(n_cells, values, kind):
    """The _Plan of a case (shared by the cases that differ in R and pending only; nothing modifies it)."""
    from mcmc_gpu_amd import interpolate
    xx, yy = np.meshgrid(np.arange(W) * 500.0, np.arange(H) * 500.0)
    flat = np.arange(H * W).reshape(H, W)
    sim_mask = flat < n_cells
    r = np.random.default_rng(97)
    holds = ~sim_mask                                      # the cells behind the mask: always values
    if values == "all":
        holds = np.full((H, W), True)
    elif values == "some":
        holds = holds | (sim_mask & (r.random((H, W)) < 0.3))
    grid = np.where(holds, ic.field(H, W, 41), np.nan)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        p = interpolate._Plan(xx, yy, grid, VARIO, 3000.0, 16, "ok", sim_mask, None, None, None)
    if kind == "truncated":
        # bounds in normal-score space, as _Plan keeps them: a fifth of the cells with lower == upper (no draw), NaN in either
        # bound (NaN != x: a draw), the rest an interval
        lo = r.normal(0.0, 1.0, (H, W))
        hi = lo + 1.0
        what = r.random((H, W))
        hi[what < 0.2] = lo[what < 0.2]
        lo[(what >= 0.2) & (what < 0.25)] = np.nan
        hi[(what >= 0.25) & (what < 0.3)] = np.nan
        p.bounds = (np.ascontiguousarray(lo), np.ascontiguousarray(hi))
    return p


def generators(R, pending):
    """The generators a case starts from (fresh objects on every call: run one set on the device, its twin through NumPy)."""
    gens = [np.random.default_rng(SEED0 + r) for r in range(R)]
    if pending:
        gens[min(1, R - 1)].integers(0, 10)
    return gens


def small_30():
    """A 30 x 30 whole-grid problem (sim_mask None, bounds on) for the end-to-end check of the generator's cached word: with seed
    SEED_30 the shuffle of its 900 cells leaves has_uint32 == 1."""
    n = 30
    xx, yy = np.meshgrid(np.arange(n) * 500.0, np.arange(n) * ic.TIE_FREE_DY)
    cond = np.zeros((n, n), bool)
    cond[::5, :] = True
    cond[:, ::6] = True
    bed = ic.field(n, n, 43)
    grid = np.where(cond, bed, np.nan)
    kw = dict(radius=3000.0, num_points=16, ktype="ok", bounds=(float(np.nanmin(grid)) - 50.0, bed + 300.0))
    return xx, yy, grid, VARIO, kw


SEED_30 = 7
