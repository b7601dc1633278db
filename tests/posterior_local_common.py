"""NumPy restatement of the posterior cross sums of every cell with its neighbours (mcmc_gpu_amd/posterior.py's docstring, `local`),
the cases of the device tests and the bound they assert.  Shares nothing with the package.

Definitions.  Reach R in 1 .. 4; the K = 2 R^2 + 2 R offsets (di, dj) of the upper half plane in this order: (0, 1) .. (0, R), then for
di = 1 .. R: (di, -R) .. (di, R).  x [n, H, W] the n beds that enter (chains x snapshots that belong to a sequence x calls), g [H, W]
the common field, d = x - g.  X[k, i, j] = sum over the n beds of d[i, j] d[i + di_k, j + dj_k] where the partner (i + di_k, j + dj_k)
lies inside the grid; every other entry is exactly 0.  A NaN bed at a cell makes NaN exactly the entries that pair that cell: its own
K entries and entry k of the cell at minus offset k, where the partner of that entry is inside the grid.

Bound (derived, not tuned), u = 2^-53, reference in np.longdouble on the bits the device sees (f32 data cast to f64).  The device
rounds each difference once (two factors of 1 + delta per product), and every fused step rounds once: a term passes through at
most the steps of its own part of the chain axis, the additions of the part merge and the addition onto the caller's array, which
together never exceed n + 1 for n terms cut into parts; one further unit covers the second-order terms:
    |X^ - X| <= (n + 4) u sum |d| |d'|."""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble


def offsets(R):
    """[(di, dj)] in the order of the planes."""
    return [(0, dj) for dj in range(1, R + 1)] + [(di, dj) for di in range(1, R + 1) for dj in range(-R, R + 1)]


def pair_slices(H, W, di, dj):
    """(cells, partners): slices of the cells whose partner at (di, dj) lies inside the grid, and of those partners; None when
    there are none."""
    i0, i1, j0, j1 = max(0, -di), min(H, H - di), max(0, -dj), min(W, W - dj)
    if i0 >= i1 or j0 >= j1:
        return None
    return (slice(i0, i1), slice(j0, j1)), (slice(i0 + di, i1 + di), slice(j0 + dj, j1 + dj))


def inside(H, W, R):
    """[K, H, W] bool: the entries whose partner lies inside the grid."""
    m = np.zeros((2 * R * R + 2 * R, H, W), dtype=bool)
    for k, (di, dj) in enumerate(offsets(R)):
        sl = pair_slices(H, W, di, dj)
        if sl is not None:
            m[k][sl[0]] = True
    return m


def reference(x, g, R):
    """(X [K, H, W], sum |d| |d'| [K, H, W]) in np.longdouble over the beds x [n, H, W]; 0 where the partner is outside the grid."""
    x = np.asarray(x, dtype=np.float64)
    n, H, W = x.shape
    d = x.astype(LD) - np.asarray(g, dtype=np.float64).astype(LD)
    a = np.abs(d)
    K = 2 * R * R + 2 * R
    X, mag = np.zeros((K, H, W), dtype=LD), np.zeros((K, H, W), dtype=LD)
    with np.errstate(invalid="ignore"):
        for k, (di, dj) in enumerate(offsets(R)):
            sl = pair_slices(H, W, di, dj)
            if sl is None:
                continue
            (ci, cj), (pi, pj) = sl
            X[k][ci, cj] = (d[:, ci, cj] * d[:, pi, pj]).sum(axis=0)
            mag[k][ci, cj] = (a[:, ci, cj] * a[:, pi, pj]).sum(axis=0)
    return X, mag


def plain_float64(x, g, R):
    """X [K, H, W] by a plain float64 accumulation in the order of x's first axis: rounded differences, rounded products, rounded
    additions, nothing fused.  What a careful NumPy user would write; the fairness check of the bound."""
    x = np.asarray(x, dtype=np.float64)
    n, H, W = x.shape
    d = x - np.asarray(g, dtype=np.float64)
    X = np.zeros((2 * R * R + 2 * R, H, W))
    with np.errstate(invalid="ignore"):
        for k, (di, dj) in enumerate(offsets(R)):
            sl = pair_slices(H, W, di, dj)
            if sl is None:
                continue
            (ci, cj), (pi, pj) = sl
            for c in range(n):
                X[k][ci, cj] += d[c, ci, cj] * d[c, pi, pj]
    return X


def nan_entries(H, W, R, cells):
    """[K, H, W] bool: the entries a NaN bed at the cells [(i, j), ...] makes NaN."""
    m = np.zeros((2 * R * R + 2 * R, H, W), dtype=bool)
    for (i, j) in cells:
        for k, (di, dj) in enumerate(offsets(R)):
            if 0 <= i + di < H and 0 <= j + dj < W:
                m[k, i, j] = True                                    # the cell's own entry: its partner is inside
            if 0 <= i - di < H and 0 <= j - dj < W:
                m[k, i - di, j - dj] = True                          # the entry of the cell whose partner it is
    return m


def check(got, x, g, R, label="", n_terms=None, scale=1):
    """Assert got [K, H, W] float64 against scale * reference(x, g, R): entries whose partner is outside the grid exactly 0, NaN
    sets equal, every other entry within (n + 4) u sum |d| |d'| with n = n_terms (default: scale * len(x)).  Prints and returns the
    largest error as a share of the bound."""
    x = np.asarray(x, dtype=np.float64)
    n, H, W = x.shape
    n_t = scale * n if n_terms is None else n_terms
    got = np.asarray(got, dtype=np.float64)
    K = 2 * R * R + 2 * R
    assert got.shape == (K, H, W), (got.shape, (K, H, W))
    X, mag = reference(x, g, R)
    X, mag = scale * X, scale * mag
    ins = inside(H, W, R)
    assert (got[~ins] == 0).all(), f"{label}: {int((got[~ins] != 0).sum())} entries whose partner is outside the grid are not 0"
    assert np.array_equal(np.isnan(got), np.isnan(X)), f"{label}: NaN entries differ ({np.isnan(got).sum()} vs {np.isnan(X).sum()})"
    ok = ins & ~np.isnan(X)
    err = np.abs(got[ok].astype(LD) - X[ok])
    bound = (n_t + 4) * U * mag[ok]
    pos = bound > 0
    share = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    print(f"local cross {label}: n={n_t}, largest error {share:.3e} of the bound (n + 4) u sum |d||d'|")
    assert (err <= bound).all(), f"{label}: {int((err > bound).sum())} entries beyond (n + 4) u sum |d||d'|, worst {share:.3e} of it"
    return share


def beds(H, W, Cn, seed, f32):
    """(x [Cn, H, W], g [H, W]): x = -300 + 100 N(0, 1) plus a part common to a chain's cells (so that neighbours co-vary), rounded
    to float with f32 so that both state types see the values the reference sees; g = -300 + 10 N(0, 1)."""
    rng = np.random.default_rng(seed)
    x = -300.0 + 100.0 * rng.normal(size=(Cn, H, W)) + 60.0 * rng.normal(size=(Cn, 1, 1))
    g = -300.0 + 10.0 * rng.normal(size=(H, W))
    if f32:
        x = x.astype(np.float32).astype(np.float64)
    return x, g


# (H, W, reach, chains, state): the grids with few chains -- one chain per part where the rule of parts allows as many parts as
# chains.  (3, 9) at reach 4: the offsets with di >= 3 never pair.  (9, 257): 2 x 5 tiles, every reach.
FEW = [
    (3, 9, 4, 3, "f64"), (3, 9, 4, 4, "f32"),
    (5, 7, 1, 5, "f32"), (5, 7, 3, 4, "f64"),
    (70, 3, 2, 8, "f64"), (70, 3, 4, 4, "f32"),
    (9, 257, 1, 8, "f32"), (9, 257, 2, 7, "f64"), (9, 257, 3, 6, "f32"), (9, 257, 4, 4, "f64"),
    (33, 130, 2, 6, "f32"), (33, 130, 4, 3, "f64"),
    (64, 64, 1, 8, "f64"), (64, 64, 3, 5, "f32"),
]

# (H, W, reach, chains, state) -> what the pass must reach on a device of 256 compute units: (parts, cpp, last, empty)
MANY = {
    (33, 130, 1, 101, "f64"): (40, 3, 2, 6),          # ragged last part and empty parts
    (9, 257, 1, 390, "f32"): (40, 10, 10, 1),         # ten chains per part, staged four at a time: a short last group; an empty part
    (9, 257, 3, 101, "f32"): (6, 17, 16, 0),          # an odd count per part, staged two at a time; a ragged last part
    (33, 130, 4, 390, "f64"): (4, 98, 96, 0),         # many chains per part at the largest reach
}

# (H, W, reach, chains, state, NaN cells of the last chain): an interior cell and a corner
WITH_NAN = [
    (33, 130, 2, 5, "f64", [(17, 70), (0, 0)]),
    (9, 257, 4, 4, "f32", [(4, 128), (8, 256)]),
    (5, 7, 3, 4, "f64", [(2, 3), (4, 0)]),
]


def case_seed(H, W, R, Cn):
    return ((H * 1000 + W) * 10 + R) * 1000 + Cn


def split_plan(H, W, R, n_chains, n_cu):
    """How gsm_posterior_local cuts the chain axis, restated from include/gsm.h (nothing of the library is called): tiles of 8 x 64
    cells; parts = min(ceil(4 n_cu / tiles), n_chains, 160 // K, what keeps parts K H W doubles within 1 GiB), cpp = ceil(n_chains /
    parts) chains to a part; `last` is the chain count of the last part that holds a chain and `empty` the parts after it."""
    K = 2 * R * R + 2 * R
    tiles = -(-H // 8) * -(-W // 64)
    fill = max(1, min(-(-4 * n_cu // tiles), n_chains))
    parts = max(1, min(fill, 160 // K, (1 << 27) // (K * H * W)))
    cpp = -(-n_chains // parts)
    filled = -(-n_chains // cpp)
    return dict(parts=parts, cpp=cpp, last=n_chains - (filled - 1) * cpp, empty=parts - filled)


def all_cases():
    """Every (H, W, R, chains, state, NaN cells) the device tests feed, for the fairness check on the host."""
    return [c + ([],) for c in FEW] + [k + ([],) for k in MANY] + list(WITH_NAN)


def case_beds(H, W, R, Cn, state, nan_cells):
    x, g = beds(H, W, Cn, case_seed(H, W, R, Cn), state == "f32")
    for (i, j) in nan_cells:
        x[Cn - 1, i, j] = np.nan
    return x, g
