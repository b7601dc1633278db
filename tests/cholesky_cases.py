"""Case data of tests/test_gpu_cholesky_tiles.py: a block table aimed at the tile geometry of the precomputed-factor
("L z") proposal generator (cholesky_kernel.hip), the launch sequence that runs on it, and the record-by-record comparison
with cholesky_oracle.proposal.  Plain module: no GPU is touched on import, and the oracle side is computed once per
launch and shared.

The generator multiplies Z^T [records of a group, padded to 64] by U [Npad x Npad, Npad = N rounded up to 64] in output
tiles of 64 records x 128 cells whose right half is dropped when Npad ends inside it.  What decides the code path is
therefore N mod 128 (<= 64 or not), the number of 128-wide cell tiles, and the number of records of a group relative
to 64."""
import numpy as np

import cholesky_oracle as co
import mcmc_oracle as orc

JITTER = 1e-8
EPS = 2.2e-16

# (bh, bw) -> N = bh * bw, in table order
TILE_TABLE = [
    (2, 2),      # N = 4:   Npad 64, almost all padding
    (8, 8),      # N = 64:  exactly one half tile, no right half at n0 = 0
    (10, 10),    # N = 100: right half exists, padded
    (8, 16),     # N = 128: one full tile
    (10, 14),    # N = 140: Npad 192, second tile left half only, padded
    (12, 16),    # N = 192: the same, unpadded
    (14, 14),    # N = 196: Npad 256
    (16, 16),    # N = 256: two full tiles
    (16, 24),    # N = 384: three tiles
    (18, 22),    # N = 396: Npad 448, fourth tile left half only
    (20, 26),    # N = 520: Npad 576, five tiles
]
SEEDS = [7, 2 ** 40 + 12345, 99, 1234567, 5, 6, 8, 9, 10, 11, 12]

# the launches, in the order they run on ONE engine (a later one meets the earlier one's scratch)
LAUNCHES = [
    dict(name="big", n_steps=192, step0=500, n_classes=1),        # 2112 records: 3-4 record tiles per group, partial last tile
    dict(name="tiny", n_steps=1, step0=6, n_classes=1),           # 11 records on the big launch's scratch: five empty groups (the first among them), one of one
    dict(name="at64", n_steps=64, step0=1000, n_classes=1),       # 704 records: groups of 63, 64 and 65+ records
    dict(name="classes3", n_steps=64, step0=0, n_classes=3),      # 33 groups: the scratch set is rebuilt
]


def rf_params():
    """The Exponential parameters of test_cholesky_proposals_match_oracle."""
    return orc.RFParams(10e3, 50e3, 12e3, 40e3, 50, 150, 0.0, "Exponential", True, None)


def tile_pairs():
    """RandField.pairs layout: row 0 widths, row 1 heights."""
    return np.array([[bw for _, bw in TILE_TABLE], [bh for bh, _ in TILE_TABLE]])


def tile_masks():
    """One array per size of uniform values in [0.25, 1]: no symmetry, so mask[n] is checked cell by cell and a transposed
    or shifted index shows."""
    g = np.random.default_rng(20240611)
    return [g.uniform(0.25, 1.0, size=(bh, bw)) for bh, bw in TILE_TABLE]


class OracleLaunch:
    """cholesky_oracle.proposal of every record of a launch, stacked."""

    def __init__(self, launch, rfp, pairs, masks, centres, W, resolution, varios, cache):
        n_chains, n_steps = len(SEEDS), launch["n_steps"]
        self.n_classes = len(varios)
        self.rec = [[co.proposal(SEEDS[c], launch["step0"] + s, rfp, pairs, masks, centres, W, resolution, varios, JITTER, cache)
                     for s in range(n_steps)] for c in range(n_chains)]
        flat = [e for row in self.rec for e in row]
        shp = (n_chains, n_steps)
        self.size_idx = np.array([e["size_idx"] for e in flat]).reshape(shp)
        self.range_class = np.array([e["range_class"] for e in flat]).reshape(shp)
        self.centre = np.array([e["centre"] for e in flat]).reshape(shp + (2,))
        self.u = np.array([e["u"] for e in flat]).reshape(shp)
        self.scale = np.array([e["scale"] for e in flat]).reshape(shp)
        self.group = self.size_idx * self.n_classes + self.range_class
        self.counts = np.bincount(self.group.ravel(), minlength=pairs.shape[1] * self.n_classes)


def compare_launch(out, ora, factors_host, masks, oracle_allow):
    """Every record of a launch (none skipped) against the oracle.  out: propose_philox's dict as host arrays; factors_host[g]:
    the device factor U of group g on the host; oracle_allow: the allowance, in units of a record's scale, of the comparison
    with the oracle's own factor.  Returns (largest |f - U^T z scale mask| / scale, largest |f - oracle field| / scale)."""
    assert np.array_equal(out["size_idx"], ora.size_idx)
    assert np.array_equal(out["centre"], ora.centre)
    assert np.array_equal(out["u"], ora.u)
    assert np.array_equal(out["rf_scalars"][..., 0], ora.scale)
    assert np.array_equal(out["rf_scalars"][..., 2], ora.range_class.astype(np.float64))
    fields = out["fields"]
    n_records = 0
    worst_exact = worst_oracle = 0.0
    for g in np.flatnonzero(ora.counts):
        cs, ss = np.nonzero(ora.group == g)
        si = int(g) // ora.n_classes
        bh, bw = TILE_TABLE[si]
        N = bh * bw
        f = fields[cs, ss]                                              # [records of the group, field_stride]
        scale = ora.scale[cs, ss][:, None]
        Z = np.stack([ora.rec[c][s]["z"] for c, s in zip(cs, ss)], axis=1)      # [N, records]
        U = factors_host[g][:N, :N]
        exact = ((U.T @ Z).T * scale) * masks[si].ravel()[None, :]
        e_exact = np.abs(f[:, :N] - exact) / scale
        bad = np.argwhere(e_exact > 1e-12)
        assert bad.size == 0, (f"group {g} (N = {N}, {len(cs)} records): {len(bad)} cells differ from U^T z * scale * mask, first at "
                               f"(chain {cs[bad[0][0]]}, step {ss[bad[0][0]]}, cell {bad[0][1]}), largest error {e_exact.max():.3e} of the scale")
        want = np.stack([ora.rec[c][s]["field"].ravel() for c, s in zip(cs, ss)])
        e_oracle = np.abs(f[:, :N] - want) / scale
        assert e_oracle.max() <= oracle_allow, (f"group {g} (N = {N}): {e_oracle.max():.3e} of the scale from the oracle's field, "
                                                f"allowed {oracle_allow:.3e}")
        # the buffer was zero-filled: a tile that writes past N, or into another record, shows here
        assert not f[:, N:].any(), f"group {g} (N = {N}): cells written past the block"
        assert np.abs(exact).max() > 0.2 * scale.min()                  # the comparison is not of zeros
        worst_exact, worst_oracle = max(worst_exact, e_exact.max()), max(worst_oracle, e_oracle.max())
        n_records += len(cs)
    assert n_records == ora.size_idx.size                               # the share left out is zero
    return worst_exact, worst_oracle


def unblocked_cholesky_first_failure(S, jitter=0.0):
    """Plain unblocked Cholesky loop on S + jitter I: 0 when it is positive definite, else the 1-based index of the first pivot
    that is not positive (a NaN pivot is not positive)."""
    A = np.array(S, dtype=np.float64)
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        piv = A[j, j] + jitter - np.dot(L[j, :j], L[j, :j])
        if not piv > 0.0:
            return j + 1
        L[j, j] = np.sqrt(piv)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return 0


def spd(n, seed):
    g = np.random.default_rng(seed)
    M = g.normal(size=(n, n))
    return M @ M.T + n * np.eye(n)


def fail_at(S, pivot):
    """S with its diagonal entry changed so that the factorisation first fails at 1-based `pivot` (the pivot there becomes -1)."""
    L = np.linalg.cholesky(S)
    j = pivot - 1
    B = S.copy()
    B[j, j] = np.dot(L[j, :j], L[j, :j]) - 1.0
    return B
