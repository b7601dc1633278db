"""Shared by tests/test_qt_fit_host.py and tests/test_gpu_qt_fit.py: the cases of the device fit of scikit-learn's QuantileTransformer
(gsm_qt_fit, sgs.fit_normal_scores) and the NumPy restatement of what it computes.  Every check on these cases is an equality.

A case is a number of cells; its fields and the table lengths follow from it:
  sizes      every n in 1 .. 40; powers of two from 256 to 16384 and their two neighbours (every power-of-two tile boundary, odd tile
             counts, ragged last tiles; the sort's tile is 4096 keys); 3 * 4096, 5 * 4096 + 7, 65536, 100 * 130
  contents   cycled over the sizes (CONTENTS): normal deviates at scales 1e-3 .. 1e6 with offsets, values rounded to integers and
             to one decimal (ties), already sorted, reverse sorted, all equal, both signs of zero with subnormals mixed in, NaN in 5 %
             and in 20 % of the cells
  batch      fields(cells): one field without NaN, one with some NaN, one all NaN and, for cells >= 2, one with a single finite value
  nq         those of 2, 3, 150 and 1000 that are at most `cells` (cells == 1: 2, the shortest table there is)."""
import functools
import warnings

import numpy as np

TILE = 4096
SIZES = (list(range(1, 41)) + [p + d for p in (256, 1024, 2048, 4096, 8192, 16384) for d in (-1, 0, 1)]
         + [3 * TILE, 5 * TILE + 7, 65536, 100 * 130])
CONTENTS = ("normal_1e-3", "integers", "normal_1", "one_decimal", "sorted", "normal_1e3", "reversed", "all_equal", "zeros_subnormals",
            "normal_1e6", "nan_5", "nan_20")


def case_id(cells):
    return f"{cells}-{CONTENTS[SIZES.index(cells) % len(CONTENTS)]}"


def nqs(cells):
    return [k for k in (2, 3, 150, 1000) if k <= cells] or [2]


def _content(kind, cells, rng):
    z = rng.standard_normal(cells)
    if kind.startswith("normal_"):
        scale = float(kind.split("_")[1])
        return scale * z + 37.0 * scale * (1 if cells % 2 else -1)
    if kind == "integers":
        return np.round(4.0 * z)
    if kind == "one_decimal":
        return np.round(30.0 * z, 1)
    if kind == "sorted":
        return np.sort(250.0 * z - 1000.0)
    if kind == "reversed":
        return np.sort(250.0 * z + 1000.0)[::-1].copy()
    if kind == "all_equal":
        return np.full(cells, -412.625)
    if kind == "zeros_subnormals":
        pool = np.array([0.0, -0.0, 5e-324, -5e-324, 2.5e-310, -2.5e-310, 2.2250738585072014e-308, -2.2250738585072014e-308, 1.0, -1.0])
        return pool[rng.integers(0, pool.size, cells)]
    if kind in ("nan_5", "nan_20"):
        return 80.0 * z - 300.0
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def fields(cells):
    """The batch of a case, [3 or 4, cells] float64 (read-only): no NaN | some NaN | all NaN | (cells >= 2) a single finite value"""
    kind = CONTENTS[SIZES.index(cells) % len(CONTENTS)]
    rng = np.random.default_rng(1000 + cells)
    clean = _content(kind, cells, rng)
    some = _content(kind, cells, rng)
    frac = 0.2 if kind == "nan_20" else 0.05
    k = min(max(1, int(round(frac * cells))), cells - 1)            # at least one NaN and one value; cells == 1 leaves no room: no NaN
    some[rng.choice(cells, size=k, replace=False)] = np.nan
    rows = [clean, some, np.full(cells, np.nan)]
    if cells >= 2:
        one = np.full(cells, np.nan)
        one[int(rng.integers(0, cells))] = clean[0]
        rows.append(one)
    out = np.ascontiguousarray(np.stack(rows))
    out.setflags(write=False)
    return out


def probabilities(nq):
    """q as scikit-learn and NumPy make it: references_ * 100 (to percent), / 100 (back)"""
    return (np.linspace(0, 1, nq, endpoint=True) * 100) / 100


def restate(x, nq):
    """quantiles_[:, 0] of QuantileTransformer(n_quantiles=nq, subsample=None).fit(x.reshape(-1, 1)) in plain NumPy on the sorted values
    that are not NaN: np.nanpercentile(method='linear') with NumPy's _lerp, every operation rounded on its own, then
    np.maximum.accumulate.  No value: a row of NaN."""
    x = np.asarray(x, dtype=np.float64).ravel()
    s = np.sort(x[~np.isnan(x)])
    m = s.size
    if m == 0:
        return np.full(nq, np.nan)
    v = (m - 1) * probabilities(nq)
    fl = np.floor(v)
    g = v - fl
    lo = fl.astype(np.int64)
    hi = np.minimum(lo + 1, m - 1)
    a, b = s[lo], s[hi]
    with np.errstate(invalid="ignore"):                    # infinities: inf - inf, inf * 0, as NumPy has them
        d = b - a
        t = np.where(g >= 0.5, b - d * (1 - g), a + d * g)
    return np.maximum.accumulate(t)


def sklearn_fit(x, nq, random_state=None):
    from sklearn.preprocessing import QuantileTransformer
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                    # all-NaN slices, n_quantiles above n_samples
        return QuantileTransformer(n_quantiles=nq, output_distribution="normal", subsample=None,
                                   random_state=random_state).fit(np.asarray(x, dtype=np.float64).reshape(-1, 1))


@functools.lru_cache(maxsize=None)
def reference(cells, nq):
    """Per field of the case: (restate's table, scikit-learn's quantiles_[:, 0] or None where the field has fewer than nq values)"""
    out = []
    for f in fields(cells):
        sk = sklearn_fit(f, nq).quantiles_[:, 0] if np.count_nonzero(~np.isnan(f)) >= nq else None
        out.append((restate(f, nq), sk))
    return out


def assembled(quantiles, nq, random_state=None):
    """A transformer built from a table, the way sgs.fit_normal_scores(device=True) builds it"""
    from sklearn.preprocessing import QuantileTransformer
    t = QuantileTransformer(n_quantiles=nq, output_distribution="normal", subsample=None, random_state=random_state)
    t.n_quantiles_, t.references_, t.n_features_in_ = nq, np.linspace(0, 1, nq, endpoint=True), 1
    t.quantiles_ = np.ascontiguousarray(np.asarray(quantiles, dtype=np.float64).reshape(nq, 1))
    return t
