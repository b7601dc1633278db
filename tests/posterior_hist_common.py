"""NumPy restatement of the posterior histogram (include/gsm.h, gsm_posterior_histogram; mcmc_gpu_amd/posterior.py's `hist`) and of
the rule by which its kernel divides the chains.  Shares nothing with the package.

Slot rule.  For a value x of a cell with common field g: d = x - g, kf = floor(d * inv_w) + B / 2 in float64, inv_w = B / (2
half_width); NaN -> slot B + 2, kf < 0 -> slot 0, kf >= B -> slot B + 1, otherwise slot int(kf) + 1.  Slot B + 3 + l counts x <
levels[l].  A difference, a product, a floor and a sum of an integer: each is one correctly rounded IEEE operation, so the slot
computed here and on the device are the same number and the expected counts are exact.

Quantiles.  NumPy's method='inverted_cdf' returns the order statistic of rank ceil(q n).  The histogram's cumulative count reaches
that rank in the bin that holds this order statistic, and PosteriorSummary.quantile returns a point of that bin's closure, so the
two differ by less than one bin width w = 2 half_width / B wherever the bin is one of the B inner ones."""
import numpy as np

HIST_BLOCK = 256        # cells per workgroup, one per lane
HIST_CHAINS = 8         # chains whose loads are in flight together
HIST_MAX_CPP = 65535    # chains per part that a 16-bit LDS counter holds


def used_values(x, split):
    """x [C, T, H, W] -> the [M * N, H, W] values that belong to a sequence (split: the last 2 (T // 2) snapshots of every chain)."""
    x = np.asarray(x, dtype=np.float64)
    T = x.shape[1]
    lo = T - 2 * (T // 2) if split else 0
    return x[:, lo:].reshape((-1,) + x.shape[2:])


def slots(values, g, B, half_width):
    """Slot of every value [..., H, W] about g [H, W]."""
    inv_w = B / (2 * half_width)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.asarray(values, dtype=np.float64) - g
        kf = np.floor(d * inv_w) + B // 2
        s = np.where(np.isnan(kf), B + 2, np.where(kf < 0, 0, np.where(kf >= B, B + 1, 0)))
        inner = ~np.isnan(kf) & (kf >= 0) & (kf < B)
        s[inner] = kf[inner].astype(np.int64) + 1
    return s.astype(np.int64)


def hist_counts(values, g, B, half_width, levels=()):
    """[(B + 3 + L), H, W] int64 counts of values [n, H, W]."""
    values = np.asarray(values, dtype=np.float64)
    H, W = g.shape
    s = slots(values, g, B, half_width)
    flat = (s * (H * W) + np.arange(H * W).reshape(H, W)).ravel()
    out = [np.bincount(flat, minlength=(B + 3) * H * W).reshape(B + 3, H, W).astype(np.int64)]
    with np.errstate(invalid="ignore"):
        for lv in levels:
            out.append((values < float(lv)).sum(axis=0, dtype=np.int64)[None])
    return np.concatenate(out, axis=0)


def numpy_quantile(values, q):
    """The order statistic of rank ceil(q n) per cell (NaN where the cell holds a NaN)."""
    with np.errstate(invalid="ignore"):
        return np.quantile(values, q, axis=0, method="inverted_cdf")


def hist_plan(H, W, n_chains, n_cu):
    """How post_hist_kernel divides n_chains beds of H x W on n_cu compute units, restated from the comments of
    posterior_hist_kernel.hip: cell_blocks workgroups of 256 lanes, one cell per lane (`dead` lanes in the last one); the chain axis
    in parts = max(min(ceil(4 n_cu / cell_blocks), n_chains), ceil(n_chains / 65535)) of cpp = ceil(n_chains / parts) chains.  A full
    part takes `trips` trips of the loop with 8 loads in flight and then `rem` single chains; `last` is the chain count of the last
    part that holds a chain (`last_trips`, `last_rem` likewise) and `empty` the number of parts after it."""
    plane = H * W
    cell_blocks = -(-plane // HIST_BLOCK)
    parts = max(1, min(-(-4 * n_cu // cell_blocks), n_chains))
    parts = max(parts, -(-n_chains // HIST_MAX_CPP))
    cpp = -(-n_chains // parts)
    filled = -(-n_chains // cpp)
    last = n_chains - (filled - 1) * cpp
    return dict(cell_blocks=cell_blocks, dead=cell_blocks * HIST_BLOCK - plane, parts=parts, cpp=cpp, trips=cpp // HIST_CHAINS,
                rem=cpp % HIST_CHAINS, last=last, last_trips=last // HIST_CHAINS, last_rem=last % HIST_CHAINS, empty=parts - filled)
