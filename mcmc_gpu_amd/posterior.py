"""Posterior mean, spread and split-R-hat of the bed over all chains of a run, accumulated on the device.

The reference looks inside a run through host caches of ONE chain: bed_cache (only_save_last_bed=False, MCMC.py:1198, :1363)
and sample_values (set_sample_points_locations, MCMC.py:1174-1182, :1366), one whole-bed copy per iteration.  Here the chains
of a handle advance from snapshot to snapshot and a HIP kernel folds each snapshot into per-cell running sums that stay on the
device (gsm_posterior_* of include/gsm.h); only [H, W] maps and the thinned traces at the sample points come back.

Definitions.  Iterations are numbered as in the reference's caches: 0 is the initial bed, n_iter - 1 the last.
  snapshots   iterations k with burn_in <= k < n_iter and (k - burn_in) % thin == 0; T of them.
  sequences   split=False: every chain is one sequence of N = T snapshots.  split=True: the last 2N, N = T // 2, snapshots are
              used (an odd T drops the first) and every chain gives two sequences, its first and second half: M = 2C.
  per cell    mu_m, v_m: mean and ddof=1 variance of sequence m.  mean = mean of all M*N values; sd = sqrt of their ddof=1
              variance; W = mean_m(v_m); B_over_N = var_m(mu_m, ddof=1); rhat = sqrt(((N-1)/N W + B_over_N) / W), NaN where
              W == 0 (exactly the cells that are constant within every sequence).  A NaN bed value makes its cell NaN everywhere.
  rhat=False  mean and sd only, from sums pooled over the chains: no per-chain storage.
  sample_values[c, p, t]   bed of chain c at sample point p at snapshot t, for all T snapshots (also one that split drops).
  hist        optional per-cell histogram of the same M*N values about the common field g (gsm_posterior_histogram): `bins` = B
              equal bins of width w = 2 half_width / B over [g - half_width, g + half_width), an underflow, an overflow and a NaN
              slot, and per level the count of values below it.  Integer counts, on the device, added over ranks: quantiles to
              within w (PosteriorSummary.quantile, .interval) and P(bed < level) exactly (.prob_below).
  ess         optional effective sample size of the same M*N values (needs rhat: it uses W and B_over_N), BDA3 section 11.5 in
              variogram form.  Per cell and lag t = 1 .. K (`max_lag`, odd, <= 15): S_t = sum over the M sequences and n = 0 ..
              N - 1 - t of (x[n + t, m] - x[n, m])^2 -- both members of a pair in the same sequence --, accumulated on the device
              from a ring of every chain's last K snapshots (gsm_posterior_lagged) and added over ranks.  On the host V_t = S_t /
              (M (N - t)), var+ = (N - 1)/N W + B_over_N, rho_t = 1 - V_t / (2 var+), rho_0 = 1; Geyer pairs P_k = rho_2k +
              rho_(2k+1), k = 0 .. (K - 1)/2; tau = -1 + 2 sum of the pairs before the first negative one, floored at
              1 / log10(M N); ess = M N / tau and mcse = sd / sqrt(ess).  A cell without a negative pair sums them all and is
              flagged `truncated`: its ess is an upper bound (raise max_lag or thin).  NaN where W == 0 and where the cell saw a NaN.
  cov         optional covariance of every cell with K <= 15 linear functionals of the bed, f_k = sum over the support of Omega_k
              of Omega_k * bed: the posterior covariance matrix applied to the weight fields ("probes") Omega [K, H, W].  Per
              snapshot and chain, with d = bed - g, the device computes the projection p[c, k] = sum over the cells with Omega_k
              != 0 of Omega_k * d (gsm_posterior_project; zero weights are skipped, so a NaN bed outside a probe's support does
              not touch it) and adds d * p[c, k] to the cross sum Y [K, H, W] (gsm_posterior_cross) at the snapshots that belong
              to a sequence; Y adds over ranks.  With n = M N, S1 = n (mean - g) and q_k = sum of p over the same values:
              cov_k = (Y_k - S1 q_k / n) / (n - 1), pooled over all chains and snapshots, ddof=1.  probe_values[c, k, t] = f_k
              of chain c at snapshot t (Omega_k . g over the support, summed on the host, plus p), for all T snapshots.
  residual    optional maps of the mass-conservation residual r = d/dx(velx (surf - bed)) + d/dy(vely (surf - bed)) + dhdt - smb,
              the quantity every chain is scored on, over the same M*N values: the posterior predictive check of the sampler.  For
              chain c at a snapshot that belongs to a sequence, r is the residual of (double)bed_c with np.gradient's differences
              (one-sided at the four borders), bit for bit what gsm_residual gives for that bed.  rg [H, W] is the residual of the
              common field g, non-finite values set to 0 (residual_field, NumPy): a shift only, no result depends on it beyond
              rounding.  Per cell, over the values with finite r (the loss's nansum, MCMC.py:1041), the device keeps the fp64
              planes residual_sums [3 + L, H, W] (gsm_posterior_residual): cnt = their number, S1 = sum d, S2 = sum d d with d =
              r - rg, and for each of the L <= 4 `levels` (finite, >= 0, in the residual's unit) A_l = the number with |r| > level_l
              (a NaN compares false).  Counts are exact integers; no atomics, a fixed order (chains in index order within a part
              of the chain axis, parts in part order, snapshots in schedule order); the planes add over ranks.  On the host:
              residual_mean = rg + S1 / cnt, residual_sd = sqrt((S2 - S1^2 / cnt) / (cnt - 1)) (NaN where cnt < 2), residual_rms
              = sqrt(sum r^2 / cnt) with sum r^2 = S2 + 2 rg S1 + cnt rg^2, prob_residual_above(level) = A_l / cnt (exact),
              loss_density = sum r^2 / (2 sigma_mc^2 M N) on the cells with mc_mask == 1 (0 on the others) and expected_loss = its
              sum: the mean of chain.loss over the same M*N states.  A cell with cnt == 0 is NaN in the maps and adds 0 to the loss.
  local       optional covariance of every cell with its neighbours within `reach` R in 1 .. 4: the short-range structure of the
              uncertainty, which turns the per-cell sd into the sd of anything local and linear (a slope, a block mean).  The K = 2 R^2
              + 2 R offsets of the upper half plane (local_offsets: (0, 1) .. (0, R), then for di = 1 .. R: (di, -R) .. (di, R); the
              lower half plane holds the same pairs).  Per snapshot that belongs to a sequence, with d = bed - g, the device adds
              sum_c d_c[i, j] d_c[i + di, j + dj] to local_cross [K, H, W] where the partner lies inside the grid
              (gsm_posterior_local; the other entries stay exactly 0): fp64 fused multiply-adds, no atomics, a fixed order; the planes
              add over ranks.  On the host, with n = M N, m = mean - g at the cell and m' at its partner: local_covariance =
              (X_k - n m m') / (n - 1), pooled over all chains and snapshots, ddof=1 -- the expression that gives sd^2 at offset
              (0, 0) --, NaN where the partner is outside the grid.  From it local_correlation, difference_sd(di, dj),
              gradient_sd(resolution) and block_mean_sd(k).  A NaN bed makes NaN exactly the entries that pair its cell.
  regions     optional non-linear functionals of every chain's bed over K <= 8 regions (masks that may overlap, or a label map): the
              scalars an ensemble is published as.  Per snapshot (all T of them), chain and region the device writes eight slots
              (gsm_posterior_regions) over the cells whose bed x and surface s are finite: their number, sum x, sum max(s - x, 0) (ice
              thickness), sum max((s - x) + (rho_water / rho_ice) min(x - sea_level, 0), 0) (thickness above flotation), the number with x <
              sea_level, the number of those that are grounded (thickness above flotation > 0), min x and max x; fp64, no fused
              multiply-adds, a fixed summation tree.  region_values(what)[c, k, t] turns them into counts, volumes and areas (x
              resolution^2), region_stats() into mean, sd, 2.5 / 50 / 97.5 % quantiles and split-R-hat over the M N values.  With hyps=
              dict(lo, hi, bins) the device also counts, per chain and region, the valid cells per elevation bin (int32, an underflow and
              an overflow slot) over the snapshots that belong to a sequence: hypsometry().  Both are per chain: over ranks they are
              gathered in rank order (merge_regions), not summed.  Needs eng.set_static (the surface).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, fields

import numpy as np


def snapshot_iterations(n_iter, burn_in, thin):
    """The iterations of a run of n_iter iterations that are snapshots (ascending int64 array)."""
    n_iter, burn_in, thin = int(n_iter), int(burn_in), int(thin)
    if burn_in < 0:
        raise ValueError("burn_in must be >= 0")
    if thin < 1:
        raise ValueError("thin must be >= 1")
    return np.arange(burn_in, max(n_iter, burn_in), thin, dtype=np.int64)


def sequence_plan(n_iter, burn_in, thin, split=True):
    """(snapshot iterations, N snapshots per sequence, number of leading snapshots that belong to no sequence).  Raises
    ValueError when the schedule gives fewer than 2 snapshots (4 with split): a variance needs two values per sequence."""
    its = snapshot_iterations(n_iter, burn_in, thin)
    T = int(its.size)
    need = 4 if split else 2
    if T < need:
        raise ValueError(f"n_iter={int(n_iter)}, burn_in={int(burn_in)}, thin={int(thin)} give {T} snapshots; "
                         f"split={bool(split)} needs at least {need}")
    N = T // 2 if split else T
    return its, N, T - (2 * N if split else N)


@dataclass
class PosteriorSummary:
    """Maps are [H, W] float64.  rhat, within_var and between_var_over_n are None for a summary made with rhat=False;
    sample_values [n_chains, n_points, T] and sample_loc are None without sample points."""
    mean: np.ndarray
    sd: np.ndarray
    rhat: np.ndarray | None
    within_var: np.ndarray | None
    between_var_over_n: np.ndarray | None
    n_chains: int
    n_sequences: int
    n_per_sequence: int
    snapshot_iterations: np.ndarray
    burn_in: int
    thin: int
    split: bool
    sample_values: np.ndarray | None = None
    sample_loc: np.ndarray | None = None
    # with hist=: counts [B + 3, H, W] int64 (slot 0 underflow, 1 .. B the bins, B + 1 overflow, B + 2 NaN) of the M*N values about
    # hist_centre = g [H, W], bins of width 2 hist_half_width / B; level_counts [L, H, W] int64: values below level_values [L]
    hist_counts: np.ndarray | None = None
    hist_half_width: float | None = None
    hist_centre: np.ndarray | None = None
    level_values: np.ndarray | None = None
    level_counts: np.ndarray | None = None
    # with ess=: lag_sqdiff [K, H, W] float64, S_t of the lags t = 1 .. K over all M sequences
    lag_sqdiff: np.ndarray | None = None
    # with cov=: probes [K, H, W] float64 weight fields, probe_names K strings or None, probe_values [n_chains, K, T] the
    # functionals at all T snapshots, probe_cross [K, H, W] the cross sums Y about probe_centre = g [H, W]
    probes: np.ndarray | None = None
    probe_names: tuple | None = None
    probe_values: np.ndarray | None = None
    probe_cross: np.ndarray | None = None
    probe_centre: np.ndarray | None = None
    # with residual=: residual_sums [3 + L, H, W] float64 (cnt, S1, S2, then A_l per level) about residual_ref = rg [H, W];
    # residual_levels [L]; residual_sigma_mc and residual_mc_mask [H, W] bool: what the loss is made of
    residual_sums: np.ndarray | None = None
    residual_ref: np.ndarray | None = None
    residual_levels: np.ndarray | None = None
    residual_sigma_mc: float | None = None
    residual_mc_mask: np.ndarray | None = None
    # with local=: local_cross [K, H, W] float64, the cross sums of d = bed - local_centre (= g [H, W]) with d at the K = 2 R^2 + 2 R
    # offsets local_offsets(local_reach)
    local_cross: np.ndarray | None = None
    local_reach: int | None = None
    local_centre: np.ndarray | None = None
    # with regions=: region_func [n_chains, K, T, 8] float64, the eight slots of gsm_posterior_regions of every chain and region at
    # all T snapshots; region_masks [K, H, W] bool, region_names K strings; region_sea_level, region_density_ratio (rho_water /
    # rho_ice) and region_resolution (metres per cell) that the slots were made with; region_hyps [n_chains, K, B + 2] int64 cell
    # counts over the snapshots that belong to a sequence (slot 0 below region_hyps_range[0], B + 1 at or above region_hyps_range[1])
    region_func: np.ndarray | None = None
    region_masks: np.ndarray | None = None
    region_names: tuple | None = None
    region_sea_level: float | None = None
    region_density_ratio: float | None = None
    region_resolution: float | None = None
    region_hyps: np.ndarray | None = None
    region_hyps_range: np.ndarray | None = None

    def _need_regions(self):
        if self.region_func is None or self.region_resolution is None:
            raise ValueError("this summary holds no region functionals: run with posterior=dict(..., regions=dict(masks=...))")
        return np.asarray(self.region_func, dtype=np.float64)

    def region_values(self, what):
        """[n_chains, K, T] the quantity `what` (one of REGION_QUANTITIES) of every chain and region at all T snapshots: count (valid
        cells), mean_bed (NaN for a region without a valid cell), volume (ice thickness summed, x resolution^2), volume_above_flotation,
        area_below_sea_level, area_marine_grounded (below sea level and grounded: thickness above flotation > 0), min_bed and max_bed
        (NaN for a region without a valid cell)."""
        F = self._need_regions()
        a = float(self.region_resolution) ** 2
        if what not in REGION_QUANTITIES:
            raise KeyError(f"unknown region quantity {what!r}; the quantities are {REGION_QUANTITIES}")
        if what == "count":
            return F[..., 0].copy()
        if what == "mean_bed":
            with np.errstate(invalid="ignore", divide="ignore"):
                return np.where(F[..., 0] > 0, F[..., 1] / F[..., 0], np.nan)
        if what in ("min_bed", "max_bed"):
            v = F[..., 6 if what == "min_bed" else 7]
            return np.where(F[..., 0] > 0, v, np.nan)
        return F[..., {"volume": 2, "volume_above_flotation": 3, "area_below_sea_level": 4, "area_marine_grounded": 5}[what]] * a

    def region_stats(self):
        """{quantity: dict(mean, sd, q025, q50, q975, rhat)}, each [K], of every quantity of REGION_QUANTITIES over the M N values
        that mean and sd describe (the snapshots that split drops are left out, every chain cut into the summary's sequences): mean,
        ddof=1 sd, the 2.5 / 50 / 97.5 % quantiles (NumPy's default, linear) and the split R-hat of probe_stats()."""
        self._need_regions()
        out = {}
        for what in REGION_QUANTITIES:
            s = self._sequences(self.region_values(what))
            st = _sequence_stats(s)
            with np.errstate(invalid="ignore"):
                q = np.quantile(s.reshape(-1, s.shape[2]), (0.025, 0.5, 0.975), axis=0)
            out[what] = dict(mean=st["mean"], sd=st["sd"], q025=q[0], q50=q[1], q975=q[2], rhat=st["rhat"])
        return out

    def hypsometry(self):
        """dict(edges [B + 1] the bin edges in metres; area [n_chains, K, B + 2] every chain's mean area per slot over its snapshots
        that belong to a sequence (slot 0: below edges[0], slots 1 .. B the bins, slot B + 1: at or above edges[B]), in resolution^2;
        mean [K, B + 2] the mean of `area` over the chains: the pooled hypsometric curve)."""
        self._need_regions()
        if self.region_hyps is None or self.region_hyps_range is None:
            raise ValueError("this summary holds no hypsometry: run with regions=dict(..., hyps=dict(lo=, hi=, bins=))")
        cnt = np.asarray(self.region_hyps, dtype=np.float64)
        B = cnt.shape[2] - 2
        lo, hi = (float(v) for v in np.asarray(self.region_hyps_range).ravel())
        n = self.n_per_sequence * (2 if self.split else 1)
        area = cnt / n * float(self.region_resolution) ** 2
        return dict(edges=lo + np.arange(B + 1) * ((hi - lo) / B), area=area, mean=area.mean(axis=0))

    def _sequences(self, v):
        """[M, N, K] from per-chain traces v [C, K, T]: the M N values that mean and sd describe -- v without the snapshots that split
        drops, every chain cut into its sequences."""
        v = np.asarray(v, dtype=np.float64)
        C, K, T = v.shape
        N = self.n_per_sequence
        n_seq = 2 if self.split else 1
        return v[:, :, T - n_seq * N:].transpose(0, 2, 1).reshape(C * n_seq, N, K)

    def _need_local(self, reach=1, what=None):
        if self.local_cross is None or self.local_reach is None or self.local_centre is None:
            raise ValueError("this summary holds no local cross sums: run with posterior=dict(..., local=dict(reach=...))")
        if int(self.local_reach) < reach:
            raise ValueError(f"{what} needs local reach >= {reach}, this summary was made with reach {int(self.local_reach)}")
        return self.n_sequences * self.n_per_sequence

    def local_covariance(self):
        """[K, H, W] covariance of every cell with its partner at offset k of local_offsets(local_reach) over the M N values, ddof=1:
        (X_k - n m m') / (n - 1), m = mean - g at the cell and m' at the partner.  NaN where the partner is outside the grid and
        where either mean is NaN."""
        n = self._need_local()
        X = np.asarray(self.local_cross, dtype=np.float64)
        m = np.asarray(self.mean, dtype=np.float64) - np.asarray(self.local_centre, dtype=np.float64)
        out = np.empty_like(X)
        with np.errstate(invalid="ignore"):
            for k, (di, dj) in enumerate(local_offsets(self.local_reach)):
                mp = _shifted(m, di, dj)
                out[k] = np.where(np.isnan(mp), np.nan, (X[k] - n * m * mp) / (n - 1))
        return out

    def local_correlation(self):
        """[K, H, W] local_covariance() / (sd of the cell * sd of its partner).  NaN where either sd is 0."""
        cov = self.local_covariance()
        sd = np.asarray(self.sd, dtype=np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            for k, (di, dj) in enumerate(local_offsets(self.local_reach)):
                sp = _shifted(sd, di, dj)
                cov[k] = np.where((sd == 0) | (sp == 0), np.nan, cov[k] / (sd * sp))
        return cov

    def _pair_covariance(self, di, dj, what):
        """[H, W] covariance of bed[i, j] with bed[i + di, j + dj] for any offset within reach, either sign; sd^2 at (0, 0)."""
        di, dj = int(di), int(dj)
        self._need_local(max(abs(di), abs(dj), 1), what)
        if di == 0 and dj == 0:
            return np.asarray(self.sd, dtype=np.float64) ** 2
        table = [tuple(o) for o in local_offsets(self.local_reach).tolist()]
        cov = self.local_covariance()
        if (di, dj) in table:
            return cov[table.index((di, dj))]
        return _shifted(cov[table.index((-di, -dj))], di, dj)          # the pair is held at the partner, under the opposite offset

    def difference_sd(self, di, dj):
        """[H, W] standard deviation of bed[i + di, j + dj] - bed[i, j] over the M N values (ddof=1), for any offset within reach,
        either sign: sqrt(var + var' - 2 cov).  NaN where the partner is outside the grid."""
        what = f"difference_sd({int(di)}, {int(dj)})"
        cov = self._pair_covariance(di, dj, what)
        var = np.asarray(self.sd, dtype=np.float64) ** 2
        with np.errstate(invalid="ignore"):
            v = var + _shifted(var, int(di), int(dj)) - 2.0 * cov
            return np.sqrt(np.where(np.isnan(v), np.nan, np.maximum(v, 0.0)))

    def gradient_sd(self, resolution):
        """(sd along axis 0, sd along axis 1), each [H, W]: the standard deviation of the central differences np.gradient(bed,
        resolution) takes in the interior, (bed[i + 1] - bed[i - 1]) / (2 resolution).  NaN in the first and last row (column), where
        np.gradient takes one-sided differences.  Needs reach >= 2."""
        h = float(resolution)
        if not (h > 0.0 and np.isfinite(h)):
            raise ValueError(f"resolution must be finite and > 0, got {resolution!r}")
        self._need_local(2, "gradient_sd")
        # sd of bed[i + 2] - bed[i] is held at i: moved to i + 1, the cell the difference is centred on
        return tuple(_shifted(self.difference_sd(di, dj), -di // 2, -dj // 2) / (2.0 * h) for di, dj in ((2, 0), (0, 2)))

    def block_mean_sd(self, k):
        """[H - k + 1, W - k + 1] standard deviation of the mean of the bed over every k x k block (entry [i, j]: the block with its
        first cell at (i, j)): sqrt of the sum of all pair covariances in the block over k^4.  Needs reach >= k - 1."""
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
            raise ValueError(f"block_mean_sd: k must be an integer >= 1, got {k!r}")
        k = int(k)
        self._need_local(max(k - 1, 1), f"block_mean_sd({k})")
        H, W = np.asarray(self.sd).shape
        if k > H or k > W:
            raise ValueError(f"block_mean_sd: a {k} x {k} block does not fit the {H} x {W} grid")
        nh, nw = H - k + 1, W - k + 1
        var = np.asarray(self.sd, dtype=np.float64) ** 2
        total = np.zeros((nh, nw))
        for a in range(k):
            for b in range(k):
                total += var[a:a + nh, b:b + nw]
        cov = self.local_covariance()
        for idx, (di, dj) in enumerate(local_offsets(self.local_reach).tolist()):
            if di > k - 1 or abs(dj) > k - 1:
                continue
            for a in range(k - di):                                    # the cells of the block whose partner is in the block too
                for b in range(max(0, -dj), min(k, k - dj)):
                    total += 2.0 * cov[idx][a:a + nh, b:b + nw]
        with np.errstate(invalid="ignore"):
            return np.sqrt(np.where(np.isnan(total), np.nan, np.maximum(total, 0.0))) / (k * k)

    def _need_residual(self):
        if self.residual_sums is None or self.residual_ref is None:
            raise ValueError("this summary holds no residual sums: run with posterior=dict(..., residual=True)")
        P = np.asarray(self.residual_sums, dtype=np.float64)
        return P[0], P[1], P[2], np.asarray(self.residual_ref, dtype=np.float64)

    def residual_count(self):
        """[H, W] int64: how many of the M*N values of every cell have a finite residual."""
        return self._need_residual()[0].astype(np.int64)

    def residual_mean(self):
        """[H, W] mean of the finite residuals of every cell: rg + S1 / cnt.  NaN where cnt == 0."""
        cnt, S1, _, rg = self._need_residual()
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(cnt > 0, rg + S1 / cnt, np.nan)

    def residual_sd(self):
        """[H, W] ddof=1 standard deviation of the finite residuals of every cell: how far the chains disagree.  NaN where cnt < 2."""
        cnt, S1, S2, _ = self._need_residual()
        with np.errstate(invalid="ignore", divide="ignore"):
            var = np.maximum(S2 - S1 * S1 / cnt, 0.0) / (cnt - 1)
            return np.where(cnt > 1, np.sqrt(var), np.nan)

    def _residual_sumsq(self):
        cnt, S1, S2, rg = self._need_residual()
        return S2 + 2.0 * rg * S1 + cnt * rg * rg

    def residual_rms(self):
        """[H, W] root mean square of the finite residuals of every cell.  NaN where cnt == 0."""
        cnt = self._need_residual()[0]
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(cnt > 0, np.sqrt(np.maximum(self._residual_sumsq(), 0.0) / cnt), np.nan)

    def prob_residual_above(self, level):
        """[H, W] share of the finite residuals of every cell with |r| > level (exact: a ratio of counts; NaN where cnt == 0).
        KeyError for a level that the run was not asked to count."""
        cnt = self._need_residual()[0]
        levels = [] if self.residual_levels is None else [float(v) for v in np.asarray(self.residual_levels).ravel()]
        if float(level) not in levels:
            raise KeyError(f"level {level!r} was not counted; the levels of this summary are {levels}")
        above = np.asarray(self.residual_sums, dtype=np.float64)[3 + levels.index(float(level))]
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(cnt > 0, above / cnt, np.nan)

    def loss_density(self):
        """[H, W] every cell's term of expected_loss(): sum r^2 / (2 sigma_mc^2 M N) where mc_mask == 1, 0 elsewhere; NaN where cnt == 0."""
        cnt = self._need_residual()[0]
        if self.residual_sigma_mc is None or self.residual_mc_mask is None:
            raise ValueError("this summary holds no sigma_mc / mc_mask")
        n = self.n_sequences * self.n_per_sequence
        dens = self._residual_sumsq() / (2.0 * float(self.residual_sigma_mc) ** 2 * n)
        dens = np.where(np.asarray(self.residual_mc_mask) == 1, dens, 0.0)
        return np.where(cnt > 0, dens, np.nan)

    def expected_loss(self):
        """The mean of the chains' loss over the M*N states: the sum of loss_density() (a cell without a finite residual adds 0, as
        the loss's nansum does)."""
        return float(np.nansum(self.loss_density()))

    def _need_cov(self):
        if self.probes is None or self.probe_cross is None or self.probe_values is None:
            raise ValueError("this summary holds no probes: run with posterior=dict(..., cov=dict(probes=...))")
        return self.n_sequences * self.n_per_sequence

    def _probe_sequences(self):
        """[M, N, K] the functionals at the M N values that mean and sd describe: probe_values without the snapshots that split drops,
        every chain cut into its sequences."""
        return self._sequences(self.probe_values)

    def covariance(self):
        """[K, H, W] covariance of every cell with every functional over the M N values, ddof=1: (Y_k - S1 q_k / n) / (n - 1) with
        S1 = n (mean - g) and q_k the sum of the projections.  NaN where `mean` is NaN and for a probe that saw a NaN."""
        n = self._need_cov()
        g = np.asarray(self.probe_centre, dtype=np.float64)
        P = np.asarray(self.probes, dtype=np.float64)
        with np.errstate(invalid="ignore"):
            off = np.array([(w[w != 0] * g[w != 0]).sum() for w in P])
            q = np.array([math.fsum(v) for v in (self._probe_sequences().reshape(n, -1) - off).T])   # exactly rounded: no order to depend on
            S1 = n * (np.asarray(self.mean, dtype=np.float64) - g)
            cov = (np.asarray(self.probe_cross, dtype=np.float64) - S1[None] * q[:, None, None] / n) / (n - 1)
        cov[:, np.isnan(self.mean)] = np.nan
        return cov

    def probe_stats(self):
        """dict of host statistics of the functionals over the same M N values: mean [K], sd [K] (ddof=1), rhat [K] (split R-hat over
        the summary's sequences, NaN where the within-sequence variance is 0 or there is one sequence) and cov [K, K], the ddof=1
        covariance of the functionals with each other."""
        self._need_cov()
        return _sequence_stats(self._probe_sequences())

    def correlation(self):
        """[K, H, W] covariance() / (sd of the cell * sd of the functional).  NaN where either sd is 0."""
        cov = self.covariance()
        sd = np.asarray(self.sd, dtype=np.float64)
        sd_f = self.probe_stats()["sd"]
        with np.errstate(invalid="ignore", divide="ignore"):
            rho = cov / (sd[None] * sd_f[:, None, None])
        rho[:, sd == 0] = np.nan
        rho[sd_f == 0] = np.nan
        return rho

    def sketch(self):
        """(probes [K, H, W], covariance() [K, H, W]) = (Omega, (C Omega^T)^T): the pair a randomized low-rank factorisation of the
        posterior covariance matrix C consumes (range finder: an orthonormal basis of the columns of C Omega^T; with Gaussian
        probes its span approaches that of the leading eigenvectors of C).  The factorisation itself is not part of this class."""
        return np.asarray(self.probes, dtype=np.float64), self.covariance()

    def _need_hist(self):
        if self.hist_counts is None:
            raise ValueError("this summary holds no histogram: run with posterior=dict(..., hist=dict(half_width=...))")
        return int(self.hist_counts.shape[0]) - 3, self.n_sequences * self.n_per_sequence

    def prob_below(self, l):
        """[H, W] share of the M*N values of every cell that lie below level_values[l] (strictly; exact: a ratio of counts)."""
        _, n = self._need_hist()
        return np.asarray(self.level_counts)[l] / n

    def quantile(self, q):
        """[H, W] q-quantile of the M*N values of every cell, 0 < q <= 1, from the histogram: the bin s in which the cumulative
        count reaches the rank ceil(q n) holds the order statistic of that rank (NumPy's method='inverted_cdf'), and the value
        returned is placed inside that bin by the share of its count below q n, so it is within one bin width of that order
        statistic.  NaN where the rank falls into the underflow or the overflow slot and where the cell saw a NaN."""
        B, n = self._need_hist()
        q = float(q)
        if not 0.0 < q <= 1.0:
            raise ValueError("q must be in (0, 1]")
        cnt = np.asarray(self.hist_counts, dtype=np.int64)
        w = 2.0 * float(self.hist_half_width) / B
        cum = np.cumsum(cnt[:B + 2], axis=0)
        s = np.argmax(cum >= np.ceil(q * n), axis=0)
        here = np.take_along_axis(cnt, s[None], axis=0)[0]
        before = np.take_along_axis(cum, s[None], axis=0)[0] - here
        with np.errstate(invalid="ignore", divide="ignore"):
            val = np.asarray(self.hist_centre, dtype=np.float64) + (s - 1 - B // 2) * w + (q * n - before) / here * w
        return np.where((s == 0) | (s == B + 1) | (cnt[B + 2] != 0), np.nan, val)

    def interval(self, p):
        """(lower, upper) [H, W] maps of the central credible interval of probability p: quantile((1 - p) / 2), quantile((1 + p) / 2)."""
        p = float(p)
        if not 0.0 < p < 1.0:
            raise ValueError("p must be in (0, 1)")
        return self.quantile((1.0 - p) / 2.0), self.quantile((1.0 + p) / 2.0)

    def autocorrelation(self):
        """[K, H, W] rho_t of the lags t = 1 .. K: 1 - S_t / (M (N - t)) / (2 var+).  NaN where W == 0 and where the cell saw a NaN."""
        if self.lag_sqdiff is None or self.within_var is None:
            raise ValueError("this summary holds no lagged sums: run with posterior=dict(..., ess=dict(max_lag=...))")
        S = np.asarray(self.lag_sqdiff, dtype=np.float64)
        M, N = self.n_sequences, self.n_per_sequence
        W = np.asarray(self.within_var, dtype=np.float64)
        rho = np.empty_like(S)
        with np.errstate(invalid="ignore", divide="ignore"):
            var_plus = (N - 1) / N * W + np.asarray(self.between_var_over_n, dtype=np.float64)
            for t in range(1, S.shape[0] + 1):
                rho[t - 1] = 1.0 - S[t - 1] / (M * (N - t)) / (2.0 * var_plus)
        rho[:, (W == 0) | np.isnan(self.mean)] = np.nan
        return rho

    def ess(self):
        """(ess, truncated): [H, W] effective sample size of the M*N values of every cell, M N / tau with tau from Geyer's pairs of
        autocorrelation(), and the bool map of the cells in which no pair up to max_lag was negative (ess is an upper bound there)."""
        rho = self.autocorrelation()
        K, n = rho.shape[0], self.n_sequences * self.n_per_sequence
        if K % 2 == 0:
            raise ValueError(f"lag_sqdiff holds {K} lags; Geyer's pairs need an odd number")
        tau = np.full(rho.shape[1:], -1.0)
        alive = ~np.isnan(rho).any(axis=0)                   # no negative pair so far
        with np.errstate(invalid="ignore", divide="ignore"):
            for k in range((K + 1) // 2):
                pair = (1.0 if k == 0 else rho[2 * k - 1]) + rho[2 * k]
                alive &= ~(pair < 0)
                tau = np.where(alive, tau + 2.0 * pair, tau)
            tau = np.where(np.isnan(rho).any(axis=0), np.nan, np.maximum(tau, 1.0 / np.log10(n)))
            return n / tau, alive

    def mcse(self):
        """[H, W] Monte-Carlo standard error of `mean`: sd / sqrt(ess)."""
        with np.errstate(invalid="ignore"):
            return np.asarray(self.sd, dtype=np.float64) / np.sqrt(self.ess()[0])

    def save(self, path):
        """One .npz; fields that are None are left out."""
        np.savez_compressed(path, **{f.name: np.asarray(getattr(self, f.name)) for f in fields(self)
                                     if getattr(self, f.name) is not None})

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            kw = {f.name: (z[f.name] if f.name in z.files else None) for f in fields(cls)}
        for k in ("n_chains", "n_sequences", "n_per_sequence", "burn_in", "thin"):
            kw[k] = int(kw[k])
        kw["split"] = bool(kw["split"])
        if kw["hist_half_width"] is not None:
            kw["hist_half_width"] = float(kw["hist_half_width"])
        if kw["probe_names"] is not None:
            kw["probe_names"] = tuple(str(v) for v in kw["probe_names"])
        if kw["residual_sigma_mc"] is not None:
            kw["residual_sigma_mc"] = float(kw["residual_sigma_mc"])
        if kw["local_reach"] is not None:
            kw["local_reach"] = int(kw["local_reach"])
        if kw["region_names"] is not None:
            kw["region_names"] = tuple(str(v) for v in kw["region_names"])
        for k in ("region_sea_level", "region_density_ratio", "region_resolution"):
            if kw[k] is not None:
                kw[k] = float(kw[k])
        return cls(**kw)


def _sequence_stats(s):
    """dict(mean [K], sd [K] (ddof=1), rhat [K], cov [K, K]) of K scalar quantities over M sequences of N values, s [M, N, K]: pooled
    over all M N values, and the split R-hat over the sequences (NaN where the within-sequence variance is 0 or there is one sequence)."""
    M, N, K = s.shape
    n = M * N
    flat = s.reshape(n, K)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = flat.mean(axis=0)
        dev = flat - mean
        cov = dev.T @ dev / (n - 1)
        mu = s.mean(axis=1)
        v = np.where((s == s[:, :1]).all(axis=1), 0.0, s.var(axis=1, ddof=1))
        W = v.mean(axis=0)
        B_over_N = mu.var(axis=0, ddof=1) if M > 1 else np.full(K, np.nan)
        rhat = np.where(W == 0, np.nan, np.sqrt(((N - 1) / N * W + B_over_N) / W))
    return dict(mean=mean, sd=np.sqrt(np.diagonal(cov)), rhat=rhat, cov=cov)


def _host_array(x, shape, dtype, what):
    """A device tensor or an array as a new numpy array of `dtype`; ValueError unless it has `shape`."""
    a = np.array(x.detach().cpu().numpy() if hasattr(x, "detach") else x, dtype=dtype)
    if a.shape != tuple(shape):
        raise ValueError(f"{what} of shape {a.shape}, expected {tuple(shape)}")
    return a


def finalize(partials_sum, M, N, common_ref, rhat=True, **meta):
    """PosteriorSummary from the partials summed over all handles / ranks (gsm_posterior_partials), the number of sequences
    M behind them, the snapshots per sequence N and the common field g.  partials_sum [3, H, W]: with rhat, P0 = sum_m a_m,
    P1 = sum_m a_m^2, P2 = sum_m v_m (a_m: sequence mean minus g, v_m: sequence variance); without, P0 = sum d, P1 = sum d^2
    over all M*N values, d = bed - g.  meta: the remaining PosteriorSummary fields."""
    g = np.asarray(common_ref, dtype=np.float64)
    P = _host_array(partials_sum, (3,) + g.shape, np.float64, "partials")
    M, N = int(M), int(N)
    if N < 2 or M < 1:
        raise ValueError("need at least one sequence of at least two snapshots")
    with np.errstate(invalid="ignore", divide="ignore"):
        if rhat:
            if M < 2:
                raise ValueError("rhat needs at least two sequences")
            mean = g + P[0] / M
            W = P[2] / M
            ss_between = P[1] - P[0] * P[0] / M
            B_over_N = ss_between / (M - 1)
            var = ((N - 1) * P[2] + N * ss_between) / (M * N - 1)
            r = np.sqrt(((N - 1) / N * W + B_over_N) / W)
            r = np.where(W == 0, np.nan, r)
        else:
            n = M * N
            mean = g + P[0] / n
            var = (P[1] - P[0] * P[0] / n) / (n - 1)
            W = B_over_N = r = None
        sd = np.sqrt(var)
    return PosteriorSummary(mean=mean, sd=sd, rhat=r, within_var=W, between_var_over_n=B_over_N, n_sequences=M, n_per_sequence=N, **meta)


ESS_KEYS = ("max_lag",)
ESS_MAX_LAG = 15


def check_ess(ess, N=None, rhat=True):
    """Validate the `ess` option: None (also False), True (the default) or dict(max_lag=7).  Returns None or dict(max_lag=K), K an
    odd int in [1, 15] and, when the snapshots per sequence N are given, at most N - 1 (lag t needs N - t >= 1 pairs)."""
    if ess is None or ess is False:
        return None
    if ess is True:
        ess = {}
    if not isinstance(ess, dict):
        raise ValueError("ess must be None, True or a dict with the key max_lag")
    unknown = set(ess) - set(ESS_KEYS)
    if unknown:
        raise ValueError(f"unknown ess option(s) {sorted(unknown)}; the options are {ESS_KEYS}")
    K = ess.get("max_lag", 7)
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or K < 1 or K > ESS_MAX_LAG or K % 2 == 0:
        raise ValueError(f"ess max_lag must be an odd integer in [1, {ESS_MAX_LAG}], got {K!r}")
    if not rhat:
        raise ValueError("ess needs rhat=True: the autocorrelation uses the within- and between-sequence variances")
    if N is not None and K > int(N) - 1:
        raise ValueError(f"ess max_lag={int(K)} needs at least {int(K) + 1} snapshots per sequence, the schedule gives {int(N)}: "
                         f"lower max_lag or thin less")
    return dict(max_lag=int(K))


COV_KEYS = ("probes", "names")
COV_MAX_PROBES = 15


def check_cov(cov, H=None, W=None):
    """Validate the `cov` option: None, or dict(probes=<[K, H, W] or [H, W] finite floats>, names=<K strings, optional>) with 1 <= K
    <= 15 and at least one non-zero weight in every probe.  Returns None or dict(probes=<[K, h, w] float64, contiguous>, names=<tuple
    of K str, or None>); with H and W given the probes must have the grid's shape."""
    if cov is None:
        return None
    if not isinstance(cov, dict):
        raise ValueError("cov must be None or a dict with the key probes and optionally names")
    unknown = set(cov) - set(COV_KEYS)
    if unknown:
        raise ValueError(f"unknown cov option(s) {sorted(unknown)}; the options are {COV_KEYS}")
    if "probes" not in cov:
        raise ValueError("cov needs probes: an array [K, H, W] of weight fields")
    try:
        P = np.array(cov["probes"], dtype=np.float64, order="C")
    except (TypeError, ValueError):
        raise ValueError("cov probes must be an array of numbers of shape [K, H, W] or [H, W]") from None
    if P.ndim == 2:
        P = P[None]
    if P.ndim != 3 or 0 in P.shape:
        raise ValueError(f"cov probes must have shape [K, H, W] or [H, W] with K >= 1, got {P.shape}")
    if H is not None and P.shape[1:] != (int(H), int(W)):
        raise ValueError(f"cov probes of shape {P.shape}, the grid is {(int(H), int(W))}")
    K = P.shape[0]
    if K > COV_MAX_PROBES:
        raise ValueError(f"cov takes at most {COV_MAX_PROBES} probes, got {K}")
    if not np.isfinite(P).all():
        raise ValueError("cov probes must be finite")
    if not (P != 0).any(axis=(1, 2)).all():
        raise ValueError("every cov probe needs at least one non-zero weight")
    names = cov.get("names")
    if names is not None:
        if isinstance(names, str) or not all(isinstance(v, str) for v in names) or len(names) != K:
            raise ValueError(f"cov names must be a sequence of {K} strings, one per probe")
        names = tuple(names)
    return dict(probes=P, names=names)


def point_probes(H, W, cells):
    """[K, H, W] indicator probes at the flat cell indices `cells` (row * W + col): the covariance and correlation maps with
    those points."""
    cells = np.asarray(cells, dtype=np.int64).ravel()
    if cells.size == 0 or (cells < 0).any() or (cells >= int(H) * int(W)).any():
        raise ValueError("point_probes: cell outside the grid")
    P = np.zeros((cells.size, int(H) * int(W)))
    P[np.arange(cells.size), cells] = 1.0
    return P.reshape(cells.size, int(H), int(W))


def region_mean_probes(masks):
    """[K, H, W] probes of region means: each mask of `masks` ([K, H, W] or [H, W], non-zero = inside) divided by its cell count."""
    m = np.asarray(masks) != 0
    if m.ndim == 2:
        m = m[None]
    count = m.sum(axis=(1, 2)) if m.ndim == 3 else np.zeros(1)
    if m.ndim != 3 or (count == 0).any():
        raise ValueError("region_mean_probes: masks must be [K, H, W] or [H, W] with at least one cell inside each")
    return m / count[:, None, None].astype(np.float64)


RESIDUAL_KEYS = ("levels",)
RESIDUAL_MAX_LEVELS = 4


def check_residual(residual):
    """Validate the `residual` option: None (also False), True or dict(levels=(l1, ...)) with up to 4 finite thresholds >= 0 on |r|.
    Returns None or dict(levels=<tuple of floats>)."""
    if residual is None or residual is False:
        return None
    if residual is True:
        residual = {}
    if not isinstance(residual, dict):
        raise ValueError("residual must be None, True or a dict with the key levels")
    unknown = set(residual) - set(RESIDUAL_KEYS)
    if unknown:
        raise ValueError(f"unknown residual option(s) {sorted(unknown)}; the options are {RESIDUAL_KEYS}")
    try:
        levels = tuple(float(v) for v in np.asarray(residual.get("levels", ()), dtype=np.float64).ravel())
    except (TypeError, ValueError):
        raise ValueError("residual levels must be a sequence of numbers") from None
    if len(levels) > RESIDUAL_MAX_LEVELS:
        raise ValueError(f"residual takes at most {RESIDUAL_MAX_LEVELS} levels, got {len(levels)}")
    if not all(np.isfinite(v) and v >= 0.0 for v in levels):
        raise ValueError(f"residual levels must be finite and >= 0, got {levels}")
    return dict(levels=levels)


def residual_field(bed, surf, velx, vely, dhdt, smb, resolution):
    """[H, W] mass-conservation residual of one bed in NumPy's np.gradient form (Topography.py:592-600)."""
    thick = np.asarray(surf, dtype=np.float64) - np.asarray(bed, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        dx = np.gradient(np.asarray(velx, dtype=np.float64) * thick, float(resolution), axis=1)
        dy = np.gradient(np.asarray(vely, dtype=np.float64) * thick, float(resolution), axis=0)
        return dx + dy + np.asarray(dhdt, dtype=np.float64) - np.asarray(smb, dtype=np.float64)


LOCAL_KEYS = ("reach",)
LOCAL_MAX_REACH = 4


def local_offsets(reach):
    """[K, 2] int64 table of the K = 2 R^2 + 2 R offsets (di, dj) of the upper half plane within reach R, in the order of the planes
    of local_cross: (0, 1) .. (0, R), then for di = 1 .. R: (di, -R) .. (di, R)."""
    if isinstance(reach, bool) or not isinstance(reach, (int, np.integer)) or reach < 1 or reach > LOCAL_MAX_REACH:
        raise ValueError(f"local reach must be an integer in [1, {LOCAL_MAX_REACH}], got {reach!r}")
    R = int(reach)
    return np.array([(0, dj) for dj in range(1, R + 1)] + [(di, dj) for di in range(1, R + 1) for dj in range(-R, R + 1)], dtype=np.int64)


def check_local(local):
    """Validate the `local` option: None (also False), True (reach 1) or dict(reach=R), R an integer in [1, 4].  Returns None or
    dict(reach=R)."""
    if local is None or local is False:
        return None
    if local is True:
        local = {}
    if not isinstance(local, dict):
        raise ValueError("local must be None, True or a dict with the key reach")
    unknown = set(local) - set(LOCAL_KEYS)
    if unknown:
        raise ValueError(f"unknown local option(s) {sorted(unknown)}; the options are {LOCAL_KEYS}")
    R = local.get("reach", 1)
    local_offsets(R)
    return dict(reach=int(R))


def _shifted(a, di, dj):
    """b[i, j] = a[i + di, j + dj], NaN where that cell is outside the grid."""
    a = np.asarray(a, dtype=np.float64)
    H, W = a.shape
    b = np.full((H, W), np.nan)
    i0, i1, j0, j1 = max(0, -di), min(H, H - di), max(0, -dj), min(W, W - dj)
    if i0 < i1 and j0 < j1:
        b[i0:i1, j0:j1] = a[i0 + di:i1 + di, j0 + dj:j1 + dj]
    return b


REGION_KEYS = ("masks", "names", "sea_level", "rho_ice", "rho_water", "hyps")
REGION_HYPS_KEYS = ("lo", "hi", "bins")
REGION_MAX, REGION_MAX_BINS = 8, 64
REGION_QUANTITIES = ("count", "mean_bed", "volume", "volume_above_flotation", "area_below_sea_level", "area_marine_grounded", "min_bed",
                     "max_bed")


def check_regions(regions, H=None, W=None):
    """Validate the `regions` option: None, or dict(masks=, names=None, sea_level=0.0, rho_ice=917.0, rho_water=1028.0, hyps=None).
    masks: [K, H, W] (or [H, W], K = 1) bool or numbers, non-zero = inside, regions may overlap and may be empty; or an integer label
    map [H, W], label k in 1 .. K = region k - 1 and label 0 = no region; K <= 8.  names: K strings.  hyps: None or dict(lo=, hi=,
    bins=) with finite lo < hi (metres) and bins even in [2, 64].  Returns None or dict(masks=<[K, h, w] bool>, names=<tuple of K str>,
    sea_level, rho_ice, rho_water, hyps=<None or dict(lo, hi, bins)>); with H and W given the masks must have the grid's shape."""
    if regions is None:
        return None
    if not isinstance(regions, dict):
        raise ValueError("regions must be None or a dict with the key masks and optionally names, sea_level, rho_ice, rho_water, hyps")
    unknown = set(regions) - set(REGION_KEYS)
    if unknown:
        raise ValueError(f"unknown regions option(s) {sorted(unknown)}; the options are {REGION_KEYS}")
    if "masks" not in regions:
        raise ValueError("regions needs masks: a bool array [K, H, W] or an integer label map [H, W]")
    m = np.asarray(regions["masks"])
    if m.dtype == object or not (m.dtype == bool or np.issubdtype(m.dtype, np.number)):
        raise ValueError("regions masks must be an array of bools or numbers")
    if m.ndim == 2 and np.issubdtype(m.dtype, np.integer):
        if m.size and m.min() < 0:
            raise ValueError("regions labels must be >= 0 (0 = no region)")
        K = int(m.max()) if m.size else 0
        if K > REGION_MAX:
            raise ValueError(f"regions takes at most {REGION_MAX} regions, the label map goes up to {K}")
        m = np.stack([m == k for k in range(1, K + 1)]) if K else np.zeros((0,) + m.shape, dtype=bool)
    else:
        if m.ndim == 2:
            m = m[None]
        if m.ndim == 3 and m.shape[0] > REGION_MAX:
            raise ValueError(f"regions takes at most {REGION_MAX} regions, got {m.shape[0]}")
        with np.errstate(invalid="ignore"):
            m = m != 0
    if m.ndim != 3 or 0 in m.shape:
        raise ValueError(f"regions masks must have shape [K, H, W] with 1 <= K <= {REGION_MAX}, or be an integer label map [H, W] with a label "
                         f"above 0; got {np.asarray(regions['masks']).shape}")
    if H is not None and m.shape[1:] != (int(H), int(W)):
        raise ValueError(f"regions masks of shape {m.shape}, the grid is {(int(H), int(W))}")
    K = m.shape[0]
    names = regions.get("names")
    if names is None:
        names = tuple(f"region{k}" for k in range(K))
    elif isinstance(names, str) or not all(isinstance(v, str) for v in names) or len(names) != K:
        raise ValueError(f"regions names must be a sequence of {K} strings, one per region")
    out = dict(masks=np.ascontiguousarray(m), names=tuple(names))
    for key, default, positive in (("sea_level", 0.0, False), ("rho_ice", 917.0, True), ("rho_water", 1028.0, True)):
        try:
            v = float(regions.get(key, default))
        except (TypeError, ValueError):
            raise ValueError(f"regions {key} must be a number, got {regions.get(key)!r}") from None
        if not np.isfinite(v) or (positive and not v > 0.0):
            raise ValueError(f"regions {key} must be finite{' and > 0' if positive else ''}, got {v}")
        out[key] = v
    hyps = regions.get("hyps")
    if hyps is not None:
        if not isinstance(hyps, dict) or set(hyps) != set(REGION_HYPS_KEYS):
            raise ValueError(f"regions hyps must be None or a dict with exactly the keys {REGION_HYPS_KEYS}")
        bins = hyps["bins"]
        if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or bins < 2 or bins > REGION_MAX_BINS or bins % 2:
            raise ValueError(f"regions hyps bins must be an even integer in [2, {REGION_MAX_BINS}], got {bins!r}")
        try:
            lo, hi = float(hyps["lo"]), float(hyps["hi"])
        except (TypeError, ValueError):
            raise ValueError("regions hyps lo and hi must be numbers") from None
        if not (np.isfinite(lo) and np.isfinite(hi) and hi > lo):
            raise ValueError(f"regions hyps needs finite lo < hi, got lo={lo}, hi={hi}")
        hyps = dict(lo=lo, hi=hi, bins=int(bins))
    out["hyps"] = hyps
    return out


def region_bits(masks):
    """[H, W] uint8 bit plane of the masks [K, H, W], K <= 8: bit k of a cell is set where masks[k] is (gsm_posterior_regions)."""
    m = np.asarray(masks) != 0
    if m.ndim != 3 or not 1 <= m.shape[0] <= REGION_MAX:
        raise ValueError(f"region_bits: masks must be [K, H, W] with 1 <= K <= {REGION_MAX}")
    bits = np.zeros(m.shape[1:], dtype=np.uint8)
    for k in range(m.shape[0]):
        bits |= m[k].astype(np.uint8) << np.uint8(k)
    return bits


def check_region_count(H, W, n_iter, burn_in, thin, split=True):
    """Refuse a hypsometry whose largest possible counter, H W cells x the snapshots of a chain that belong to a sequence, does not
    fit the int32 counters."""
    _, N, _ = sequence_plan(n_iter, burn_in, thin, split)
    total = int(H) * int(W) * N * (2 if split else 1)
    if total > HIST_MAX_COUNT:
        raise ValueError(f"regions hyps: {int(H) * int(W)} cells x {N * (2 if split else 1)} snapshots = {total} exceed the int32 counters "
                         f"({HIST_MAX_COUNT}): thin more")


def merge_regions(parts):
    """The per-chain region arrays of all ranks from the ranks' own, `parts` = [(func [c_r, K, T, 8], hyps [c_r, K, B + 2] or None),
    ...] in rank order: both are per chain, so they are concatenated along the chain axis in rank order (the order of the gathered
    traces and projections), never summed.  Returns (func [n_chains, K, T, 8] float64, hyps [n_chains, K, B + 2] int64 or None)."""
    parts = list(parts)
    if not parts:
        raise ValueError("merge_regions: no rank")
    func = [np.asarray(f, dtype=np.float64) for f, _ in parts]
    hyps = [h for _, h in parts]
    if any(f.ndim != 4 or f.shape[1:] != func[0].shape[1:] or f.shape[3] != 8 for f in func):
        raise ValueError(f"merge_regions: the ranks' func arrays must be [chains, K, T, 8] with the same K and T, got {[f.shape for f in func]}")
    if any((h is None) != (hyps[0] is None) for h in hyps):
        raise ValueError("merge_regions: some ranks hold a hypsometry and some do not")
    if hyps[0] is None:
        return np.concatenate(func, axis=0), None
    hyps = [np.asarray(h, dtype=np.int64) for h in hyps]
    if any(h.ndim != 3 or h.shape[1:] != hyps[0].shape[1:] or h.shape[0] != f.shape[0] or h.shape[1] != f.shape[1] for h, f in zip(hyps, func)):
        raise ValueError(f"merge_regions: the ranks' hyps arrays must be [chains, K, B + 2] beside their func, got {[h.shape for h in hyps]}")
    return np.concatenate(func, axis=0), np.concatenate(hyps, axis=0)


HIST_KEYS = ("bins", "half_width", "levels")
HIST_MAX_BINS, HIST_MAX_LEVELS = 128, 8
HIST_MAX_COUNT = 2 ** 31 - 1


def check_hist(hist):
    """Validate the `hist` option: None, or dict(bins=64, half_width=<metres, required>, levels=()).  Returns None or the dict
    with defaults filled in, bins an int, half_width a float and levels a tuple of floats."""
    if hist is None:
        return None
    if not isinstance(hist, dict):
        raise ValueError("hist must be None or a dict with the keys half_width and optionally bins, levels")
    unknown = set(hist) - set(HIST_KEYS)
    if unknown:
        raise ValueError(f"unknown hist option(s) {sorted(unknown)}; the options are {HIST_KEYS}")
    if "half_width" not in hist:
        raise ValueError("hist needs half_width: the histogram spans [g - half_width, g + half_width) metres about the common field")
    bins = hist.get("bins", 64)
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or bins < 2 or bins > HIST_MAX_BINS or bins % 2:
        raise ValueError(f"hist bins must be an even integer in [2, {HIST_MAX_BINS}], got {bins!r}")
    try:
        hw = float(hist["half_width"])
    except (TypeError, ValueError):
        raise ValueError(f"hist half_width must be a number > 0, got {hist['half_width']!r}") from None
    if not (hw > 0.0 and np.isfinite(hw)):
        raise ValueError(f"hist half_width must be finite and > 0, got {hw}")
    try:
        levels = tuple(float(v) for v in np.asarray(hist.get("levels", ()), dtype=np.float64).ravel())
    except (TypeError, ValueError):
        raise ValueError("hist levels must be a sequence of numbers") from None
    if len(levels) > HIST_MAX_LEVELS:
        raise ValueError(f"hist takes at most {HIST_MAX_LEVELS} levels, got {len(levels)}")
    if not all(np.isfinite(v) for v in levels):
        raise ValueError("hist levels must be finite")
    return dict(bins=int(bins), half_width=hw, levels=levels)


def check_hist_count(n_chains, n_iter, burn_in, thin, split=True):
    """Refuse a histogram whose per-cell total, n_chains (of all ranks) x the snapshots that belong to a sequence, does not fit
    the int32 counters."""
    _, N, _ = sequence_plan(n_iter, burn_in, thin, split)
    total = int(n_chains) * N * (2 if split else 1)
    if total > HIST_MAX_COUNT:
        raise ValueError(f"hist: {int(n_chains)} chains x {N * (2 if split else 1)} snapshots = {total} values per cell exceed the "
                         f"int32 counters ({HIST_MAX_COUNT}): thin more or use fewer chains")


def default_common_ref(initial_bed):
    """The template chain's initial bed with non-finite cells set to 0: the same on every rank because the template is."""
    g = np.array(initial_bed, dtype=np.float64)
    g[~np.isfinite(g)] = 0.0
    return g


class PosteriorAccumulator:
    """Running moments of eng.beds over the snapshot schedule of one run.  Owns the torch tensors: with rhat, `ref`
    [n_chains, H, W] in the state dtype (every chain's bed at the first snapshot of the sequence being filled) and 1 + split pairs of [n_chains, H, W] float64 sums (1 + 2 (1 + split) arrays of
    the beds' shape); without, one [H, W] pair.  Call add() when eng.beds holds the next snapshot of the schedule, then
    partials() (sum it over ranks) and finalize().  hist (see check_hist): also one int32 tensor `hist_counts` [(B + 3 + L), H, W],
    to which add() adds the histogram of every snapshot that belongs to a sequence (sum it over ranks with all_reduce_counts).
    ess (see check_ess): also `ring` [K, n_chains, H * W] in the state dtype, every chain's last K snapshots of the sequence being
    filled, and `lag_sqdiff` [K, H, W] float64, to which add() adds the squared differences at the lags 1 .. K (sum it over ranks
    with all_reduce_sum).  The ring is released with the last snapshot.
    cov (see check_cov): also, all float64, `d_probes` [K, H, W], `d_proj` [T, n_chains, K], the projections of all T snapshots, and
    `probe_cross` [K, H, W], to which add() adds the cross sums of every snapshot that belongs to a sequence (sum it over ranks
    with all_reduce_sum; gather d_proj over ranks like the sample traces).
    residual (see check_residual; needs eng.set_static): also, float64, `d_rg` [H, W], the residual of common_ref, and `residual_sums`
    [3 + L, H, W], to which add() adds the residual sums of every snapshot that belongs to a sequence (sum it over ranks with
    all_reduce_sum).
    local (see check_local): also, float64, `local_cross` [K, H, W], K = 2 reach^2 + 2 reach, to which add() adds the cross sums with
    the neighbours of every snapshot that belongs to a sequence (sum it over ranks with all_reduce_sum).
    regions (see check_regions; needs eng.set_static): also `d_region_bits` [H, W] uint8, `d_func` [T, n_chains, K, 8] float64, the
    region slots of all T snapshots, and with hyps `region_hyps` [n_chains, K, B + 2] int32, to which add() adds the hypsometry of
    every snapshot that belongs to a sequence.  Both are per chain: gather them over ranks in rank order (merge_regions)."""

    def __init__(self, eng, n_iter, burn_in, thin, split=True, rhat=True, common_ref=None, sample_cells=None, sample_loc=None, hist=None,
                 ess=None, cov=None, residual=None, local=None, regions=None):
        import torch
        self.eng = eng
        self.n_iter, self.burn_in, self.thin, self.split, self.rhat = int(n_iter), int(burn_in), int(thin), bool(split), bool(rhat)
        self.snapshot_iterations, self.N, self.dropped = sequence_plan(n_iter, burn_in, thin, self.split)
        self.T = int(self.snapshot_iterations.size)
        self.n_seq = 2 if self.split else 1
        H, W, n = eng.H, eng.W, eng.n_chains
        self.hist = check_hist(hist)
        if self.hist is not None:
            check_hist_count(n, n_iter, burn_in, thin, self.split)
            self.hist_inv_w = self.hist["bins"] / (2 * self.hist["half_width"])
            self.hist_slots = self.hist["bins"] + 3 + len(self.hist["levels"])
        self.ess = check_ess(ess, self.N, self.rhat)
        self.n_lags = 0 if self.ess is None else self.ess["max_lag"]
        self.cov = check_cov(cov, H, W)
        self.n_probes = 0 if self.cov is None else int(self.cov["probes"].shape[0])
        self.local = check_local(local)
        self.n_local = 0 if self.local is None else int(local_offsets(self.local["reach"]).shape[0])
        self.residual = check_residual(residual)
        if self.residual is not None and getattr(eng, "static", None) is None:
            raise ValueError("residual needs the engine's static fields: call set_static() first")
        self.regions = check_regions(regions, H, W)
        self.n_regions = 0 if self.regions is None else int(self.regions["masks"].shape[0])
        self.region_bins = 0
        if self.regions is not None:
            if getattr(eng, "static", None) is None:
                raise ValueError("regions needs the engine's static fields (the surface): call set_static() first")
            hy = self.regions["hyps"]
            if hy is not None:
                check_region_count(H, W, n_iter, burn_in, thin, self.split)
                self.region_bins = hy["bins"]
                self.region_hyps_lo, self.region_hyps_inv_w = hy["lo"], hy["bins"] / (hy["hi"] - hy["lo"])
            self.region_density_ratio = self.regions["rho_water"] / self.regions["rho_ice"]
        # common_ref None: a zero field (run_many passes default_common_ref(chain.initial_bed))
        g = np.zeros((H, W)) if common_ref is None else np.ascontiguousarray(common_ref, dtype=np.float64)
        if g.shape != (H, W) or not np.isfinite(g).all():
            raise ValueError(f"common_ref must be a finite array of shape {(H, W)}")
        self.common_ref = g
        cells = None if sample_cells is None else np.ascontiguousarray(sample_cells, dtype=np.int32).ravel()
        if cells is not None and ((cells < 0).any() or (cells >= H * W).any()):
            raise ValueError("sample cell outside the grid")
        self.sample_loc = None if sample_loc is None else np.asarray(sample_loc)
        self.n_samples = 0 if cells is None else int(cells.size)
        # the second sequence's sums start on a 16-byte boundary whatever n_chains * H * W is
        self.seq_stride = (n * H * W + 31) // 32 * 32
        # every device tensor this accumulator owns, (attribute, shape, dtype, zeroed): counted, then allocated, from this one list
        sd, f64 = eng.state_dtype, torch.float64
        sums = (self.n_seq, self.seq_stride) if self.rhat else (H, W)
        table = [("d_g", (H, W), f64, False), ("s1", sums, f64, True), ("s2", sums, f64, True)]
        if self.rhat:
            table += [("ref", (n, H, W), sd, False)]
        if self.n_samples:
            table += [("d_cells", (self.n_samples,), torch.int32, False), ("d_samples", (self.T, n, self.n_samples), f64, False)]
        if self.hist is not None:
            table += [("hist_counts", (self.hist_slots, H, W), torch.int32, True)]
        if self.n_lags:
            table += [("ring", (self.n_lags, n, H * W), sd, False), ("lag_sqdiff", (self.n_lags, H, W), f64, True)]
        if self.n_probes:
            table += [("d_probes", (self.n_probes, H, W), f64, False), ("d_proj", (self.T, n, self.n_probes), f64, False),
                      ("probe_cross", (self.n_probes, H, W), f64, True)]
        if self.residual is not None:
            table += [("d_rg", (H, W), f64, False), ("residual_sums", (3 + len(self.residual["levels"]), H, W), f64, True)]
        if self.n_local:
            table += [("local_cross", (self.n_local, H, W), f64, True)]
        if self.n_regions:
            table += [("d_region_bits", (H, W), torch.uint8, False), ("d_func", (self.T, n, self.n_regions, 8), f64, False)]
            if self.region_bins:
                table += [("region_hyps", (n, self.n_regions, self.region_bins + 2), torch.int32, True)]
        self.device_bytes = need = sum(math.prod(shape) * dtype.itemsize for _, shape, dtype, _ in table)
        free = torch.cuda.mem_get_info(eng.dev)[0]
        if need > free:
            raise MemoryError(f"the posterior accumulators need {need / 2**30:.2f} GiB ({n} chains x {H} x {W}, split={self.split}), "
                              f"{free / 2**30:.2f} GiB of device memory are free: use rhat=False (two [H, W] arrays) or fewer chains")
        self.ref = self.d_cells = self.d_samples = self.hist_counts = self.ring = self.lag_sqdiff = None
        self.d_probes = self.d_proj = self.probe_cross = self.d_rg = self.residual_sums = self.local_cross = None
        self.d_region_bits = self.d_func = self.region_hyps = None
        for name, shape, dtype, zeroed in table:
            setattr(self, name, (torch.zeros if zeroed else torch.empty)(shape, dtype=dtype, device=eng.dev))
        self.d_g.copy_(torch.as_tensor(g))
        if self.n_samples:
            self.d_cells.copy_(torch.as_tensor(cells))
        if self.n_probes:
            self.d_probes.copy_(torch.as_tensor(self.cov["probes"]))
        if self.residual is not None:
            st = eng.static
            rg = residual_field(g, st["surf"], st["velx"], st["vely"], st["dhdt"], st["smb"], st["resolution"])
            rg[~np.isfinite(rg)] = 0.0
            self.residual_ref = rg
            self.d_rg.copy_(torch.as_tensor(rg))
        if self.n_regions:
            self.d_region_bits.copy_(torch.as_tensor(region_bits(self.regions["masks"])))
        self.ring_head = self.ring_valid = 0
        self.n_added = 0
        self._partials = None

    @property
    def n_sequences(self):
        """Sequences this accumulator contributes to M."""
        return self.eng.n_chains * self.n_seq

    def add(self):
        """Fold eng.beds, which must hold the next snapshot of the schedule, into the sums (asynchronous)."""
        eng, t = self.eng, self.n_added
        if t >= self.T:
            raise RuntimeError(f"all {self.T} snapshots of the schedule were added already")
        if eng.beds is None:
            raise RuntimeError("set_state() first")
        smp = None if self.d_samples is None else self.d_samples[t]
        if t < self.dropped:
            if smp is not None:
                eng.posterior_sample(self.d_cells, smp)
        elif self.rhat:
            j = t - self.dropped
            k, first = j // self.N, j % self.N == 0
            if first and k > 0:            # the finished half becomes (mean - g, variance); ref then serves this half
                eng.posterior_close(self.ref, self.d_g, self.s1[k - 1], self.s2[k - 1], self.N)
            eng.posterior_accumulate(self.ref, self.s1[k], self.s2[k], first, self.d_cells, smp)
            if self.n_lags:
                if first:                  # no pair straddles two sequences
                    self.ring_valid = 0
                eng.posterior_lagged(self.ring, self.n_lags, self.ring_head, self.ring_valid, self.lag_sqdiff)
                self.ring_head = (self.ring_head + 1) % self.n_lags
                self.ring_valid = min(self.ring_valid + 1, self.n_lags)
                if t == self.T - 1:        # stream-ordered: the allocator reuses the block only behind the last call
                    self.ring = None
        else:
            eng.posterior_accumulate_pooled(self.d_g, self.s1, self.s2, self.d_cells, smp)
        if self.hist is not None and t >= self.dropped:      # the values that mean and sd describe, each counted once
            eng.posterior_histogram(self.d_g, self.hist_inv_w, self.hist["bins"], self.hist["levels"], self.hist_counts)
        if self.n_probes:                  # the projections of every snapshot, the cross sums of those that mean and sd describe
            eng.posterior_project(self.d_g, self.d_probes, self.d_proj[t])
            if t >= self.dropped:
                eng.posterior_cross(self.d_g, self.d_proj[t], self.n_probes, self.probe_cross)
        if self.residual is not None and t >= self.dropped:  # the states that mean and sd describe, each scored once
            eng.posterior_residual(self.d_rg, self.residual["levels"], self.residual_sums)
        if self.n_local and t >= self.dropped:               # the values that mean and sd describe, each paired once
            eng.posterior_local(self.d_g, self.local["reach"], self.local_cross)
        if self.n_regions:                 # the functionals of every snapshot, the hypsometry of those that mean and sd describe
            r, counted = self.regions, self.region_bins and t >= self.dropped
            if counted:
                eng.posterior_regions(self.d_region_bits, self.n_regions, r["sea_level"], self.region_density_ratio, self.d_func[t],
                                      self.region_hyps_lo, self.region_hyps_inv_w, self.region_bins, self.region_hyps)
            else:
                eng.posterior_regions(self.d_region_bits, self.n_regions, r["sea_level"], self.region_density_ratio, self.d_func[t])
        self.n_added += 1
        self._partials = None

    def _require_complete(self):
        if self.n_added != self.T:
            raise RuntimeError(f"{self.n_added} of {self.T} snapshots added")

    def partials(self):
        """[3, H, W] float64 device tensor of this handle's chains (see finalize); sums over ranks with all_reduce_posterior.
        Kept, so that it can be read after the engine is closed."""
        import torch
        self._require_complete()
        if self._partials is None:
            if self.rhat:
                self._partials = self.eng.posterior_partials(self.ref, self.d_g, self.s1, self.s2, self.n_seq, self.seq_stride,
                                                             self.n_seq - 1, self.N)
            else:
                self._partials = torch.stack([self.s1, self.s2, torch.zeros_like(self.s1)])
        return self._partials

    def local_sums(self):
        """Everything of this accumulator that adds over ranks, as device tensors under the names finalize() takes the sums by:
        partials_sum, the sequence count M (one int64) and, where the options ask for them, hist_counts, lag_sqdiff, probe_cross,
        residual_sums and local_cross."""
        import torch
        out = dict(partials_sum=self.partials(), M=torch.tensor([self.n_sequences], dtype=torch.int64, device=self.d_g.device))
        if self.hist is not None:
            out["hist_counts"] = self.hist_counts
        if self.n_lags:
            out["lag_sqdiff"] = self.lag_sqdiff
        if self.n_probes:
            out["probe_cross"] = self.probe_cross
        if self.residual is not None:
            out["residual_sums"] = self.residual_sums
        if self.n_local:
            out["local_cross"] = self.local_cross
        return out

    def sample_values(self):
        """[n_chains, n_points, T] numpy array of the traces, or None."""
        return None if self.d_samples is None else np.ascontiguousarray(self.d_samples.permute(1, 2, 0).cpu().numpy())

    def projections(self):
        """[n_chains, K, T] numpy array of the projections p of all snapshots, or None."""
        return None if self.d_proj is None else np.ascontiguousarray(self.d_proj.permute(1, 2, 0).cpu().numpy())

    def region_functionals(self):
        """[n_chains, K, T, 8] numpy array of the region slots of all snapshots, or None."""
        return None if self.d_func is None else np.ascontiguousarray(self.d_func.permute(1, 2, 0, 3).cpu().numpy())

    def region_hypsometry(self):
        """[n_chains, K, B + 2] int64 numpy array of the hypsometry counts, or None."""
        return None if self.region_hyps is None else self.region_hyps.cpu().numpy().astype(np.int64)

    def finalize(self, partials_sum=None, M=None, sample_values=None, hist_counts=None, lag_sqdiff=None, probe_cross=None, projections=None,
                 residual_sums=None, local_cross=None, region_func=None, region_hyps=None):
        """PosteriorSummary from the sums of local_sums() added over ranks (all_reduce_posterior, all_reduce_counts, all_reduce_sum);
        each defaults to this accumulator's own.  projections: [n_chains, K, T] of all ranks' chains (projections(), gathered);
        region_func and region_hyps: those of all ranks' chains (merge_regions of region_functionals(), region_hypsometry())."""
        self._require_complete()
        if partials_sum is None:
            partials_sum, M = self.partials(), self.n_sequences
        M = int(M)
        grid = self.common_ref.shape
        meta = {}
        if self.hist is not None:
            hc = _host_array(self.hist_counts if hist_counts is None else hist_counts, (self.hist_slots,) + grid, np.int64, "histogram counts")
            B = self.hist["bins"]
            meta = dict(hist_counts=hc[:B + 3].copy(), hist_half_width=self.hist["half_width"], hist_centre=self.common_ref.copy(),
                        level_values=np.asarray(self.hist["levels"], dtype=np.float64), level_counts=hc[B + 3:].copy())
        if self.n_lags:
            meta["lag_sqdiff"] = _host_array(self.lag_sqdiff if lag_sqdiff is None else lag_sqdiff, (self.n_lags,) + grid, np.float64, "lagged sums")
        if self.n_probes:
            P, g = self.cov["probes"], self.common_ref
            p = _host_array(self.projections() if projections is None else projections, (M // self.n_seq, self.n_probes, self.T), np.float64,
                            "projections")
            off = np.array([(w[w != 0] * g[w != 0]).sum() for w in P])           # Omega_k . g over the support
            meta.update(probes=P.copy(), probe_names=self.cov["names"], probe_values=off[None, :, None] + p, probe_centre=g.copy(),
                        probe_cross=_host_array(self.probe_cross if probe_cross is None else probe_cross, (self.n_probes,) + grid, np.float64,
                                                "cross sums"))
        if self.residual is not None:
            L = len(self.residual["levels"])
            st = self.eng.static
            meta.update(residual_sums=_host_array(self.residual_sums if residual_sums is None else residual_sums, (3 + L,) + grid, np.float64,
                                                  "residual sums"),
                        residual_ref=self.residual_ref.copy(), residual_levels=np.asarray(self.residual["levels"], dtype=np.float64),
                        residual_sigma_mc=st["sigma_mc"], residual_mc_mask=np.array(st["mc_mask"], dtype=bool))
        if self.n_local:
            meta.update(local_cross=_host_array(self.local_cross if local_cross is None else local_cross, (self.n_local,) + grid, np.float64,
                                                "local cross sums"),
                        local_reach=self.local["reach"], local_centre=self.common_ref.copy())
        if self.n_regions:
            C, K, r = M // self.n_seq, self.n_regions, self.regions
            meta.update(region_func=_host_array(self.region_functionals() if region_func is None else region_func, (C, K, self.T, 8), np.float64,
                                                "region functionals"),
                        region_masks=r["masks"].copy(), region_names=r["names"], region_sea_level=r["sea_level"],
                        region_density_ratio=self.region_density_ratio, region_resolution=float(self.eng.static["resolution"]))
            if self.region_bins:
                meta.update(region_hyps=_host_array(self.region_hypsometry() if region_hyps is None else region_hyps, (C, K, self.region_bins + 2),
                                                    np.int64, "hypsometry counts"),
                            region_hyps_range=np.array([r["hyps"]["lo"], r["hyps"]["hi"]], dtype=np.float64))
        return finalize(partials_sum, M, self.N, self.common_ref, rhat=self.rhat, n_chains=M // self.n_seq,
                        snapshot_iterations=self.snapshot_iterations, burn_in=self.burn_in, thin=self.thin, split=self.split,
                        sample_values=self.sample_values() if sample_values is None else sample_values, sample_loc=self.sample_loc, **meta)


POSTERIOR_KEYS = ("burn_in", "thin", "split", "rhat", "common_ref", "hist", "ess", "cov", "residual", "local", "regions")


def check_options(posterior, n_iter, n_chains=None):
    """Validate the `posterior=` dict of run_many / largeScaleChain_mp before anything runs; returns it with defaults filled in.
    n_chains: the chains of all ranks, for the histogram's count limit."""
    if not isinstance(posterior, dict):
        raise TypeError("posterior must be a dict with the keys burn_in, thin and optionally split, rhat, common_ref, hist, ess, cov, residual, local, regions")
    unknown = set(posterior) - set(POSTERIOR_KEYS)
    if unknown:
        raise ValueError(f"unknown posterior option(s) {sorted(unknown)}; the options are {POSTERIOR_KEYS}")
    opt = dict(burn_in=0, thin=1, split=True, rhat=True, common_ref=None, hist=None, ess=None, cov=None, residual=None, local=None, regions=None)
    opt.update(posterior)
    _, N, _ = sequence_plan(n_iter, opt["burn_in"], opt["thin"], opt["split"])
    opt["ess"] = check_ess(opt["ess"], N, opt["rhat"])
    opt["hist"] = check_hist(opt["hist"])
    opt["cov"] = check_cov(opt["cov"])
    opt["residual"] = check_residual(opt["residual"])
    opt["local"] = check_local(opt["local"])
    opt["regions"] = check_regions(opt["regions"])
    if opt["hist"] is not None and n_chains is not None:
        check_hist_count(n_chains, n_iter, opt["burn_in"], opt["thin"], opt["split"])
    return opt
