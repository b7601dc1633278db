"""GsmEngine: owns one libgsm_hip handle and the torch device tensors of a shard of chains.

PyTorch is plumbing here -- device memory, streams and (in parallel.py) torch.distributed.  All compute
is in the HIP library behind the C ABI of include/gsm.h.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from ._lib import GsmError, RfParams, MODEL_IDS


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def binary_mask(mask, name):
    """Masks of this path are 0/1 (bool or numeric).  The reference mixes `mask == 1` and truthiness
    tests (MCMC.py:1257, :1288, :1328); they agree only for 0/1 masks, so anything else is refused."""
    m = np.asarray(mask)
    if m.dtype != bool:
        if np.isnan(m.astype(float)).any() or not np.isin(m, (0, 1)).all():
            raise ValueError(f"{name} must contain only 0/1 (or bool) values")
    return np.ascontiguousarray(m.astype(np.uint8))


class GsmEngine:
    def __init__(self, H: int, W: int, n_chains: int, device: int | None = None, state_dtype="f64"):
        if not torch.cuda.is_available():
            raise RuntimeError("no ROCm/HIP device visible to torch: the sampler has no CPU fallback")
        self.lib = _lib.load()
        self.H, self.W, self.n_chains = int(H), int(W), int(n_chains)
        self.device_index = torch.cuda.current_device() if device is None else int(device)
        self.dev = torch.device("cuda", self.device_index)
        h = C.c_void_p()
        if state_dtype not in ("f64", "f32"):
            raise ValueError("state_dtype must be 'f64' or 'f32'")
        self.state_dtype = torch.float64 if state_dtype == "f64" else torch.float32
        rc = self.lib.gsm_create(C.byref(h), self.H, self.W, self.n_chains, 0 if state_dtype == "f64" else 1,
                                 self.device_index)
        if rc != 0:
            raise GsmError(rc, self.lib.gsm_last_error(None).decode())
        self.h = h
        for name, value in _lib.options_from_env(os.environ).items():      # GSM_STRIP, GSM_SPLIT2, GSM_FUSED_SEGMENT: read here, per handle
            self.set_option(name, value)
        self.beds = self.energy = self.resampled = self.loss_sum = self.static = None
        self.field_stride = 0
        self.n_sizes = 0

    # ------------------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "h", None):
            self.lib.gsm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise GsmError(rc, self.lib.gsm_last_error(self.h).decode())

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def _f64(self, a):
        return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(self.dev)

    def mask_u8(self, mask):
        """Device uint8 copy of a 0/1 mask: 1 where mask == 1."""
        return torch.as_tensor(np.ascontiguousarray(np.asarray(mask) == 1, dtype=np.uint8)).to(self.dev)

    def call(self, fn, *args, stream=None):
        """fn(handle, *args, stream) under the device guard, its return code checked.  Tensors become pointers (None is ctypes'
        NULL already); `stream` is a torch stream (default: the current one)."""
        args = [_ptr(a) if isinstance(a, torch.Tensor) else a for a in args]
        st = self._stream() if stream is None else C.c_void_p(stream.cuda_stream)
        with torch.cuda.device(self.dev):
            self._check(fn(self.h, *args, st))

    # ------------------------------------------------------------------------------------------
    def set_static(self, surf, velx, vely, dhdt, smb, crf_weight, update_mask, mc_mask, resolution, sigma_mc):
        shp = (self.H, self.W)
        arrs = []
        for a in (surf, velx, vely, dhdt, smb):
            a = np.asarray(a)
            if a.shape != shp:
                raise ValueError(f"static field of shape {a.shape}, grid is {shp}")
            arrs.append(self._f64(a))
        w = None
        if crf_weight is not None:
            if np.asarray(crf_weight).shape != shp:
                raise ValueError("crf_data_weight has the wrong shape")
            w = self._f64(crf_weight)
        um = torch.as_tensor(binary_mask(update_mask, "update mask")).to(self.dev)
        mm = torch.as_tensor(binary_mask(mc_mask, "mc_region_mask")).to(self.dev)
        if um.shape != shp or mm.shape != shp:
            raise ValueError("mask has the wrong shape")
        self.call(self.lib.gsm_set_static, *arrs, w, um, mm, float(resolution), float(sigma_mc))
        # host copies of what the residual and the loss are made of (posterior.PosteriorAccumulator, `residual`)
        self.static = dict(zip(("surf", "velx", "vely", "dhdt", "smb"), (np.array(a, dtype=np.float64) for a in (surf, velx, vely, dhdt, smb))),
                           mc_mask=np.asarray(mc_mask) == 1, resolution=float(resolution), sigma_mc=float(sigma_mc))

    def set_blocks(self, pairs, edge_masks=None):
        """pairs: (2, n) int array, row 0 widths, row 1 heights (RandField.pairs, MCMC.py:576-579)."""
        pairs = np.asarray(pairs)
        n = pairs.shape[1]
        bw = (C.c_int32 * n)(*[int(v) for v in pairs[0]])
        bh = (C.c_int32 * n)(*[int(v) for v in pairs[1]])
        packed = offs = None
        if edge_masks is not None:
            o, chunks, tot = [], [], 0
            for i in range(n):
                m = np.ascontiguousarray(edge_masks[i], dtype=np.float64)
                if m.shape != (int(pairs[1, i]), int(pairs[0, i])):
                    raise ValueError("edge mask shape does not match its block size")
                o.append(tot)
                chunks.append(m.ravel())
                tot += m.size
            packed = self._f64(np.concatenate(chunks))
            offs = (C.c_int64 * n)(*o)
        self.call(self.lib.gsm_set_blocks, n, bh, bw, packed, offs)
        self.bh = np.array(pairs[1], dtype=np.int64)
        self.bw = np.array(pairs[0], dtype=np.int64)
        self.n_sizes = n
        self.field_stride = int(self.bh.max() * self.bw.max())

    def set_centres(self, region_mask):
        cells = np.flatnonzero(np.asarray(region_mask).ravel() == 1).astype(np.int32)
        if cells.size == 0:
            raise ValueError("region_mask has no cell equal to 1")
        t = torch.as_tensor(cells).to(self.dev)
        self.call(self.lib.gsm_set_centres, t, int(cells.size))

    def set_state(self, beds, resampled=None):
        """beds: (n_chains, H, W) array or cuda tensor.  Returns loss_cache[0] per chain (numpy)."""
        if isinstance(beds, torch.Tensor):
            b = beds.to(device=self.dev, dtype=self.state_dtype).contiguous()
            if b.data_ptr() == beds.data_ptr():
                b = b.clone()          # the engine updates its state in place: never alias the caller's tensor
        else:
            b = self._f64(beds).to(self.state_dtype)
        if tuple(b.shape) != (self.n_chains, self.H, self.W):
            raise ValueError(f"beds must have shape {(self.n_chains, self.H, self.W)}, got {tuple(b.shape)}")
        self.beds = b
        if resampled is None:
            self.resampled = torch.zeros((self.n_chains, self.H, self.W), dtype=torch.int32, device=self.dev)
        else:
            self.resampled = torch.as_tensor(resampled).to(device=self.dev, dtype=torch.int32).contiguous()
        self.loss_sum = torch.zeros((self.n_chains, 2), dtype=torch.float64, device=self.dev)
        self.energy = torch.empty((self.n_chains, self.H, self.W), dtype=self.state_dtype, device=self.dev)
        loss0 = torch.zeros(self.n_chains, dtype=torch.float64, device=self.dev)
        self.call(self.lib.gsm_init_loss, self.beds, self.energy, self.loss_sum, loss0)
        return loss0.cpu().numpy()

    def min_dist_from_mask(self, xx, yy, mask):
        """Distance of every cell to the nearest masked cell on the device (Utilities.py:21-24)."""
        m = np.ascontiguousarray(np.asarray(mask) != 0).astype(np.uint8)
        if m.shape != (self.H, self.W):
            raise ValueError("mask has the wrong shape")
        dx, dy, dm = self._f64(xx), self._f64(yy), torch.as_tensor(m).to(self.dev)
        out = torch.empty((self.H, self.W), dtype=torch.float64, device=self.dev)
        self.call(self.lib.gsm_min_dist_from_mask, dx, dy, dm, out)
        return out.cpu().numpy()

    def gaussian_filter(self, fields, w0, w1):
        """gsm_gaussian_filter of a stack [n, H, W] (array or device tensor) with the two axes' weights (host arrays of odd
        length); returns a device tensor."""
        x = fields.to(device=self.dev, dtype=torch.float64).contiguous() if isinstance(fields, torch.Tensor) else self._f64(fields)
        if x.dim() != 3 or tuple(x.shape[1:]) != (self.H, self.W) or x.shape[0] < 1:
            raise ValueError(f"fields must have shape (n, {self.H}, {self.W})")
        w0, w1 = (np.ascontiguousarray(w, dtype=np.float64) for w in (w0, w1))
        if w0.ndim != 1 or w1.ndim != 1 or w0.size % 2 != 1 or w1.size % 2 != 1:
            raise ValueError("the weights of an axis are a 1-D array of odd length")
        out = torch.empty_like(x)
        dp = C.POINTER(C.c_double)
        self.call(self.lib.gsm_gaussian_filter, x, out, int(x.shape[0]), self.H, self.W, w0.ctypes.data_as(dp), w0.size // 2,
                  w1.ctypes.data_as(dp), w1.size // 2)
        return out

    def qt_fit(self, fields, q, want_sorted=False):
        """gsm_qt_fit of n fields [n, cells] (array or device tensor; `cells` need not be the handle's H * W) at the probabilities q
        (host array, ascending in [0, 1]).  Returns device tensors (quantiles [n, nq], n_valid [n] int64, n_inf [n] int64, sorted
        [n, cells] or None)."""
        x = fields.to(device=self.dev, dtype=torch.float64).contiguous() if isinstance(fields, torch.Tensor) else self._f64(fields)
        if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
            raise ValueError("fields must have shape (n, cells)")
        q = np.ascontiguousarray(q, dtype=np.float64)
        if q.ndim != 1:
            raise ValueError("q is a 1-D array")
        n, cells = int(x.shape[0]), int(x.shape[1])
        quantiles = torch.empty((n, q.size), dtype=torch.float64, device=self.dev)
        n_valid = torch.empty(n, dtype=torch.int64, device=self.dev)
        n_inf = torch.empty(n, dtype=torch.int64, device=self.dev)
        srt = torch.empty_like(x) if want_sorted else None
        self.call(self.lib.gsm_qt_fit, x, n, cells, q.ctypes.data_as(C.POINTER(C.c_double)), int(q.size), quantiles, n_valid, n_inf, srt)
        return quantiles, n_valid, n_inf, srt

    def residual(self, beds):
        b = beds.to(device=self.dev, dtype=torch.float64).contiguous() if isinstance(beds, torch.Tensor) else self._f64(beds)
        if tuple(b.shape) != (self.n_chains, self.H, self.W):
            raise ValueError("beds has the wrong shape")
        out = torch.empty_like(b)
        self.call(self.lib.gsm_residual, b, out)
        return out

    # ---- posterior accumulator (gsm_posterior_*; mcmc_gpu_amd/posterior.py owns the tensors) ------------------------------
    def _sample_args(self, sample_cells, sample_out):
        if sample_out is None:
            return None, 0, None
        if sample_cells is None or sample_cells.dtype != torch.int32 or sample_out.dtype != torch.float64 or \
                sample_out.numel() != self.n_chains * sample_cells.numel() or not sample_out.is_contiguous():
            raise ValueError("sample_cells must be an int32 device tensor and sample_out a contiguous float64 one of n_chains x n_samples")
        return sample_cells, int(sample_cells.numel()), sample_out

    def _need_beds(self):
        if self.beds is None:
            raise RuntimeError("set_state() first")

    def _check_state(self, name, t, k=1):
        if t.dtype != self.state_dtype or t.numel() != k * self.n_chains * self.H * self.W or not t.is_contiguous() or t.device != self.dev:
            raise ValueError(f"{name} must be a contiguous tensor of {k} x the beds' shape and dtype on {self.dev}")

    def _check_sums(self, n, **tensors):
        for name, t in tensors.items():
            if t.dtype != torch.float64 or t.numel() < n or not t.is_contiguous() or t.device != self.dev:
                raise ValueError(f"{name} must be a contiguous float64 tensor of at least {n} elements on {self.dev}")

    def posterior_accumulate(self, ref, s1, s2, first, sample_cells=None, sample_out=None):
        """One snapshot of self.beds into the per-chain sums of one sequence: d = bed - ref, s1 += d, s2 += d * d (first: ref = bed is
        written and the sums are set).  ref [n_chains, H, W] in the state dtype, s1 / s2 float64 of the same size.  Asynchronous."""
        self._need_beds()
        self._check_state("ref", ref)
        self._check_sums(self.n_chains * self.H * self.W, s1=s1, s2=s2)
        self.call(self.lib.gsm_posterior_accumulate, self.beds, ref, s1, s2, 1 if first else 0, *self._sample_args(sample_cells, sample_out))

    def posterior_accumulate_pooled(self, g, s1, s2, sample_cells=None, sample_out=None):
        """One snapshot of self.beds into sums over all chains: S1 += sum_c d, S2 += sum_c d * d, d = bed_c - g; g, s1, s2 [H, W] float64."""
        self._need_beds()
        self._check_sums(self.H * self.W, g=g, s1=s1, s2=s2)
        self.call(self.lib.gsm_posterior_accumulate_pooled, self.beds, g, s1, s2, *self._sample_args(sample_cells, sample_out))

    def posterior_sample(self, sample_cells, sample_out):
        """sample_out[c, p] = self.beds[c] at flat cell sample_cells[p]."""
        self._need_beds()
        self.call(self.lib.gsm_posterior_sample, self.beds, *self._sample_args(sample_cells, sample_out))

    def posterior_close(self, ref, g, s1, s2, n_per_seq):
        """A finished sequence's sums become, in place, s1 = its mean minus g and s2 = its ddof=1 variance; `ref` is then free for
        the chains' next sequence (posterior_accumulate with first=True)."""
        self._check_sums(self.H * self.W, g=g)
        self._check_sums(self.n_chains * self.H * self.W, s1=s1, s2=s2)
        self._check_state("ref", ref)
        self.call(self.lib.gsm_posterior_close, ref, g, s1, s2, int(n_per_seq))

    def posterior_partials(self, ref, g, s1, s2, n_seq_per_chain, seq_stride, n_closed, n_per_seq):
        """[3, H, W] device tensor (sum of sequence means minus g, of their squares, of sequence variances) over this handle's
        n_chains * n_seq_per_chain sequences of n_per_seq snapshots; sequence k's sums start at s1.view(-1)[k * seq_stride]; the
        first n_closed sequences of every chain were closed (posterior_close), `ref` belongs to the others."""
        n = self.n_chains * self.H * self.W
        self._check_sums(self.H * self.W, g=g)
        self._check_sums((int(n_seq_per_chain) - 1) * int(seq_stride) + n if n_seq_per_chain in (1, 2) else n, s1=s1, s2=s2)
        self._check_state("ref", ref)
        out = torch.empty((3, self.H, self.W), dtype=torch.float64, device=self.dev)
        self.call(self.lib.gsm_posterior_partials, ref, g, s1, s2, int(n_seq_per_chain), int(seq_stride), int(n_closed), int(n_per_seq), out)
        return out

    def posterior_histogram(self, g, inv_width, n_bins, levels, counts):
        """One snapshot of self.beds ADDED to the per-cell counts [(n_bins + 3 + L), H, W] int32: slot 0 underflow, 1 .. n_bins the
        bins of floor((bed - g) * inv_width) + n_bins / 2, n_bins + 1 overflow, n_bins + 2 NaN, then one slot per level counting
        bed < level.  g [H, W] float64 on the device, levels a host sequence of L <= 8 floats.  Asynchronous."""
        self._need_beds()
        self._check_sums(self.H * self.W, g=g)
        lv = np.ascontiguousarray(levels, dtype=np.float64).ravel()
        n = (int(n_bins) + 3 + lv.size) * self.H * self.W
        if counts.dtype != torch.int32 or counts.numel() != n or not counts.is_contiguous() or counts.device != self.dev:
            raise ValueError(f"counts must be a contiguous int32 tensor of {n} elements on {self.dev}")
        self.call(self.lib.gsm_posterior_histogram, self.beds, g, float(inv_width), int(n_bins), lv.ctypes.data if lv.size else None,
                  int(lv.size), counts)

    def posterior_lagged(self, ring, n_lags, head, n_valid, lag_sqdiff):
        """One snapshot of self.beds into the per-cell sums of squared differences at the lags 1 .. n_lags over all chains:
        lag_sqdiff[t - 1] += sum_c (bed_c - ring[(head - t) % n_lags, c]) ** 2 for t = 1 .. n_valid, then ring[head] = beds.  ring
        [n_lags, n_chains, H * W] in the state dtype, lag_sqdiff [n_lags, H, W] float64; the caller advances head and n_valid
        (n_valid = 0 starts a sequence).  Asynchronous."""
        self._need_beds()
        n_lags = int(n_lags)
        self._check_state("ring", ring, n_lags)
        if lag_sqdiff.numel() != n_lags * self.H * self.W:
            raise ValueError(f"lag_sqdiff must hold n_lags x H x W = {n_lags * self.H * self.W} elements")
        self._check_sums(n_lags * self.H * self.W, lag_sqdiff=lag_sqdiff)
        self.call(self.lib.gsm_posterior_lagged, self.beds, ring, n_lags, int(head), int(n_valid), lag_sqdiff)

    def _probe_count(self, n_probes):
        n_probes = int(n_probes)
        if not 1 <= n_probes <= 15:
            raise ValueError(f"n_probes must be in [1, 15], got {n_probes}")
        return n_probes

    def posterior_project(self, g, probes, out):
        """One snapshot of self.beds projected onto the K <= 15 weight fields probes [K, H, W] float64: out[c, k] = sum over the
        cells with probes[k] != 0 of probes[k] * (bed_c - g); out [n_chains, K] float64 is written.  g [H, W] float64.  Asynchronous."""
        self._need_beds()
        self._check_sums(self.H * self.W, g=g)
        if probes.dim() != 3 or tuple(probes.shape[1:]) != (self.H, self.W):
            raise ValueError(f"probes must have shape [K, {self.H}, {self.W}], got {tuple(probes.shape)}")
        K = self._probe_count(probes.shape[0])
        self._check_sums(K * self.H * self.W, probes=probes)
        if out.numel() != self.n_chains * K:
            raise ValueError(f"out must hold n_chains x K = {self.n_chains * K} elements")
        self._check_sums(self.n_chains * K, out=out)
        self.call(self.lib.gsm_posterior_project, self.beds, g, probes, K, out)

    def posterior_cross(self, g, proj, n_probes, cross):
        """One snapshot of self.beds into the per-cell cross sums with the projections proj [n_chains, K] float64 of the same
        snapshot (posterior_project): cross[k] += sum_c (bed_c - g) * proj[c, k]; cross [K, H, W] float64.  Asynchronous."""
        self._need_beds()
        K = self._probe_count(n_probes)
        self._check_sums(self.H * self.W, g=g)
        if proj.numel() != self.n_chains * K or cross.numel() != K * self.H * self.W:
            raise ValueError(f"proj must hold n_chains x K = {self.n_chains * K} elements and cross K x H x W = {K * self.H * self.W}")
        self._check_sums(self.n_chains * K, proj=proj)
        self._check_sums(K * self.H * self.W, cross=cross)
        self.call(self.lib.gsm_posterior_cross, self.beds, g, proj, K, cross)

    def posterior_residual(self, rg, levels, sums):
        """One snapshot of self.beds into the per-cell sums of the mass-conservation residual r over all chains (set_static's fields;
        gsm_residual's bits): over the chains with finite r, sums[0] += their number, sums[1] += sum d, sums[2] += sum d * d with d =
        r - rg, sums[3 + l] += the number with |r| > levels[l].  rg [H, W] and sums [3 + L, H, W] float64 on the device, levels a
        host sequence of L <= 4 finite floats >= 0.  Asynchronous."""
        self._need_beds()
        if self.static is None:
            raise RuntimeError("set_static() first")
        lv = np.ascontiguousarray(levels, dtype=np.float64).ravel()
        if lv.size > 4 or not (np.isfinite(lv).all() and (lv >= 0).all()):
            raise ValueError(f"levels must be at most 4 finite values >= 0, got {lv.tolist()}")
        n = (3 + lv.size) * self.H * self.W
        if rg.numel() != self.H * self.W or sums.numel() != n:
            raise ValueError(f"rg must hold H x W = {self.H * self.W} elements and sums (3 + L) x H x W = {n}")
        self._check_sums(self.H * self.W, rg=rg)
        self._check_sums(n, sums=sums)
        self.call(self.lib.gsm_posterior_residual, self.beds, rg, lv.ctypes.data if lv.size else None, int(lv.size), sums)

    def posterior_local(self, g, reach, cross):
        """One snapshot of self.beds into the per-cell cross sums with the neighbours within `reach` (1 .. 4): cross[k] += sum_c d_c *
        d_c shifted by offset k of posterior.local_offsets(reach), d_c = bed_c - g, where the partner lies inside the grid (the other
        entries are not touched).  g [H, W] and cross [K, H, W] float64 on the device, K = 2 reach^2 + 2 reach.  Asynchronous."""
        self._need_beds()
        if isinstance(reach, bool) or not isinstance(reach, (int, np.integer)) or not 1 <= reach <= 4:
            raise ValueError(f"reach must be an integer in [1, 4], got {reach!r}")
        K = 2 * int(reach) * int(reach) + 2 * int(reach)
        if g.numel() != self.H * self.W or cross.numel() != K * self.H * self.W:
            raise ValueError(f"g must hold H x W = {self.H * self.W} elements and cross K x H x W = {K * self.H * self.W}")
        self._check_sums(self.H * self.W, g=g)
        self._check_sums(K * self.H * self.W, cross=cross)
        self.call(self.lib.gsm_posterior_local, self.beds, g, int(reach), cross)

    def posterior_regions(self, region_bits, n_regions, sea_level, density_ratio, func, hyps_lo=0.0, hyps_inv_width=0.0, n_bins=0, hyps=None):
        """One snapshot of self.beds into the per-chain, per-region functionals func [n_chains, K, 8] float64 (written): over the cells
        of region k (bit k of region_bits [H, W] uint8) whose bed x and set_static surf s are finite, 0 their number, 1 sum x, 2 sum
        max(s - x, 0), 3 sum max((s - x) + density_ratio * min(x - sea_level, 0), 0), 4 the number with x < sea_level, 5 the number of
        those with slot 3's term > 0, 6 min x, 7 max x.  With n_bins > 0 (even, <= 64) the hypsometry of the same cells is ADDED to hyps
        [n_chains, K, n_bins + 2] int32: slot 0 below hyps_lo, then n_bins bins of width 1 / hyps_inv_width, then the overflow.
        Asynchronous."""
        self._need_beds()
        if self.static is None:
            raise RuntimeError("set_static() first")
        K, B = int(n_regions), int(n_bins)
        if not 1 <= K <= 8:
            raise ValueError(f"n_regions must be in [1, 8], got {K}")
        if B != 0 and (B < 2 or B > 64 or B % 2):
            raise ValueError(f"n_bins must be 0 or an even integer in [2, 64], got {B}")
        if not np.isfinite(sea_level) or not (np.isfinite(density_ratio) and density_ratio > 0):
            raise ValueError("sea_level must be finite and density_ratio finite and > 0")
        if region_bits.dtype != torch.uint8 or region_bits.numel() != self.H * self.W or not region_bits.is_contiguous() or region_bits.device != self.dev:
            raise ValueError(f"region_bits must be a contiguous uint8 tensor of H x W = {self.H * self.W} elements on {self.dev}")
        if func.numel() != self.n_chains * K * 8:
            raise ValueError(f"func must hold n_chains x K x 8 = {self.n_chains * K * 8} elements")
        self._check_sums(self.n_chains * K * 8, func=func)
        if B:
            if not (np.isfinite(hyps_lo) and np.isfinite(hyps_inv_width) and hyps_inv_width > 0):
                raise ValueError("hyps_lo must be finite and hyps_inv_width finite and > 0")
            n = self.n_chains * K * (B + 2)
            if hyps is None or hyps.dtype != torch.int32 or hyps.numel() != n or not hyps.is_contiguous() or hyps.device != self.dev:
                raise ValueError(f"hyps must be a contiguous int32 tensor of n_chains x K x (n_bins + 2) = {n} elements on {self.dev}")
        self.call(self.lib.gsm_posterior_regions, self.beds, region_bits, K, float(sea_level), float(density_ratio), func, float(hyps_lo),
                  float(hyps_inv_width), B, hyps if B else None)

    # ------------------------------------------------------------------------------------------
    def pack_fields(self, fields):
        """fields[c][s] = masked proposal (bh, bw) -> (n_chains, n_steps, field_stride) float64."""
        n_steps = len(fields[0])
        out = np.zeros((self.n_chains, n_steps, self.field_stride))
        for c in range(self.n_chains):
            for s in range(n_steps):
                f = np.asarray(fields[c][s], dtype=np.float64)
                out[c, s, :f.size] = f.ravel()
        return out

    def run_replay(self, size_idx, centre, u, fields_packed):
        """size_idx (n_chains, n_steps) int, centre (n_chains, n_steps, 2) int, u (n_chains, n_steps),
        fields_packed (n_chains, n_steps, field_stride).  Returns (loss, accept) as numpy arrays."""
        size_idx = np.ascontiguousarray(size_idx, dtype=np.int32)
        n_steps = size_idx.shape[1]
        centre = np.ascontiguousarray(centre, dtype=np.int32)
        u = np.ascontiguousarray(u, dtype=np.float64)
        if size_idx.shape != (self.n_chains, n_steps) or centre.shape != (self.n_chains, n_steps, 2) or \
                u.shape != (self.n_chains, n_steps):
            raise ValueError("replay arrays have inconsistent shapes")
        if (size_idx < 0).any() or (size_idx >= self.n_sizes).any():
            raise ValueError("size_idx out of range")
        if (centre < 0).any() or (centre[..., 0] >= self.H).any() or (centre[..., 1] >= self.W).any():
            raise ValueError("block centre outside the grid")
        if isinstance(fields_packed, torch.Tensor):
            f = fields_packed.to(device=self.dev, dtype=torch.float64).contiguous()
        else:
            f = self._f64(fields_packed)
        if tuple(f.shape) != (self.n_chains, n_steps, self.field_stride):
            raise ValueError("fields_packed has the wrong shape")
        self._need_beds()
        d_si = torch.as_tensor(size_idx).to(self.dev)
        d_c = torch.as_tensor(centre).to(self.dev)
        d_u = torch.as_tensor(u).to(self.dev)
        loss = torch.empty((self.n_chains, n_steps), dtype=torch.float64, device=self.dev)
        acc = torch.empty((self.n_chains, n_steps), dtype=torch.uint8, device=self.dev)
        self.call(self.lib.gsm_run_replay, n_steps, self.beds, self.energy, self.resampled, self.loss_sum, d_si, d_c, d_u, f, self.field_stride,
                  loss, acc)
        return loss.cpu().numpy(), acc.cpu().numpy()

    # ------------------------------------------------------------------------------------------
    @staticmethod
    def rf_struct(rf, resolution=None) -> RfParams:
        """RfParams from any object with the RandField attributes (MCMC.py:497-510)."""
        p = RfParams()
        p.range_min_x, p.range_max_x = float(rf.range_min_x), float(rf.range_max_x)
        p.range_min_y, p.range_max_y = float(rf.range_min_y), float(rf.range_max_y)
        p.scale_min, p.scale_max = float(rf.scale_min), float(rf.scale_max)
        p.nugget_max = float(rf.nugget_max)
        p.smoothness = float(rf.smoothness) if rf.smoothness else 0.0
        p.resolution = float(resolution if resolution is not None else rf.resolution)
        p.model = MODEL_IDS[rf.model_name]
        p.isotropic = 1 if rf.isotropic else 0
        p.generator = 1 if getattr(rf, "generator", "spectral") == "cholesky" else 0
        return p

    def _seeds(self, seeds):
        s = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64))
        if s.shape != (self.n_chains,):
            raise ValueError("need one seed per chain")
        return torch.as_tensor(s.view(np.int64)).to(self.dev)

    def propose_philox(self, n_steps, step0, seeds, rf, want_scalars=True):
        d_seeds = self._seeds(seeds)
        n = self.n_chains * n_steps
        si = torch.empty(n, dtype=torch.int32, device=self.dev)
        ce = torch.empty(n * 2, dtype=torch.int32, device=self.dev)
        u = torch.empty(n, dtype=torch.float64, device=self.dev)
        fl = torch.zeros((self.n_chains, n_steps, self.field_stride), dtype=torch.float64, device=self.dev)
        sc = torch.empty(n * 4, dtype=torch.float64, device=self.dev) if want_scalars else None
        p = rf if isinstance(rf, RfParams) else self.rf_struct(rf)
        self.call(self.lib.gsm_propose_philox, int(n_steps), int(step0), d_seeds, C.byref(p), si, ce, u, fl, self.field_stride, sc)
        torch.cuda.synchronize(self.dev)
        return dict(size_idx=si.view(self.n_chains, n_steps), centre=ce.view(self.n_chains, n_steps, 2),
                    u=u.view(self.n_chains, n_steps), fields=fl,
                    rf_scalars=None if sc is None else sc.view(self.n_chains, n_steps, 4))

    def spectral_from_noise(self, size_idx, rf_scalars, rf, noise_re, noise_im, nugget_fields=None):
        """The device spectral synthesis on caller-supplied white noise (gsm_spectral_from_noise): for field r,
        size_idx[r] picks the block shape, rf_scalars[r] = (scale, nugget, range_x, range_y) as drawn at
        MCMC.py:200-207 (scale already / 3), noise_re[r] / noise_im[r] are the two (bh, bw) normal planes of MCMC.py:242,
        nugget_fields[r] the rng.normal(0, sqrt(nug)) plane of MCMC.py:251 (or None).  Returns the masked fields, a list
        of (bh, bw) arrays."""
        size_idx = np.ascontiguousarray(size_idx, dtype=np.int32)
        n = size_idx.shape[0]
        sc = np.ascontiguousarray(rf_scalars, dtype=np.float64)
        if sc.shape != (n, 4):
            raise ValueError("rf_scalars must have shape (n, 4)")

        def pack(planes):
            out = np.zeros((n, self.field_stride))
            for r, a in enumerate(planes):
                a = np.asarray(a, dtype=np.float64)
                if a.shape != (int(self.bh[size_idx[r]]), int(self.bw[size_idx[r]])):
                    raise ValueError("noise plane shape does not match its block size")
                out[r, :a.size] = a.ravel()
            return self._f64(out)

        d_re, d_im = pack(noise_re), pack(noise_im)
        d_ng = pack(nugget_fields) if nugget_fields is not None else None
        d_si, d_sc = torch.as_tensor(size_idx).to(self.dev), self._f64(sc)
        out = torch.zeros((n, self.field_stride), dtype=torch.float64, device=self.dev)
        p = rf if isinstance(rf, RfParams) else self.rf_struct(rf)
        self.call(self.lib.gsm_spectral_from_noise, n, d_si, d_sc, C.byref(p), d_re, d_im, d_ng, out, self.field_stride)
        torch.cuda.synchronize(self.dev)
        h = out.cpu().numpy()
        return [h[r, :int(self.bh[size_idx[r]] * self.bw[size_idx[r]])].reshape(int(self.bh[size_idx[r]]), int(self.bw[size_idx[r]]))
                for r in range(n)]

    # ---- 'pcg64' draw mode: NumPy's generator streams on the device (gsm_draw_pcg64) ------------------------------------
    @staticmethod
    def pack_pcg64_states(gens):
        """[n, 6] uint64 from numpy Generators / bit_generator.state dicts: state lo, hi, inc lo, hi, has_uint32, uinteger."""
        out = np.zeros((len(gens), 6), dtype=np.uint64)
        m = (1 << 64) - 1
        for i, g in enumerate(gens):
            st = g if isinstance(g, dict) else g.bit_generator.state
            if st.get("bit_generator") != "PCG64":
                raise ValueError("the pcg64 draw mode needs numpy.random.Generator(PCG64) generators (numpy.random.default_rng)")
            s, inc = int(st["state"]["state"]), int(st["state"]["inc"])
            out[i] = [s & m, s >> 64, inc & m, inc >> 64, int(st["has_uint32"]), int(st["uinteger"])]
        return out

    @staticmethod
    def unpack_pcg64_states(words):
        """numpy bit_generator.state dicts from [n, 6] uint64 (assign to generator.bit_generator.state)."""
        return [{"bit_generator": "PCG64", "state": {"state": int(w[0]) | (int(w[1]) << 64), "inc": int(w[2]) | (int(w[3]) << 64)},
                 "has_uint32": int(w[4]), "uinteger": int(w[5])} for w in np.asarray(words, dtype=np.uint64)]

    def pcg64_to_device(self, gens):
        """int64 [n, 6] device tensor of pack_pcg64_states(gens): what gsm_draw_pcg64 and its kin advance in place."""
        return torch.as_tensor(self.pack_pcg64_states(gens).view(np.int64)).to(self.dev)

    @staticmethod
    def pcg64_from_device(t):
        """bit_generator.state dicts of such a tensor."""
        return GsmEngine.unpack_pcg64_states(t.cpu().numpy().view(np.uint64))

    def blocks_of(self, size_idx, centre):
        """The reference's block records (row, col, bh, bw), float64 [..., n, 4], of host arrays size_idx [..., n] and centre [..., n, 2]."""
        out = np.empty(size_idx.shape + (4,))
        out[..., 0:2] = centre
        out[..., 2] = self.bh[size_idx]
        out[..., 3] = self.bw[size_idx]
        return out

    def alloc_pcg64_buffers(self, n_steps, nugget):
        """Caller-owned outputs of draw_pcg64 for batches of n_steps (reused from batch to batch: only the bh * bw leading doubles of
        a record's planes are written and read)."""
        n = self.n_chains * n_steps
        shape = (self.n_chains, n_steps, self.field_stride)
        z = lambda: torch.zeros(shape, dtype=torch.float64, device=self.dev)
        return dict(size_idx=torch.empty(n, dtype=torch.int32, device=self.dev), centre=torch.empty(n * 2, dtype=torch.int32, device=self.dev),
                    u=torch.empty(n, dtype=torch.float64, device=self.dev), rf_scalars=torch.empty(n * 4, dtype=torch.float64, device=self.dev),
                    noise_re=z(), noise_im=z(), nugget=z() if nugget else None, n_steps=n_steps)

    def draw_pcg64(self, n_steps, rf, d_rf_state, d_chain_state, d_region_mask=None, buffers=None):
        """n_steps Metropolis steps' worth of the reference's NumPy draws for every chain, on the device (asynchronous on the
        current stream).  d_rf_state / d_chain_state: int64 device tensors [n_chains, 6] (pack_pcg64_states), advanced in place.
        Returns device tensors size_idx [n, s], centre [n, s, 2], u [n, s], rf_scalars [n, s, 4], noise_re / noise_im
        [n, s, field_stride] and nugget (or None); `buffers` (alloc_pcg64_buffers of the same n_steps) are used if given."""
        p = rf if isinstance(rf, RfParams) else self.rf_struct(rf)
        b = buffers if (buffers is not None and buffers["n_steps"] == n_steps) else self.alloc_pcg64_buffers(n_steps, p.nugget_max > 0.0)
        self.call(self.lib.gsm_draw_pcg64, int(n_steps), C.byref(p), d_rf_state, d_chain_state, d_region_mask, b["size_idx"], b["centre"], b["u"],
                  b["rf_scalars"], b["noise_re"], b["noise_im"], b["nugget"], self.field_stride)
        return dict(size_idx=b["size_idx"].view(self.n_chains, n_steps), centre=b["centre"].view(self.n_chains, n_steps, 2),
                    u=b["u"].view(self.n_chains, n_steps), rf_scalars=b["rf_scalars"].view(self.n_chains, n_steps, 4),
                    noise_re=b["noise_re"], noise_im=b["noise_im"], nugget=b["nugget"])

    def run_noise(self, n_steps, d, rf, loss, accept):
        """n_steps Metropolis steps for every chain with synthesis and step in one kernel (gsm_run_noise; block tables on the strip
        kernels only), on the device draws `d` of draw_pcg64.  loss [n_chains, n_steps] float64 and accept [n_chains, n_steps] uint8
        are device tensors that receive the results.  Asynchronous on the current stream."""
        self._need_beds()
        p = rf if isinstance(rf, RfParams) else self.rf_struct(rf)
        self.call(self.lib.gsm_run_noise, int(n_steps), self.beds, self.energy, self.resampled, self.loss_sum, d['size_idx'], d['centre'], d['u'],
                  d['rf_scalars'], C.byref(p), d['noise_re'], d['noise_im'], d['nugget'], self.field_stride, loss, accept)

    def step_on_draws(self, n_steps, d, p, loss, accept, fields=None):
        """The device draws `d` of draw_pcg64 to losses and accepts: the fused kernel (run_noise), or with `fields`
        [n_chains, n_steps, field_stride] the synthesis into it (gsm_spectral_from_noise) and the step from it (gsm_run_replay).
        Asynchronous on the current stream; allocates nothing."""
        if fields is None:
            return self.run_noise(n_steps, d, p, loss, accept)
        self.call(self.lib.gsm_spectral_from_noise, self.n_chains * n_steps, d['size_idx'], d['rf_scalars'], C.byref(p), d['noise_re'],
                  d['noise_im'], d['nugget'], fields, self.field_stride)
        self.call(self.lib.gsm_run_replay, n_steps, self.beds, self.energy, self.resampled, self.loss_sum, d['size_idx'], d['centre'], d['u'],
                  fields, self.field_stride, loss, accept)

    def enable_timing(self, on=True):
        self._check(self.lib.gsm_enable_timing(self.h, 1 if on else 0))

    def last_timing(self):
        a, b = C.c_double(), C.c_double()
        na, nb = C.c_int32(), C.c_int32()
        self._check(self.lib.gsm_last_timing(self.h, C.byref(a), C.byref(na), C.byref(b), C.byref(nb)))
        return dict(step_ms=a.value, step_launches=na.value, proposal_ms=b.value, proposal_launches=nb.value)

    def set_fused(self, on: bool):
        """Philox mode, spectral generator: fused chain kernel (default) or the two-kernel pipeline (same results)."""
        self.set_option("fused", int(bool(on)))

    def set_option(self, name: str, value: int):
        """gsm_set_option (include/gsm.h): 'fused', 'strip', 'split2' (0 / 1) or 'fused_segment' (>= 1); from the next call on."""
        self._check(self.lib.gsm_set_option(self.h, _lib.OPTION_IDS[name], int(value)))

    def last_run_fused(self) -> int:
        return int(self.lib.gsm_last_run_fused(self.h))

    def strip_active(self) -> bool:
        """True when this handle's tables go to the strip kernels (two chains per CU), False for the flux-tile kernels."""
        rc = int(self.lib.gsm_strip_active(self.h))
        if rc < 0:
            self._check(rc)
        return bool(rc)

    def run_philox(self, n_steps, step0, seeds, rf, batch=8, out=None, to_host=True):
        """n_steps Metropolis steps for every chain with on-device proposals.
        Returns (loss, accept, blocks): (n_chains, n_steps), (n_chains, n_steps), (n_chains, n_steps, 4)."""
        self._need_beds()
        d_seeds = self._seeds(seeds)
        if out is None:
            loss = torch.empty((self.n_chains, n_steps), dtype=torch.float64, device=self.dev)
            acc = torch.empty((self.n_chains, n_steps), dtype=torch.uint8, device=self.dev)
            blocks = torch.empty((self.n_chains, n_steps, 4), dtype=torch.int32, device=self.dev)
        else:
            loss, acc, blocks = out
        p = rf if isinstance(rf, RfParams) else self.rf_struct(rf)
        self.call(self.lib.gsm_run_philox, int(n_steps), int(step0), int(batch), d_seeds, C.byref(p), self.beds, self.energy, self.resampled,
                  self.loss_sum, loss, acc, blocks)
        if to_host:
            return loss.cpu().numpy(), acc.cpu().numpy(), blocks.cpu().numpy()
        return loss, acc, blocks
