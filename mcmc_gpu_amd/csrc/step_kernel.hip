// Metropolis step kernels for gfx950 (MI355X): one workgroup per chain, the CANDIDATE bed of the proposal
// window (+1-cell halo) staged in LDS, all steps of a launch looped inside the kernel.
//
// Replaces the loop body of chain_crf.run (reference gstatsMCMC/MCMC.py:1263-1360):
//   window/clipping         MCMC.py:1266-1276
//   perturb + update mask   MCMC.py:1279-1290
//   residual on window+halo MCMC.py:1293-1315 -> Topography.get_mass_conservation_residual (Topography.py:592-600)
//   Gaussian loss           MCMC.py:1318      -> chain.loss (MCMC.py:1021-1044)
//   thickness guard         MCMC.py:1321-1329
//   accept / bookkeeping    MCMC.py:1331-1360
//
// What is carried between steps (per chain, in HBM): the bed, the "energy" e = r^2 where the cell enters the loss
// (mc_mask == 1 and r is not NaN -- nansum semantics, MCMC.py:1041) else 0, the uint32 resampled counts, and the
// compensated pair (hi, lo) with hi + lo = sum(e).  The reference carries the residual array r itself
// (MCMC.py:1308-1315, :1340) and re-reduces the whole grid every step; because the edge taper is exactly 0 on the
// block border (MCMC.py:583-623 with the driver's logistic parameters) a proposal changes r only inside its window,
// so   sum_next = sum_prev - sum_window(e_old) + sum_window(e_new)   is the same quantity.  Arithmetic per residual
// is the reference's, operation for operation (this file is built with -ffp-contract=off; the only fused op is the
// explicit fma pair of exact_div, which returns the correctly rounded quotient), so only the summation order of the
// loss differs (|rel diff| ~1e-15; test bound 1e-10) and accept decisions are identical.
//
// Per step:  A  stage bed window+halo in LDS with the perturbation already applied (f * weight where update_mask),
//               thickness guard, and sum the carried e of the window          -- 1 barrier
//            D  5-point stencil on the LDS tile -> e_new kept in registers, summed
//            R  workgroup reduction, every thread evaluates the same accept test -- 1 barrier
//            E  on accept: write bed window, e window, bump resampled           -- 1 barrier (a full fence only
//               when the next step's halo window overlaps this window; see the end of the step loop)
// HBM bytes per chain-step: read (bh+2)(bw+2) bed + bh*bw e + bh*bw f; on accept write bh*bw bed + bh*bw e and
// read-modify-write bh*bw uint32.  Static fields are shared by all chains and stay in L2 / Infinity Cache.

#include "gsm_internal.h"
#include "residual_device.h"
#include "step_common.h"
#include <math.h>
#include <stdlib.h>
#include <algorithm>

namespace gsm {

using dev::magic_for;
using dev::two_sum;

// q = __umulhi(n, M) == n / d with M = magic_for(d), for n*d < 2^32 (here n < 2^16, 2 <= d < 2^8); d == 1 would need M = 2^32
__device__ __forceinline__ int div_magic(int n, uint32_t d, uint32_t M) {
  return (d == 1u) ? n : (int)__umulhi((uint32_t)n, M);   // a 2-wide block clipped at the grid edge is 1 cell wide
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;  // valid in lane 0
}

// ---------------------------------------------------------------------------------------------------
// step kernel.  NT threads per workgroup, KMAX = ceil(max window cells / NT) window cells per thread.
// ---------------------------------------------------------------------------------------------------
// TS = state element type: double, or float ("fp32 state, fp64 arithmetic": the candidate bed and the new
// energies are rounded to float BEFORE they are used, so the carried sum always equals the sum of what is stored).
template <typename TS, int NT, int KMAX, bool FAST_DIV, int MINW>
__global__ __launch_bounds__(NT, MINW) void step_kernel(const StepArgs a) {
  constexpr bool F32 = sizeof(TS) == 4;
  constexpr bool DEEP = (MINW * 256 / NT) <= 1;   // one workgroup per CU: registers to spare for deep load batching
  constexpr int NW = NT / 64;
  extern __shared__ double lds[];
  double* tile = lds;
  double* red = lds + a.tile_cap;  // [NW][3]

  const StaticFields& S = a.S;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int chain = blockIdx.x;
  const int H = S.H, W = S.W;
  const size_t plane = (size_t)H * W;
  TS* __restrict__ bed = (TS*)a.beds + (size_t)chain * plane;
  TS* __restrict__ energy = (TS*)a.energy + (size_t)chain * plane;
  uint32_t* __restrict__ resamp = a.resampled + (size_t)chain * plane;
  const double2* __restrict__ svx = S.svx;
  const double2* __restrict__ svy = S.svy;
  const double2* __restrict__ dsp = S.ds;

  double s_hi = a.loss_sum[2 * chain], s_lo = a.loss_sum[2 * chain + 1];
  double loss_prev = (s_hi + s_lo) / S.two_sigma2;

  // block-size table -> LDS once; per-step scalars are fetched one step ahead (the end-of-step fence below needs the
  // next window before the step ends)
  int* tab = (int*)(red + 3 * 16);
  for (int i = tid; i < a.B.n_sizes; i += NT) { tab[2 * i] = a.B.bh[i]; tab[2 * i + 1] = a.B.bw[i]; }
  const int64_t rin0 = (int64_t)chain * a.in_stride;
  step::ReplayRec nxt = step::read_replay(a, rin0);
  const step::StepConsts SC{S.res, S.rcp_res, S.two_res, S.rcp_two_res};
  __syncthreads();

  for (int s = 0; s < a.n_steps; ++s) {
    const int64_t rin = rin0 + s;
    const int64_t rout = step::record_index(a, chain, s);
    const step::ReplayRec cur = nxt;
    const bool has_next = s + 1 < a.n_steps;
    if (has_next) nxt = step::read_replay(a, rin + 1);
    if (!step::replay_valid(a, cur)) {
      if (tid == 0) step::reject_record(a, rout, loss_prev, cur);
      continue;  // uniform across the workgroup
    }
    const int bh = tab[2 * cur.si], bw = tab[2 * cur.si + 1];
    const double* __restrict__ fld = a.fields + rin * a.field_stride;

    const step::Window G = step::clip_window(H, W, cur.row, cur.col, bh, bw);
    const step::HaloTile T = step::halo_tile(H, W, G);
    const int r0 = G.r0, c0 = G.c0, ww = G.ww, hr0 = T.hr0, hc0 = T.hc0, tw = T.tw;
    const int ncell = T.ncell, nwin = G.wh * ww;
    const uint32_t m_tw = magic_for((uint32_t)tw), m_ww = magic_for((uint32_t)ww);

    // ---- A: candidate bed -> LDS, guard, sum of the carried energy of the window ------------------
    double acc_old = 0.0;
    int guard = 0;
    if (DEEP) {
      // deep variant (one workgroup per CU, 128-VGPR budget): every HBM-latency load of the step (bed, energy, f)
      // is issued before the first is consumed -- one exposed HBM round trip instead of one per unrolled pair
      constexpr int KT = KMAX + 1;           // tile cells per thread: (bh+2)(bw+2) <= (KMAX + 1) * NT (host-checked)
      double vb[KT], vf[KT], ve[KT];
#pragma unroll
      for (int k = 0; k < KT; ++k) {
        const int i = tid + k * NT;
        vb[k] = 0.0; vf[k] = 0.0; ve[k] = 0.0;
        if (i < ncell) {
          const int lr = (int)__umulhi((uint32_t)i, m_tw);
          const int lc = i - lr * tw;
          const int g = (hr0 + lr) * W + hc0 + lc;
          vb[k] = (double)__builtin_nontemporal_load(&bed[g]);
          if (step::in_window(G, T, lr, lc)) {
            ve[k] = (double)__builtin_nontemporal_load(&energy[g]);
            vf[k] = __builtin_nontemporal_load(&fld[step::field_index(G, T, lr, lc, bw)]);
          }
        }
      }
#pragma unroll
      for (int k = 0; k < KT; ++k) acc_old += ve[k];
#pragma unroll
      for (int k = 0; k < KT; ++k) {
        const int i = tid + k * NT;
        if (i < ncell) {
          const int lr = (int)__umulhi((uint32_t)i, m_tw);
          const int lc = i - lr * tw;
          const int g = (hr0 + lr) * W + hc0 + lc;
          double v = vb[k];
          if (step::in_window(G, T, lr, lc) && S.upd[g]) {
            const double pert = S.weight ? vf[k] * S.weight[g] : vf[k];
            v = v + pert;
            if (F32) v = (double)(float)v;
            if (svx[g].x - v <= 0.0) guard = 1;
          }
          tile[i] = v;
        }
      }
    } else {
#pragma unroll 2
    for (int i = tid; i < ncell; i += NT) {
      const int lr = (int)__umulhi((uint32_t)i, m_tw);
      const int lc = i - lr * tw;
      const int g = (hr0 + lr) * W + hc0 + lc;
      double v = (double)__builtin_nontemporal_load(&bed[g]);
      if (step::in_window(G, T, lr, lc)) {
        acc_old += (double)__builtin_nontemporal_load(&energy[g]);
        if (S.upd[g]) {
          const double f = __builtin_nontemporal_load(&fld[step::field_index(G, T, lr, lc, bw)]);
          const double pert = S.weight ? f * S.weight[g] : f;
          v = v + pert;
          if (F32) v = (double)(float)v;
          if (svx[g].x - v <= 0.0) guard = 1;
        }
      }
      tile[i] = v;
    }
    }
    __syncthreads();

    // ---- D: residual stencil on the candidate tile ---------------------------------------------------
    double e_new[KMAX];
    double acc_new = 0.0;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      const int i = tid + k * NT;
      double e = 0.0;
      if (i < nwin) {
        const int wr = div_magic(i, (uint32_t)ww, m_ww);
        const int wc = i - wr * ww;
        const int r = r0 + wr, c = c0 + wc;
        const int g = r * W + c;
        if (S.mc[g] == 1) {
          const int cl = (c == 0) ? 0 : c - 1, cr = (c == W - 1) ? W - 1 : c + 1;
          const int ru = (r == 0) ? 0 : r - 1, rd = (r == H - 1) ? H - 1 : r + 1;
          const double2 xr = svx[r * W + cr], xl = svx[r * W + cl];
          const double2 yd = svy[rd * W + c], yu = svy[ru * W + c];
          const double2 dd = dsp[g];
          const int trow = (r - hr0) * tw - hc0;
          const double qxr = xr.y * (xr.x - tile[trow + cr]);
          const double qxl = xl.y * (xl.x - tile[trow + cl]);
          const double qyd = yd.y * (yd.x - tile[(rd - hr0) * tw + (c - hc0)]);
          const double qyu = yu.y * (yu.x - tile[(ru - hr0) * tw + (c - hc0)]);
          e = step::flux_energy<FAST_DIV, F32, false>(qxr - qxl, qyd - qyu, cr - cl == 2, rd - ru == 2, dd, SC);   // dd = (dhdt, smb), mc_mask tested above
        }
      }
      e_new[k] = e;
      acc_new += e;
    }

    // ---- R: reduce, decide (every thread evaluates the same numbers in the same order) ----------------
    acc_old = wave_sum(acc_old);
    acc_new = wave_sum(acc_new);
    const int any_guard = __any(guard);
    if (lane == 0) {
      red[wave * 3 + 0] = acc_old;
      red[wave * 3 + 1] = acc_new;
      red[wave * 3 + 2] = any_guard ? 1.0 : 0.0;
    }
    __syncthreads();
    double so = 0.0, sn = 0.0, gd = 0.0;
#pragma unroll
    for (int w = 0; w < NW; ++w) { so += red[w * 3]; sn += red[w * 3 + 1]; gd += red[w * 3 + 2]; }
    // the guard is counted apart from the (finite) sums; this kernel divides plainly in both instantiations
    double c_hi, c_lo, loss_next;
    const bool acc = step::decide<false>(sn - so, gd > 0.0, s_hi, s_lo, S.two_sigma2, S.rcp_two_sigma2, loss_prev, cur.u, c_hi, c_lo, loss_next);

    // ---- E: commit -------------------------------------------------------------------------------------
    if (acc) {
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        const int i = tid + k * NT;
        if (i < nwin) {
          const int wr = div_magic(i, (uint32_t)ww, m_ww);
          const int wc = i - wr * ww;
          const int r = r0 + wr, c = c0 + wc;
          const size_t g = (size_t)r * W + c;
          __builtin_nontemporal_store((TS)e_new[k], &energy[g]);
          if (S.upd[g]) {
            __builtin_nontemporal_store((TS)tile[(r - hr0) * tw + (c - hc0)], &bed[g]);
            __builtin_nontemporal_store(__builtin_nontemporal_load(&resamp[g]) + 1u, &resamp[g]);
          }
        }
      }
      two_sum(c_hi, c_lo, s_hi, s_lo);
      loss_prev = loss_next;
    }
    if (tid == 0) step::write_record(a, rout, loss_prev, acc, cur.row, cur.col, bh, bw);
    // End of step.  The LDS tile / reduction scratch may be reused once every wave is here (raw barrier after the
    // wave's own LDS reads have returned).  The global stores of an accepted step must be visible to the next step's
    // loads only if the next halo window touches this window; otherwise the workgroup does not wait for them
    // (__syncthreads() would: its release fence drains vmcnt, one exposed HBM round trip per step).
    bool fence = acc;
    if (fence && has_next && (unsigned)nxt.si < (unsigned)a.B.n_sizes)
      fence = step::halo_touches(step::clip_window(H, W, nxt.row, nxt.col, tab[2 * nxt.si], tab[2 * nxt.si + 1]), G);
    if (fence) __syncthreads();
    else asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  }
  if (tid == 0) {
    a.loss_sum[2 * chain] = s_hi;
    a.loss_sum[2 * chain + 1] = s_lo;
  }
}

size_t step_lds_bytes(int tile_cap) { return ((size_t)tile_cap + 3 * 16 + 64) * sizeof(double); }  // tile + reduction + size table (<= 64 sizes)

template <typename TS, int NT, int KMAX, int MINW>
static hipError_t launch_step_t(const StepArgs& a, hipStream_t st) {
  return launch_pair<step_kernel<TS, NT, KMAX, true, MINW>, step_kernel<TS, NT, KMAX, false, MINW>>(
      a.S.fast_div, 160 * 1024, dim3(a.n_chains), dim3(NT), step_lds_bytes(a.tile_cap), st, a);
}

hipError_t launch_step(const StepArgs& a, hipStream_t st) {
  // window cells per thread: the largest block of the table decides the instantiation
  // (window cells <= KMAX * NT and tile cells <= (KMAX + 1) * NT)
  if (a.strip) return launch_step_strip(a, st);      // pairs with chain_strip_kernel (same sums)
  const int max_win = std::max(a.B.max_bh * a.B.max_bw, a.tile_cap - 1024);
  // the flux-tile kernel (step_flux_kernel.hip); blocks beyond its two LDS tiles fall back to the bed-tile form
  if (step_flux_supported(a)) return launch_step_flux(a, st);
  if (a.f32_state) {
    if (max_win <= 1024 * 7) return launch_step_t<float, 1024, 7, 8>(a, st);
    if (max_win <= 1024 * 12) return launch_step_t<float, 1024, 12, 4>(a, st);
    if (max_win <= 1024 * 20) return launch_step_t<float, 1024, 20, 4>(a, st);
    return hipErrorInvalidValue;
  }
  if (max_win <= 1024 * 7) return launch_step_t<double, 1024, 7, 8>(a, st);   // <=64 VGPRs: 2 workgroups per CU (fastest measured)
  if (max_win <= 1024 * 12) return launch_step_t<double, 1024, 12, 4>(a, st);
  if (max_win <= 1024 * 20) return launch_step_t<double, 1024, 20, 4>(a, st);
  return hipErrorInvalidValue;  // gsm_set_blocks refuses such tables (LDS tile limit is reached first)
}

// ---------------------------------------------------------------------------------------------------
// full-grid residual, energy and loss of the current beds (MCMC.py:1189-1195)
// ---------------------------------------------------------------------------------------------------
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;

template <typename TS>
__global__ __launch_bounds__(kBlock) void init_loss_kernel(const StaticFields S, const TS* beds, TS* energy,
                                                           double* loss_sum, double* loss0) {
  __shared__ double red[kWaves * 2];
  const int chain = blockIdx.x, tid = threadIdx.x;
  const size_t plane = (size_t)S.H * S.W;
  const TS* bed = beds + (size_t)chain * plane;
  TS* en = energy ? energy + (size_t)chain * plane : nullptr;
  auto bed_at = [&](int rr, int cc) { return (double)bed[(size_t)rr * S.W + cc]; };
  // per-thread compensated partial
  double hi = 0.0, lo = 0.0;
  for (int g = tid; g < (int)plane; g += kBlock) {
    double e = 0.0;
    if (S.mc[g] == 1) {
      const int r = g / S.W, c = g - r * S.W;
      const double v = cell_residual(S, r, c, bed_at);
      if (!isnan(v)) e = v * v;
      if (sizeof(TS) == 4) e = (double)(float)e;
    }
    if (en) en[g] = (TS)e;
    double s, err;
    two_sum(hi, e, s, err);
    hi = s;
    lo += err;
  }
  // wave tree on (hi, lo) with two_sum at each level
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double ohi = __shfl_down(hi, off, 64), olo = __shfl_down(lo, off, 64);
    double s, e;
    two_sum(hi, ohi, s, e);
    hi = s;
    lo += olo + e;
  }
  if ((tid & 63) == 0) { red[(tid >> 6) * 2] = hi; red[(tid >> 6) * 2 + 1] = lo; }
  __syncthreads();
  if (tid == 0) {
    double th = 0.0, tl = 0.0;
    for (int w = 0; w < kWaves; ++w) {
      double s, e;
      two_sum(th, red[2 * w], s, e);
      th = s;
      tl += red[2 * w + 1] + e;
    }
    double nh, nl;
    two_sum(th, tl, nh, nl);
    loss_sum[2 * chain] = nh;
    loss_sum[2 * chain + 1] = nl;
    if (loss0) loss0[chain] = (nh + nl) / S.two_sigma2;
  }
}

hipError_t launch_init_loss(const StaticFields& S, int n_chains, const void* beds, void* energy, int f32_state,
                            double* loss_sum, double* loss0, hipStream_t st) {
  if (f32_state)
    hipLaunchKernelGGL(init_loss_kernel<float>, dim3(n_chains), dim3(kBlock), 0, st, S, (const float*)beds, (float*)energy, loss_sum, loss0);
  else
    hipLaunchKernelGGL(init_loss_kernel<double>, dim3(n_chains), dim3(kBlock), 0, st, S, (const double*)beds, (double*)energy, loss_sum, loss0);
  return hipGetLastError();
}

__global__ __launch_bounds__(kBlock) void pack_static_kernel(const StaticFields S, double2* svx, double2* svy, double2* ds) {
  const int n = S.H * S.W;
  for (int g = blockIdx.x * kBlock + threadIdx.x; g < n; g += gridDim.x * kBlock) {
    svx[g] = make_double2(S.surf[g], S.velx[g]);
    svy[g] = make_double2(S.surf[g], S.vely[g]);
    ds[g] = make_double2(S.dhdt[g], S.smb[g]);
  }
}

hipError_t launch_pack_static(const StaticFields& S, double2* svx, double2* svy, double2* ds, hipStream_t st) {
  int grid = (S.H * S.W + kBlock - 1) / kBlock;
  if (grid > 2048) grid = 2048;
  hipLaunchKernelGGL(pack_static_kernel, dim3(grid), dim3(kBlock), 0, st, S, svx, svy, ds);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// Utilities.min_dist_from_mask (Utilities.py:21-24): distance of every cell to the nearest masked cell.
// Exact brute force: min over masked points of (dx*dx + dy*dy), then sqrt -- the arithmetic of the KD-tree
// query's final distance (no FMA: this file is built with -ffp-contract=off); points staged through LDS.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void compact_points_kernel(const double* xx, const double* yy, const uint8_t* mask,
                                                                int n, double2* pts, int* count) {
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock)
    if (mask[i]) pts[atomicAdd(count, 1)] = make_double2(xx[i], yy[i]);
}

__global__ __launch_bounds__(kBlock) void min_dist_kernel(const double* __restrict__ xx, const double* __restrict__ yy,
                                                          int n, const double2* __restrict__ pts,
                                                          const int* __restrict__ count, double* __restrict__ dist) {
  __shared__ double2 sp[kBlock];
  const int m = *count;
  const int i = blockIdx.x * kBlock + threadIdx.x;
  const double x = (i < n) ? xx[i] : 0.0, y = (i < n) ? yy[i] : 0.0;
  double best = INFINITY;
  for (int p0 = 0; p0 < m; p0 += kBlock) {
    if (p0 + (int)threadIdx.x < m) sp[threadIdx.x] = pts[p0 + threadIdx.x];
    __syncthreads();
    const int lim = min(kBlock, m - p0);
    for (int j = 0; j < lim; ++j) {
      const double dx = x - sp[j].x, dy = y - sp[j].y;
      best = fmin(best, dx * dx + dy * dy);
    }
    __syncthreads();
  }
  if (i < n) dist[i] = sqrt(best);
}

hipError_t launch_min_dist(const double* xx, const double* yy, const uint8_t* mask, int n, double2* pts, int* count,
                           double* dist, hipStream_t st) {
  hipLaunchKernelGGL(compact_points_kernel, dim3(256), dim3(kBlock), 0, st, xx, yy, mask, n, pts, count);
  hipLaunchKernelGGL(min_dist_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, xx, yy, n, pts, count, dist);
  return hipGetLastError();
}

__global__ __launch_bounds__(kBlock) void stream_copy_kernel(const double* __restrict__ src, double* __restrict__ dst, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) dst[i] = src[i];
}

hipError_t launch_stream_copy(const double* src, double* dst, int64_t n, hipStream_t st) {
  hipLaunchKernelGGL(stream_copy_kernel, dim3(2048), dim3(kBlock), 0, st, src, dst, n);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// Topography.get_mass_conservation_residual for a batch of beds (Topography.py:592-600)
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void residual_kernel(const StaticFields S, int n_chains, const double* beds,
                                                          double* out) {
  const size_t plane = (size_t)S.H * S.W;
  const size_t total = plane * (size_t)n_chains;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (size_t)gridDim.x * kBlock) {
    const size_t chain = i / plane;
    const int g = (int)(i - chain * plane);
    const int r = g / S.W, c = g - r * S.W;
    const double* bed = beds + chain * plane;
    auto bed_at = [&](int rr, int cc) { return bed[(size_t)rr * S.W + cc]; };
    out[i] = cell_residual(S, r, c, bed_at);
  }
}

hipError_t launch_residual(const StaticFields& S, int n_chains, const double* beds, double* out, hipStream_t st) {
  const size_t total = (size_t)S.H * S.W * n_chains;
  int grid = (int)((total + kBlock - 1) / kBlock);
  if (grid > 2048) grid = 2048;
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL(residual_kernel, dim3(grid), dim3(kBlock), 0, st, S, n_chains, beds, out);
  return hipGetLastError();
}

}  // namespace gsm
