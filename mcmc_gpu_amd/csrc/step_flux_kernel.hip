// Metropolis step kernel, "flux tile" form, for gfx950 (MI355X): one 1024-thread workgroup per chain and per CU,
// all steps of a launch looped inside the kernel.  Same contract and the same arithmetic as step_kernel.hip
// (reference gstatsMCMC/MCMC.py:1263-1360, Topography.py:592-600); what differs is where the operands live:
//
//   * The mass fluxes  qx = velx * (surf - bed_next),  qy = vely * (surf - bed_next)  of the candidate bed are
//     computed ONCE per cell of the window + 1-cell halo and kept in two LDS tiles (2 x 82 x 82 fp64 = 105 KiB for
//     the 80 x 80 block).  The 5-point stencil then reads only LDS: np.gradient's central / one-sided differences of
//     the flux arrays are differences of tile neighbours.  (step_kernel.hip keeps the candidate bed in LDS and loads
//     surf/velx/vely of four neighbours per window cell: 80 B of static operands per cell against 48 B here.)
//   * The masks are folded into the static operands so that no load depends on another load:
//         sA = (wupd, surf)      wupd = crf weight (1.0 for block_type 'RF') where update_mask is set, else a tagged NaN
//         sB = (velx, vely)
//         sC = (dhdt_mc, smb)    dhdt_mc = dhdt where mc_mask == 1, else NaN  (a NaN residual is ignored by the loss:
//                                nansum semantics, MCMC.py:1041 -- the same outcome as "cell not in the mask")
//   * Every per-lane address is a 32-bit offset into a buffer descriptor; lanes outside the tile / window use an
//     out-of-range offset (the load returns 0, the store is dropped), so the phases have no divergent branches and the
//     loads of a phase issue back to back.
//   * One mapping for everything: thread t owns tile cells t, t + 1024, ...; it stages them, evaluates their residuals
//     and commits them, so the candidate bed and the new energies never leave its registers.
//   * resampled_times is bumped with a no-return integer atomic (no read round trip).
//
// Per step: A  loads + candidate bed + fluxes -> LDS, guard, sum of the carried energy      -- 1 barrier
//           D  stencil from LDS -> new energies (registers)
//           R  DPP wave reduction, 16 partials through LDS                                    -- 1 barrier
//           E  commit on accept; the stores are waited for only when the next window overlaps this one
#include "gsm_internal.h"
#include "device_util.h"
#include "step_common.h"
#include <math.h>
#include <stdlib.h>
#include <algorithm>

namespace gsm {

using namespace dev;

size_t step_flux_lds_bytes(int tile_cap) { return ((size_t)2 * tile_cap + 4 * kNW + 64) * sizeof(double); }

// KT = tile cells per thread: (bh + 2)(bw + 2) <= KT * 1024 for every block of the table (host-checked).
template <typename TS, int KT, bool FAST_DIV>
__global__ __launch_bounds__(kNT, 4) void step_flux_kernel(const StepArgs a) {
  constexpr bool F32 = sizeof(TS) == 4;
  extern __shared__ double lds[];
  double* __restrict__ qx = lds;
  double* __restrict__ qy = lds + a.tile_cap;
  double* __restrict__ red = lds + 2 * a.tile_cap;   // [kNW][4]
  int* tab = (int*)(red + 4 * kNW);

  const StaticFields& S = a.S;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int chain = blockIdx.x;
  const int H = S.H, W = S.W;
  const uint32_t ncells = (uint32_t)H * (uint32_t)W;
  const size_t plane = (size_t)H * W;
  const rsrc_t r_bed = make_rsrc((const TS*)a.beds + (size_t)chain * plane, ncells * (uint32_t)sizeof(TS));
  const rsrc_t r_en = make_rsrc((const TS*)a.energy + (size_t)chain * plane, ncells * (uint32_t)sizeof(TS));
  const rsrc_t r_rs = make_rsrc(a.resampled + (size_t)chain * plane, ncells * 4u);
  const rsrc_t r_sA = make_rsrc(S.sA, ncells * 16u);
  const rsrc_t r_sB = make_rsrc(S.sB, ncells * 16u);
  const rsrc_t r_sC = make_rsrc(S.sC, ncells * 16u);

  double s_hi = a.loss_sum[2 * chain], s_lo = a.loss_sum[2 * chain + 1];
  double loss_prev = (s_hi + s_lo) / S.two_sigma2;

  for (int i = tid; i < a.B.n_sizes; i += kNT) { tab[2 * i] = a.B.bh[i]; tab[2 * i + 1] = a.B.bw[i]; }
  const int64_t rin0 = (int64_t)chain * a.in_stride;
  step::ReplayRec nxt = step::read_replay(a, rin0);
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
    const rsrc_t r_f = make_rsrc(a.fields + rin * a.field_stride, (uint32_t)(bh * bw) * 8u);

    const step::Window G = step::clip_window(H, W, cur.row, cur.col, bh, bw);
    const step::HaloTile T = step::halo_tile(H, W, G);
    const int tw = T.tw, ncell = T.ncell;
    const uint32_t m_tw = magic_for((uint32_t)tw);

    // geometry of the thread's k-th tile cell (recomputed per phase: cheaper than 2 registers per cell)
    int ptid = tid;   // re-laundered at each phase so that the geometry is recomputed, not kept live across phases
    auto cell = [&](int k, int& i, int& lr, int& lc, uint32_t& g, bool& valid, bool& inwin) {
      i = ptid + k * kNT;
      valid = i < ncell;
      lr = (int)__umulhi((uint32_t)i, m_tw);
      lc = i - lr * tw;
      g = (uint32_t)((T.hr0 + lr) * W + T.hc0 + lc);
      inwin = valid && (unsigned)(lr - T.dr) < (unsigned)G.wh && (unsigned)(lc - T.dc) < (unsigned)G.ww;
    };

    // cell slot k of this wave is past the end of the tile for the later slots of smaller blocks: wave-uniform skip
    auto slot_on = [&](int k) { return k * kNT + 64 * wave < ncell; };

    // ---- A: loads, candidate bed, fluxes -> LDS, guard, carried energy of the window -----------------
    // in sub-batches of KB cells: all loads of a sub-batch are in flight together (14 VGPRs per cell)
    double v_new[KT];        // candidate bed of the thread's cells
    uint32_t upd_bits = 0;
    double acc_old = 0.0;
    int guard = 0;
    constexpr int KB = (KT > 4) ? 4 : KT;
#pragma unroll
    for (int kb = 0; kb < KT; kb += KB) {
      if (kb > 0 && !slot_on(kb)) break;   // no cell of this wave in this sub-batch nor in any later one
      double vb[KB], ve[KB], vf[KB];
      double2 A2[KB], B2[KB];
#pragma unroll
      for (int j = 0; j < KB; ++j) {
        const int k = kb + j;
        if (k < KT) {
          int i, lr, lc; uint32_t g; bool valid, inwin;
          cell(k, i, lr, lc, g, valid, inwin);
          vb[j] = StateIO<TS>::load(r_bed, valid ? g * (uint32_t)sizeof(TS) : kOOB);
          ve[j] = StateIO<TS>::load(r_en, inwin ? g * (uint32_t)sizeof(TS) : kOOB);
          vf[j] = ld_f64<2>(r_f, inwin ? (uint32_t)step::field_index(G, T, lr, lc, bw) * 8u : kOOB);
          A2[j] = ld_f64x2(r_sA, valid ? g * 16u : kOOB);   // (wupd, surf)
          B2[j] = ld_f64x2(r_sB, valid ? g * 16u : kOOB);   // (velx, vely)
        }
      }
#pragma unroll
      for (int j = 0; j < KB; ++j) {
        const int k = kb + j;
        if (k < KT) {
          int i, lr, lc; uint32_t g; bool valid, inwin;
          cell(k, i, lr, lc, g, valid, inwin);
          const step::Candidate cb = step::candidate_bed<F32>(inwin, vb[j], vf[j], A2[j]);
          upd_bits |= cb.upd ? (1u << k) : 0u;
          if (cb.grounded) guard = 1;
          v_new[k] = cb.v;
          acc_old += ve[j];
          if (valid) {
            qx[i] = B2[j].x * cb.thick;
            qy[i] = B2[j].y * cb.thick;
          }
        }
      }
      asm volatile("" : "+v"(acc_old));   // pin the partial sum here (otherwise the adds sink to phase R and the
      __builtin_amdgcn_sched_barrier(0);   // loaded energies stay live across phase D)
    }
    __syncthreads();

    // ---- D: residual stencil on the flux tiles ---------------------------------------------------------
    double e_new[KT];
    double acc_new = 0.0;
    asm volatile("" : "+v"(ptid));
    const step::StepConsts SC{S.res, S.rcp_res, S.two_res, S.rcp_two_res};
    {
      double2 C2[KT];   // (dhdt_mc, smb) of the window cells
#pragma unroll
      for (int k = 0; k < KT; ++k) {
        int i, lr, lc; uint32_t g; bool valid, inwin;
        cell(k, i, lr, lc, g, valid, inwin);
        C2[k] = ld_f64x2(r_sC, inwin ? g * 16u : kOOB);
      }
#pragma unroll
      for (int k = 0; k < KT; ++k) {
        if (!slot_on(k)) { e_new[k] = 0.0; continue; }
        int i, lr, lc; uint32_t g; bool valid, inwin;
        cell(k, i, lr, lc, g, valid, inwin);
        const int r = T.hr0 + lr, c = T.hc0 + lc;
        const int il = (c == 0) ? i : i - 1, ir = (c == W - 1) ? i : i + 1;
        const int iu = (r == 0) ? i : i - tw, id = (r == H - 1) ? i : i + tw;
        double e = 0.0;
        if (inwin) e = step::flux_energy<FAST_DIV, F32, false>(qx[ir] - qx[il], qy[id] - qy[iu], ir - il == 2, id - iu == 2 * tw, C2[k], SC);
        e_new[k] = e;
        acc_new += e;
        if ((k & 1) == 1) __builtin_amdgcn_sched_barrier(0);
      }
    }

    // ---- R: reduce, decide (every thread evaluates the same numbers in the same order) ----------------
    {
      // one sum: the thread's change of energy, or +inf from a thread whose candidate grounds the ice (MCMC.py:1321-1329:
      // loss = inf); energies are never NaN (phase D), so an infinite total can only come from the guard
      double delta = acc_new - acc_old;
      if (guard) delta = INFINITY;
      const double w_delta = wave64_sum(delta);
      if (lane == 0) red[wave] = w_delta;
    }
    __syncthreads();
    const double sd = row16_sum(red[lane & 15]);
    double c_hi, c_lo, loss_next;          // this kernel divides plainly in both instantiations
    const bool acc = step::decide<false>(sd, sd == INFINITY, s_hi, s_lo, S.two_sigma2, S.rcp_two_sigma2, loss_prev, cur.u, c_hi, c_lo, loss_next);

    // ---- E: commit -------------------------------------------------------------------------------------
    if (acc) {
      asm volatile("" : "+v"(ptid));
#pragma unroll
      for (int k = 0; k < KT; ++k) {
        if (!slot_on(k)) continue;
        int i, lr, lc; uint32_t g; bool valid, inwin;
        cell(k, i, lr, lc, g, valid, inwin);
        const bool upd = (upd_bits >> k) & 1u;
        StateIO<TS>::store(r_en, inwin ? g * (uint32_t)sizeof(TS) : kOOB, e_new[k]);
        StateIO<TS>::store(r_bed, upd ? g * (uint32_t)sizeof(TS) : kOOB, v_new[k]);
        __builtin_amdgcn_raw_ptr_buffer_atomic_add_i32(1, r_rs, (int)(upd ? g * 4u : kOOB), 0, 0);
      }
      two_sum(c_hi, c_lo, s_hi, s_lo);
      loss_prev = loss_next;
    }
    if (tid == 0) step::write_record(a, rout, loss_prev, acc, cur.row, cur.col, bh, bw);
    // End of step.  LDS needs no barrier here: the tiles are rewritten only after every wave has passed the R barrier
    // (its stencil reads are done), and `red` only after the next A barrier.  The global stores of an accepted step must
    // be visible to the next step's loads only if the next halo window touches this window.
    if (acc && has_next && (unsigned)nxt.si < (unsigned)a.B.n_sizes) {
      if (step::halo_touches(step::clip_window(H, W, nxt.row, nxt.col, tab[2 * nxt.si], tab[2 * nxt.si + 1]), G)) __syncthreads();
    }
  }
  if (tid == 0) {
    a.loss_sum[2 * chain] = s_hi;
    a.loss_sum[2 * chain + 1] = s_lo;
  }
}

template <typename TS, int KT>
static hipError_t launch_flux_t(const StepArgs& a, hipStream_t st) {
  return launch_pair<step_flux_kernel<TS, KT, true>, step_flux_kernel<TS, KT, false>>(
      a.S.fast_div, 160 * 1024, dim3(a.n_chains), dim3(kNT), step_flux_lds_bytes(a.tile_cap), st, a);
}

bool step_flux_supported(const StepArgs& a) {
  return a.tile_cap <= 7 * kNT && step_flux_lds_bytes(a.tile_cap) <= 160 * 1024 && a.S.sA != nullptr &&
         (uint64_t)a.S.H * a.S.W * 16u < 0x80000000ull;
}

hipError_t launch_step_flux(const StepArgs& a, hipStream_t st) {
  if (!step_flux_supported(a)) return hipErrorInvalidValue;
  if (a.f32_state) {
    if (a.tile_cap <= 2 * kNT) return launch_flux_t<float, 2>(a, st);
    if (a.tile_cap <= 4 * kNT) return launch_flux_t<float, 4>(a, st);
    return launch_flux_t<float, 7>(a, st);
  }
  if (a.tile_cap <= 2 * kNT) return launch_flux_t<double, 2>(a, st);
  if (a.tile_cap <= 4 * kNT) return launch_flux_t<double, 4>(a, st);
  return launch_flux_t<double, 7>(a, st);
}

// Folded static operands of the flux kernel (see the header of this file).
__global__ __launch_bounds__(256) void pack_flux_static_kernel(const StaticFields S, double2* sA, double2* sB, double2* sC) {
  const int n = S.H * S.W;
  for (int g = blockIdx.x * 256 + threadIdx.x; g < n; g += gridDim.x * 256) {
    const double w = S.weight ? S.weight[g] : 1.0;
    sA[g] = make_double2(S.upd[g] ? w : __builtin_bit_cast(double, kNoUpdBits), S.surf[g]);
    sB[g] = make_double2(S.velx[g], S.vely[g]);
    sC[g] = make_double2(S.mc[g] == 1 ? S.dhdt[g] : __builtin_nan(""), S.smb[g]);
  }
}

hipError_t launch_pack_flux_static(const StaticFields& S, double2* sA, double2* sB, double2* sC, hipStream_t st) {
  int grid = (S.H * S.W + 255) / 256;
  if (grid > 2048) grid = 2048;
  hipLaunchKernelGGL(pack_flux_static_kernel, dim3(grid), dim3(256), 0, st, S, sA, sB, sC);
  return hipGetLastError();
}

}  // namespace gsm
