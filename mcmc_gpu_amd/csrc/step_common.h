// What the five Metropolis step kernels (step_kernel, step_flux_kernel, chain_fused_kernel, step_strip_kernel,
// chain_strip_kernel) must have in common, stated once: the integer geometry of a step, the per-cell arithmetic, the accept
// test, the replay record protocol and the constant-address helpers.  Reference: gstatsMCMC/MCMC.py:1263-1360,
// Topography.py:592-600.  Where operands live, how loads are batched and in which order a kernel sums are the kernels' own
// (measured) choices and stay in their files.  The geometry is __host__ __device__: tests/native/strip_geometry_check.cpp
// runs it on the host.
#pragma once
#include "gsm_internal.h"
#include "device_util.h"
#include <math.h>

namespace gsm {
namespace step {

using namespace dev;

// ---- 1. geometry ---------------------------------------------------------------------------------------------------------
// window of a step, clipped to the grid, and the matching sub-block of the proposal field f (MCMC.py:1266-1276)
struct Window {
  int r0, r1, c0, c1;      // window rows / cols [r0, r1) x [c0, c1)
  int mr0, mc0;            // first row / col of the block that lies inside the grid
  int wh, ww;              // window size
};
__host__ __device__ __forceinline__ Window clip_window(int H, int W, int row, int col, int bh, int bw) {
  Window g;
  g.r0 = max(0, row - bh / 2); g.r1 = min(H, row + bh / 2);
  g.c0 = max(0, col - bw / 2); g.c1 = min(W, col + bw / 2);
  g.mr0 = max(bh - g.r1, 0); g.mc0 = max(bw - g.c1, 0);
  g.wh = g.r1 - g.r0; g.ww = g.c1 - g.c0;
  return g;
}
// a halo ring on all four sides lies inside the grid: no window cell touches a grid border, every difference is central
__host__ __device__ __forceinline__ bool interior(int H, int W, const Window& g) {
  return (g.r0 > 0) && (g.r1 < H) && (g.c0 > 0) && (g.c1 < W);
}

// the window plus its 1-cell halo, clipped to the grid (MCMC.py:1293-1297), as a row-major tile
struct HaloTile {
  int hr0, hr1, hc0, hc1;  // tile rows / cols
  int tw, ncell;           // tile width, tile cells
  int dr, dc;              // window origin inside the tile (0 or 1)
};
__host__ __device__ __forceinline__ HaloTile halo_tile(int H, int W, const Window& g) {
  HaloTile t;
  t.hr0 = max(0, g.r0 - 1); t.hr1 = min(H, g.r1 + 1);
  t.hc0 = max(0, g.c0 - 1); t.hc1 = min(W, g.c1 + 1);
  t.tw = t.hc1 - t.hc0;
  t.ncell = (t.hr1 - t.hr0) * t.tw;
  t.dr = g.r0 - t.hr0; t.dc = g.c0 - t.hc0;
  return t;
}
// tile width of the step with centre column `col` and block width bw: the divisor behind PropScalars::m_tw, which
// chain_fused_kernel takes from the record instead of dividing (at least 1, so that the record of a stand-in step is defined)
__host__ __device__ __forceinline__ int halo_tile_width(int W, int col, int bw) {
  const int c0 = max(0, col - bw / 2), c1 = min(W, col + bw / 2);
  return max(1, min(W, c1 + 1) - max(0, c0 - 1));
}
// Does the halo window of step `reader` touch the window `written`?  It is what makes the un-fenced stores of an accepted
// step safe: only then must they have landed before `reader` loads.  The halo is taken unclipped; against a window inside
// the grid that changes nothing.  An empty `written` (all zero: "the step before was rejected") touches nothing, except that
// a reader clipped at the grid's top left corner reports a touch -- a wait, never a missed one.
__host__ __device__ __forceinline__ bool halo_touches(const Window& reader, const Window& written) {
  return (reader.r0 - 1 < written.r1) && (written.r0 < reader.r1 + 1) && (reader.c0 - 1 < written.c1) && (written.c0 < reader.c1 + 1);
}

// tile row / col of a cell inside the window
__host__ __device__ __forceinline__ bool in_window(const Window& g, const HaloTile& t, int lr, int lc) {
  return (unsigned)(lr - t.dr) < (unsigned)g.wh && (unsigned)(lc - t.dc) < (unsigned)g.ww;
}
// index of that window cell in the bh x bw proposal field
__host__ __device__ __forceinline__ int field_index(const Window& g, const HaloTile& t, int lr, int lc, int bw) {
  return (g.mr0 + lr - t.dr) * bw + g.mc0 + lc - t.dc;
}

// ---- 2. cell arithmetic --------------------------------------------------------------------------------------------------
// Candidate bed of a cell (MCMC.py:1279-1290) and its thickness guard (MCMC.py:1321-1329).  A2 = (wupd, surf) of the packed
// static operands: wupd is the crf weight where update_mask is set, else the tagged NaN kNoUpdBits.  F32 state: the candidate
// is rounded to float BEFORE it is used, so that the carried sum equals the sum of what is stored.
struct Candidate {
  double v, thick;         // candidate bed, ice thickness above it
  bool upd, grounded;      // the cell takes the update; ... and its candidate leaves no ice (the step's loss is infinite)
};
template <bool F32>
__device__ __forceinline__ Candidate candidate_bed(const bool inwin, const double bed, const double f, const double2 A2) {
  Candidate c;
  c.upd = inwin && (__builtin_bit_cast(uint64_t, A2.x) != kNoUpdBits);
  c.v = bed;
  if (c.upd) {
    c.v = c.v + f * A2.x;
    if (F32) c.v = (double)(float)c.v;
  }
  c.thick = A2.y - c.v;
  c.grounded = c.upd && c.thick <= 0.0;
  return c;
}

struct StepConsts { double res, rcp_res, two_res, rcp_two_res; };

// Flux differences of a cell -> its energy (Topography.py:592-600 with np.gradient's rules: central difference over 2h,
// one-sided over h at a grid border; chain.loss, MCMC.py:1021-1044: a NaN residual does not count).  C2 = (dhdt_mc, smb).
// INTERIOR: both differences are central and K.res is not read.  `counted` false: the lane holds no cell of its own here.
template <bool FAST_DIV, bool F32, bool INTERIOR>
__device__ __forceinline__ double flux_energy(const double ddx, const double ddy, const bool x_central, const bool y_central, const double2 C2,
                                              const StepConsts& K, const bool counted = true) {
  double dx, dy;
  if (INTERIOR) {
    if (FAST_DIV) { dx = exact_div(ddx, K.two_res, K.rcp_two_res); dy = exact_div(ddy, K.two_res, K.rcp_two_res); }
    else { dx = ddx / K.two_res; dy = ddy / K.two_res; }
  } else if (FAST_DIV) {
    dx = x_central ? exact_div(ddx, K.two_res, K.rcp_two_res) : exact_div(ddx, K.res, K.rcp_res);
    dy = y_central ? exact_div(ddy, K.two_res, K.rcp_two_res) : exact_div(ddy, K.res, K.rcp_res);
  } else {
    dx = ddx / (x_central ? K.two_res : K.res);
    dy = ddy / (y_central ? K.two_res : K.res);
  }
  const double v = ((dx + dy) + C2.x) - C2.y;
  double e = 0.0;
  if (counted && !isnan(v)) e = v * v;
  if (F32) e = (double)(float)e;
  return e;
}

// ---- 3. accept test ------------------------------------------------------------------------------------------------------
// Accept test of a step (MCMC.py:1331-1336) on the carried compensated sum (s_hi, s_lo) and the step's change of energy sd:
// every thread evaluates the same numbers.  grounded: some candidate cell leaves no ice, the loss is infinite.  FAST_DIV
// selects the form of the division by 2 sigma^2 (the same quotient either way).  After an accept the caller carries
// two_sum(c_hi, c_lo) and loss_next on.
template <bool FAST_DIV>
__device__ __forceinline__ bool decide(const double sd, const bool grounded, const double s_hi, const double s_lo, const double two_sigma2,
                                       const double rcp_two_sigma2, const double loss_prev, const double u, double& c_hi, double& c_lo,
                                       double& loss_next) {
  double c_err;
  two_sum(s_hi, sd, c_hi, c_err);
  c_lo = s_lo + c_err;
  loss_next = FAST_DIV ? exact_div(c_hi + c_lo, two_sigma2, rcp_two_sigma2) : (c_hi + c_lo) / two_sigma2;
  if (grounded) loss_next = INFINITY;
  // every thread holds the same numbers: a scalar branch skips the exponential of a downhill step
  double p_acc = 1.0;
  if (!__builtin_amdgcn_readfirstlane((int)(loss_prev > loss_next))) p_acc = fmin(1.0, exp(loss_prev - loss_next));
  return u <= p_acc;
}

// ---- 4. records ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t record_index(const StepArgs& a, int chain, int s) { return (int64_t)chain * a.rec_stride + a.rec_offset + s; }
// what a step leaves behind (one thread): the loss after it, the decision, and optionally its block
__device__ __forceinline__ void write_record(const StepArgs& a, int64_t rout, double loss, bool acc, int row, int col, int bh, int bw) {
  a.loss[rout] = loss;
  a.accept[rout] = acc ? 1 : 0;
  if (a.blocks) { a.blocks[4 * rout] = row; a.blocks[4 * rout + 1] = col; a.blocks[4 * rout + 2] = bh; a.blocks[4 * rout + 3] = bw; }
}
// Replay: the proposal of input record r.  The kernels read it one step ahead (the end-of-step fence needs the next window
// before the step ends).
struct ReplayRec { int si, row, col; double u; };
__device__ __forceinline__ ReplayRec read_replay(const StepArgs& a, int64_t r) {
  return ReplayRec{a.size_idx[r], a.centre[2 * r], a.centre[2 * r + 1], a.u[r]};
}
__device__ __forceinline__ bool replay_valid(const StepArgs& a, const ReplayRec& q) {
  return !(q.si < 0 || q.si >= a.B.n_sizes || q.row < 0 || q.row >= a.S.H || q.col < 0 || q.col >= a.S.W);
}
// a record that is out of range: flag it, leave the chain as it is (one thread)
__device__ __forceinline__ void reject_record(const StepArgs& a, int64_t rout, double loss_prev, const ReplayRec& q) {
  atomicExch(a.err_flag, 1);
  write_record(a, rout, loss_prev, false, q.row, q.col, 0, 0);
}

// ---- 5. kernel arguments and records through the constant address space -------------------------------------------------
// The address is uniform and the memory is never written by the kernel, so every access is a scalar load.  The fused kernels
// re-read the few fields a phase needs through a laundered pointer instead of keeping the kernel arguments and the step's
// record (and everything derived from them) in SGPRs for the whole step: they have far more uniform values than scalar
// registers, and a spilled SGPR comes back through v_readlane, a VECTOR instruction (round 1 of
// chain_fused_kernel: ~8 % of the vector instructions of a step were such reloads).
template <class T> using cptr_t = const __attribute__((address_space(4))) T*;
typedef cptr_t<PropScalars> crec_t;      // a step's record (propose_scalars_kernel's output)
template <class A>
__device__ __forceinline__ cptr_t<A> kargs() {
  cptr_t<A> p = (cptr_t<A>)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return p;
}
// copy of a struct that lives in the constant address space (device pass only: the host pass never runs this code)
template <class T>
__device__ __forceinline__ T load_c(cptr_t<T> p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return *p;
#else
  (void)p;
  return T();
#endif
}

}  // namespace step
}  // namespace gsm
