// Small-scale chain on gfx950, everything of an iteration but the block simulation (sgs_kernel.hip): the full-grid loss of the
// proposed bed and the thickness guard, the windowed state that replaces them without a transformer, the acceptance test, the
// commit, the tail launch that does all of that at once, the normal-score transform and the Philox draws.
//
// Replaces, for a batch of chains:
//   chain.loss on the proposed bed + thickness guard  MCMC.py:1781-1795 (loss :1021-1044, Topography.py:592-600)
//   the acceptance test and the commit                MCMC.py:1797-1812
//   nst_trans.transform / inverse_transform           MCMC.py:1766, :1777
#include "gsm_internal.h"
#include "device_util.h"
#include "residual_device.h"
#include "normal_score.h"
#include "proposal_device.h"
#include <math.h>

namespace gsm {

// ---- what every end of an iteration shares -----------------------------------------------------------------------------------
// the block window of a chain, win[4 chain ..] = r0, r1, c0, c1, on a grid of W columns
struct BlockWin {
  int r0, r1, c0, c1, W;
  __device__ __forceinline__ BlockWin(const int32_t* win, int chain, int W_) : r0(win[4 * chain]), r1(win[4 * chain + 1]), c0(win[4 * chain + 2]), c1(win[4 * chain + 3]), W(W_) {}
  __device__ __forceinline__ int cells() const { return (r1 - r0) * (c1 - c0); }
  __device__ __forceinline__ bool holds(int r, int c) const { return r >= r0 && r < r1 && c >= c0 && c < c1; }
  // cell p of the window (row-major) as an index of the chain's map
  __device__ __forceinline__ size_t flat(int p) const { const int ww = c1 - c0; return (size_t)(r0 + p / ww) * W + c0 + p % ww; }
};
// the Metropolis test (MCMC.py:1797-1801): a smaller loss is taken, another with probability min(1, exp(loss_prev - loss_next)),
// Python's built-in min as the reference calls it: a NaN exponential gives 1 (step_common.h decides the large-scale step likewise)
__device__ __forceinline__ bool metropolis_accept(double lp, double ln, double u) {       // lp, ln: the loss of the state and of the proposal
  if (lp > ln) return true;
  const double p = exp(lp - ln);
  return u <= fmin(1.0, p);                 // p NaN (a NaN loss, or inf - inf): Python's min(1, nan) is 1, the reference accepts
}
// Chain groups (gsm_sgs_set_groups; G of the kernels below): trend is [n_groups][H*W] and the transformer's tables are [n_groups][nq],
// each read at the chain's group.  Without groups (G = false) every kernel is the one it was.
template <bool G>
__device__ __forceinline__ const double* group_plane(const double* p, const int32_t* group, int chain, size_t stride) {
  return (G && p) ? p + (size_t)group[chain] * stride : p;
}
// the squared residual of cell g = (r, c) as it enters the loss: 0 where mc_mask != 1 or the residual is NaN (nansum)
template <class BedAt>
__device__ __forceinline__ double cell_energy(const StaticFields& S, int g, int r, int c, const BedAt& bed_at) {
  double e = 0.0;
  if (S.mc[g] == 1) {
    const double v = cell_residual(S, r, c, bed_at);
    if (!isnan(v)) e = v * v;
  }
  return e;
}
// accepted: the window goes from `next` to `cur` and its resampled counts are bumped (MCMC.py:1803-1812); else the window of
// `next` is restored from `cur`, so that next == cur everywhere again.  The three planes are the chain's.
__device__ __forceinline__ void commit_window(bool acc, double* cur, double* next, uint32_t* resampled, const BlockWin& win, int tid, int stride) {
  const int n = win.cells();
  for (int p = tid; p < n; p += stride) {
    const size_t q = win.flat(p);
    if (acc) { cur[q] = next[q]; resampled[q] += 1u; }
    else next[q] = cur[q];
  }
}
// an accepted whole-map commit bumps the window's resampled counts only
__device__ __forceinline__ void bump_window(uint32_t* resampled, const BlockWin& win, int tid, int stride) {
  const int n = win.cells();
  for (int p = tid; p < n; p += stride) resampled[win.flat(p)] += 1u;
}

// ---------------------------------------------------------------------------------------------------------------------
// loss of the proposed bed (+ trend) over the whole grid and the thickness guard, one 256-thread workgroup per chain:
//   loss = nansum(residual^2 where mc_mask == 1) / (2 sigma^2)      (MCMC.py:1021-1044 on Topography.py:592-600)
//   bad  = number of cells with guard_mask == 1 and surf - (bed + trend) <= 0   (MCMC.py:1789-1795)
// S.upd is the guard mask here (grounded_ice_mask); trend may be NULL.
// ---------------------------------------------------------------------------------------------------------------------
// Several workgroups per chain (a chain's grid is split into `parts` contiguous ranges of cells), then one thread per chain
// adds the parts in order: with one workgroup per chain a 256 x 256 grid kept 16 CUs busy for 0.19 ms per iteration.
// one part of a chain's map by the 256 threads of a workgroup; thread 0 returns the part's sum and bad-cell count
// (bed[q - off] is cell q of the chain's map: off != 0 when `bed` is a tile of the map in LDS)
__device__ __forceinline__ void sgs_loss_part(const StaticFields& S, const double* bed, const int off, const double* trend, int g_lo, int g_hi, int tid,
                                              double* red, int* redb, double& sum_out, int& bad_out) {
  auto bed_at = [&](int rr, int cc) { const int q = rr * S.W + cc; return trend ? bed[q - off] + trend[q] : bed[q - off]; };
  double hi = 0.0, lo = 0.0;
  int nbad = 0;
  for (int g = g_lo + tid; g < g_hi; g += 256) {
    const int r = g / S.W, c = g - r * S.W;
    const double e = cell_energy(S, g, r, c, bed_at);
    const double s = hi + e, bb = s - hi;
    lo += (hi - (s - bb)) + (e - bb);
    hi = s;
    if (S.upd[g] == 1 && (S.surf[g] - bed_at(r, c)) <= 0.0) ++nbad;
  }
  double t = hi + lo;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { t += __shfl_xor(t, off, 64); nbad += __shfl_xor(nbad, off, 64); }
  if ((tid & 63) == 0) { red[tid >> 6] = t; redb[tid >> 6] = nbad; }
  __syncthreads();
  sum_out = ((red[0] + red[1]) + red[2]) + red[3];
  bad_out = redb[0] + redb[1] + redb[2] + redb[3];
}
template <bool G>
__global__ __launch_bounds__(256) void sgs_loss_kernel(const StaticFields S, const double* beds, const double* trend, int parts,
                                                       double* part_sum, int32_t* part_bad, const int32_t* group) {
  __shared__ double red[8];
  __shared__ int redb[4];
  const int chain = blockIdx.x, part = blockIdx.y, tid = threadIdx.x;
  const int plane = S.H * S.W;
  const int per = (plane + parts - 1) / parts, g_lo = part * per, g_hi = min(plane, g_lo + per);
  double t; int nb;
  sgs_loss_part(S, beds + (size_t)chain * plane, 0, group_plane<G>(trend, group, chain, plane), g_lo, g_hi, tid, red, redb, t, nb);
  if (tid == 0) { part_sum[chain * parts + part] = t; part_bad[chain * parts + part] = nb; }
}
__global__ __launch_bounds__(64) void sgs_loss_finish_kernel(int n_chains, int parts, double two_sigma2, const double* __restrict__ part_sum,
                                                             const int32_t* __restrict__ part_bad, double* __restrict__ loss, int32_t* __restrict__ bad) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= n_chains) return;
  double s = 0.0;
  int nb = 0;
  for (int p = 0; p < parts; ++p) { s += part_sum[c * parts + p]; nb += part_bad[c * parts + p]; }
  loss[c] = s / two_sigma2;
  bad[c] = nb;
}

// parts of a chain's map: a function of the grid alone (a chain's loss must not depend on how many chains share the handle);
// ~1024 cells each, so that a few chains still spread over the chip (4 chains at 64 x 64: +6 % per iteration against 4096)
int sgs_loss_parts(const StaticFields& S) { return std::max(1, std::min(64, (S.H * S.W + 1023) / 1024)); }

hipError_t launch_sgs_loss(const StaticFields& S, int n_chains, const double* beds, const double* trend, double* loss, int32_t* bad,
                           double* part_sum, int32_t* part_bad, const int32_t* group, hipStream_t st) {
  const int parts = sgs_loss_parts(S);
  if (group) hipLaunchKernelGGL(sgs_loss_kernel<true>, dim3(n_chains, parts), dim3(256), 0, st, S, beds, trend, parts, part_sum, part_bad, group);
  else hipLaunchKernelGGL(sgs_loss_kernel<false>, dim3(n_chains, parts), dim3(256), 0, st, S, beds, trend, parts, part_sum, part_bad, group);
  hipLaunchKernelGGL(sgs_loss_finish_kernel, dim3((n_chains + 63) / 64), dim3(64), 0, st, n_chains, parts, S.two_sigma2, part_sum, part_bad, loss, bad);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// Windowed iteration end for chains WITHOUT a normal-score transformer (gsm.h: gsm_sgs_state_init / gsm_sgs_finish).  The
// reference recomputes residual, loss and guard over the whole map every iteration (MCMC.py:1781-1795); without a
// transformer only the block changes, so only the residuals of the block and its one-cell halo change (5-point stencil).
// Carried per chain: the plane of squared residuals that enter the loss (`energy`, 0 where mc_mask != 1 or the residual is
// NaN), their compensated sum, the loss, and the number of grounded cells with non-positive thickness.
//   state[4 c .. 4 c + 3] = (sum hi, sum lo, loss = sum / (2 sigma^2), bad cells)
// One 256-thread workgroup per chain: loss / guard of the proposal from the halo window, the acceptance test, the commit.
// ---------------------------------------------------------------------------------------------------------------------
template <bool G>
__global__ __launch_bounds__(256) void sgs_state_init_kernel(const StaticFields S, const double* beds, const double* trend_all, double* energy,
                                                             double* state, const int32_t* group) {
  __shared__ double red[8];
  __shared__ int redb[4];
  const int chain = blockIdx.x, tid = threadIdx.x;
  const int plane = S.H * S.W;
  const double* bed = beds + (size_t)chain * plane;
  const double* trend = group_plane<G>(trend_all, group, chain, plane);
  double* en = energy + (size_t)chain * plane;
  auto bed_at = [&](int rr, int cc) { const int q = rr * S.W + cc; return trend ? bed[q] + trend[q] : bed[q]; };
  double hi = 0.0, lo = 0.0;
  int nbad = 0;
  for (int g = tid; g < plane; g += 256) {
    const int r = g / S.W, c = g - r * S.W;
    const double e = cell_energy(S, g, r, c, bed_at);
    en[g] = e;
    double sm, er;
    dev::two_sum(hi, e, sm, er);
    hi = sm; lo += er;
    if (S.upd[g] == 1 && (S.surf[g] - bed_at(r, c)) <= 0.0) ++nbad;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double ohi = __shfl_xor(hi, off, 64), olo = __shfl_xor(lo, off, 64);
    double sm, er;
    dev::two_sum(hi, ohi, sm, er);
    hi = sm; lo += olo + er;
    nbad += __shfl_xor(nbad, off, 64);
  }
  if ((tid & 63) == 0) { red[2 * (tid >> 6)] = hi; red[2 * (tid >> 6) + 1] = lo; redb[tid >> 6] = nbad; }
  __syncthreads();
  if (tid == 0) {
    double th = 0.0, tl = 0.0;
    for (int w = 0; w < 4; ++w) { double sm, er; dev::two_sum(th, red[2 * w], sm, er); th = sm; tl += red[2 * w + 1] + er; }
    double sm, er;
    dev::two_sum(th, tl, sm, er);
    state[4 * chain] = sm; state[4 * chain + 1] = er; state[4 * chain + 2] = (sm + er) / S.two_sigma2;
    state[4 * chain + 3] = (double)(redb[0] + redb[1] + redb[2] + redb[3]);
  }
}

constexpr int kSgsHaloMax = 36 * 36;       // cells of block + halo held in LDS: blocks up to 34 x 34 (or e.g. 16 x 70)
template <bool G>
__global__ __launch_bounds__(256) void sgs_finish_kernel(const StaticFields S, double* cur, double* next, const double* trend_all, double* energy,
                                                         double* state, const int32_t* win, const double* u, uint32_t* resampled,
                                                         uint8_t* accept, double* loss_rec, uint8_t* acc_rec, int64_t rec_stride, int32_t* err,
                                                         const int32_t* group) {
  __shared__ double e_new[kSgsHaloMax];
  __shared__ double red[16];
  __shared__ int redb[8];
  __shared__ int acc_s;
  const int chain = blockIdx.x, tid = threadIdx.x;
  const int H = S.H, W = S.W;
  const size_t base = (size_t)chain * H * W;
  const double* trend = group_plane<G>(trend_all, group, chain, (size_t)H * W);
  const BlockWin bw(win, chain, W);
  const int hr0 = max(0, bw.r0 - 1), hr1 = min(H, bw.r1 + 1), hc0 = max(0, bw.c0 - 1), hc1 = min(W, bw.c1 + 1);
  const int hww = hc1 - hc0, hn = (hr1 - hr0) * hww;
  if (bw.r0 < 0 || bw.c0 < 0 || bw.r1 > H || bw.c1 > W || bw.r1 < bw.r0 || bw.c1 < bw.c0 || hn > kSgsHaloMax) {
    if (tid == 0) { atomicOr(err, kSgsFlagWindow); accept[chain] = 0; if (acc_rec) acc_rec[(int64_t)chain * rec_stride] = 0; if (loss_rec) loss_rec[(int64_t)chain * rec_stride] = state[4 * chain + 2]; }
    return;
  }
  const double* nb = next + base;
  auto next_at = [&](int rr, int cc) { const int q = rr * W + cc; return trend ? nb[q] + trend[q] : nb[q]; };
  // the halo's old and new sums as compensated pairs, like the carried sum they update: a plain sum here would leave its rounding
  // (up to the halo's share of the whole sum) in the carried pair at every accepted iteration, and those add up over a run
  double s_old = 0.0, l_old = 0.0, s_new = 0.0, l_new = 0.0;
  int bad_old = 0, bad_new = 0;
  for (int p = tid; p < hn; p += 256) {
    const int r = hr0 + p / hww, c = hc0 + p % hww, g = r * W + c;
    const double e = cell_energy(S, g, r, c, next_at);
    e_new[p] = e;
    double sm, er;
    dev::two_sum(s_new, e, sm, er); s_new = sm; l_new += er;
    dev::two_sum(s_old, energy[base + g], sm, er); s_old = sm; l_old += er;
    if (bw.holds(r, c) && S.upd[g] == 1) {
      const double t = trend ? trend[g] : 0.0;
      bad_new += (S.surf[g] - next_at(r, c)) <= 0.0;
      bad_old += (S.surf[g] - (trend ? cur[base + g] + t : cur[base + g])) <= 0.0;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double oso = __shfl_xor(s_old, off, 64), olo = __shfl_xor(l_old, off, 64), osn = __shfl_xor(s_new, off, 64), oln = __shfl_xor(l_new, off, 64);
    double sm, er;
    dev::two_sum(s_old, oso, sm, er); s_old = sm; l_old += olo + er;
    dev::two_sum(s_new, osn, sm, er); s_new = sm; l_new += oln + er;
    bad_old += __shfl_xor(bad_old, off, 64); bad_new += __shfl_xor(bad_new, off, 64);
  }
  if ((tid & 63) == 0) {
    const int w = tid >> 6;
    red[4 * w] = s_old; red[4 * w + 1] = l_old; red[4 * w + 2] = s_new; red[4 * w + 3] = l_new;
    redb[2 * w] = bad_old; redb[2 * w + 1] = bad_new;
  }
  __syncthreads();
  if (tid == 0) {
    const int bo = redb[0] + redb[2] + redb[4] + redb[6], bn = redb[1] + redb[3] + redb[5] + redb[7];
    double hi = state[4 * chain], lo = state[4 * chain + 1];
    double sm, er;
    for (int w = 0; w < 4; ++w) {                               // minus the halo's old energies, plus its new ones
      dev::two_sum(hi, -red[4 * w], sm, er); hi = sm; lo += er - red[4 * w + 1];
      dev::two_sum(hi, red[4 * w + 2], sm, er); hi = sm; lo += er + red[4 * w + 3];
    }
    dev::two_sum(hi, lo, sm, er); hi = sm; lo = er;
    const double bad_next = state[4 * chain + 3] - (double)bo + (double)bn;
    const double lp = state[4 * chain + 2];
    const double ln = (bad_next > 0.0) ? INFINITY : (hi + lo) / S.two_sigma2;
    const bool acc = metropolis_accept(lp, ln, u[chain]);
    if (acc) { state[4 * chain] = hi; state[4 * chain + 1] = lo; state[4 * chain + 2] = ln; state[4 * chain + 3] = bad_next; }
    accept[chain] = acc ? 1 : 0;
    if (loss_rec) loss_rec[(int64_t)chain * rec_stride] = acc ? ln : lp;
    if (acc_rec) acc_rec[(int64_t)chain * rec_stride] = acc ? 1 : 0;
    acc_s = acc ? 1 : 0;
  }
  __syncthreads();
  const bool acc = acc_s != 0;
  if (acc) for (int p = tid; p < hn; p += 256) energy[base + (size_t)(hr0 + p / hww) * W + hc0 + p % hww] = e_new[p];
  commit_window(acc, cur + base, next + base, resampled + base, bw, tid, 256);
}

hipError_t launch_sgs_state_init(const StaticFields& S, int n_chains, const double* beds, const double* trend, double* energy, double* state,
                                 const int32_t* group, hipStream_t st) {
  if (group) hipLaunchKernelGGL(sgs_state_init_kernel<true>, dim3(n_chains), dim3(256), 0, st, S, beds, trend, energy, state, group);
  else hipLaunchKernelGGL(sgs_state_init_kernel<false>, dim3(n_chains), dim3(256), 0, st, S, beds, trend, energy, state, group);
  return hipGetLastError();
}
hipError_t launch_sgs_finish(const StaticFields& S, int n_chains, double* cur, double* next, const double* trend, double* energy, double* state,
                             const int32_t* win, const double* u, uint32_t* resampled, uint8_t* accept, double* loss_rec, uint8_t* acc_rec,
                             int64_t rec_stride, int32_t* err, const int32_t* group, hipStream_t st) {
  if (group) hipLaunchKernelGGL(sgs_finish_kernel<true>, dim3(n_chains), dim3(256), 0, st, S, cur, next, trend, energy, state, win, u, resampled, accept,
                                loss_rec, acc_rec, rec_stride, err, group);
  else hipLaunchKernelGGL(sgs_finish_kernel<false>, dim3(n_chains), dim3(256), 0, st, S, cur, next, trend, energy, state, win, u, resampled, accept,
                          loss_rec, acc_rec, rec_stride, err, group);
  return hipGetLastError();
}

// the acceptance test of an iteration (gsm.h: gsm_sgs_decide), one thread per chain
__global__ __launch_bounds__(64) void sgs_decide_kernel(int n, const double* __restrict__ loss_next, const int32_t* __restrict__ bad,
                                                        const double* __restrict__ u, double* __restrict__ loss_prev,
                                                        uint8_t* __restrict__ accept, double* loss_rec, uint8_t* acc_rec, int64_t rec_stride) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= n) return;
  const double ln = (bad[c] > 0) ? INFINITY : loss_next[c];
  const double lp = loss_prev[c];
  const bool acc = metropolis_accept(lp, ln, u[c]);
  const double l = acc ? ln : lp;
  loss_prev[c] = l;
  accept[c] = acc ? 1 : 0;
  if (loss_rec) loss_rec[(int64_t)c * rec_stride] = l;
  if (acc_rec) acc_rec[(int64_t)c * rec_stride] = acc ? 1 : 0;
}

hipError_t launch_sgs_decide(int n_chains, const double* loss_next, const int32_t* bad, const double* u, double* loss_prev,
                             uint8_t* accept, double* loss_rec, uint8_t* acc_rec, int64_t rec_stride, hipStream_t st) {
  hipLaunchKernelGGL(sgs_decide_kernel, dim3((n_chains + 63) / 64), dim3(64), 0, st, n_chains, loss_next, bad, u, loss_prev, accept,
                     loss_rec, acc_rec, rec_stride);
  return hipGetLastError();
}

// Philox mode: the draws of one iteration of one chain (gsm.h: gsm_sgs_draw_philox), one 64-lane workgroup per (iteration, chain)
constexpr uint32_t kStreamSgs = 4;
__global__ __launch_bounds__(64) void sgs_draw_kernel(const SgsDrawArgs a) {
  __shared__ double mt[kMathTabDoubles];
  __shared__ uint32_t key[kSgsMaxWin];
  __shared__ int geo[8];
  const int chain = blockIdx.x, j = blockIdx.y, lane = threadIdx.x;
  const int64_t rec = (int64_t)j * a.n_chains + chain, it = a.iter0 + j;
  const uint64_t seed = a.seeds[chain];
  for (int i = lane; i < kMathTabDoubles; i += 64) mt[i] = a.mathtab[i];
  if (lane == 0) {
    int row = 0, col = 0;
    for (int att = 0; att < 64; ++att) {
      const u32x4 r = philox_draw(seed, it, kStreamSgs, (uint32_t)att);
      row = (int)__umulhi(r.x, (uint32_t)a.H); col = (int)__umulhi(r.y, (uint32_t)a.W);
      if (!a.region_mask || a.region_mask[row * a.W + col] == 1) break;
      if (att == 63) atomicOr(a.err, kSgsFlagNoCentre);
    }
    const u32x4 r = philox_draw(seed, it, kStreamSgs, 64u);
    const int bsx = a.min_x + (int)__umulhi(r.x, (uint32_t)(a.max_x - a.min_x));
    const int bsy = a.min_y + (int)__umulhi(r.y, (uint32_t)(a.max_y - a.min_y));
    // int(ix -/+ bs / 2) of MCMC.py:1758-1761 (truncation towards zero of a half-integer)
    const int r0 = max(0, (2 * row - bsx) / 2), r1 = min(a.H, (2 * row + bsx) / 2);
    const int c0 = max(0, (2 * col - bsy) / 2), c1 = min(a.W, (2 * col + bsy) / 2);
    a.win[4 * rec] = r0; a.win[4 * rec + 1] = r1; a.win[4 * rec + 2] = c0; a.win[4 * rec + 3] = c1;
    a.blk[4 * rec] = row; a.blk[4 * rec + 1] = col; a.blk[4 * rec + 2] = bsx; a.blk[4 * rec + 3] = bsy;
    a.u[rec] = u01_from(r.z, r.w);
    geo[0] = r0; geo[1] = r1; geo[2] = c0; geo[3] = c1;
  }
  __syncthreads();
  const int r0 = geo[0], r1 = geo[1], c0 = geo[2], c1 = geo[3];
  const int ww = c1 - c0, n = max(0, r1 - r0) * max(0, ww);
  if (lane == 0) { a.cell_off[rec] = (int32_t)(rec * a.max_cells); a.cell_cnt[rec] = (n <= a.max_cells && n <= kSgsMaxWin) ? n : 0; }
  if (n > a.max_cells || n > kSgsMaxWin) { if (lane == 0) atomicOr(a.err, kSgsFlagWindow); return; }
  for (int p = lane; p < n; p += 64) key[p] = philox_draw(seed, it, kStreamSgs, 128u + (uint32_t)p).x;
  __syncthreads();
  for (int p = lane; p < n; p += 64) {
    const uint32_t kp = key[p];
    int rank = 0;
    for (int q = 0; q < n; ++q) { const uint32_t kq = key[q]; rank += (kq < kp || (kq == kp && q < p)) ? 1 : 0; }
    const int i = r0 + p / ww, jj = c0 + p % ww;
    const int64_t o = rec * a.max_cells + rank;
    a.cells[2 * o] = i; a.cells[2 * o + 1] = jj;
    double g1, g2;
    normals2(seed, it, kStreamSgs, 2048u + (uint32_t)(p >> 1), g1, g2, mt);
    a.z[o] = a.is_data[i * a.W + jj] ? 0.0 : ((p & 1) ? g2 : g1);
  }
}
hipError_t launch_sgs_draw(const SgsDrawArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(sgs_draw_kernel, dim3(a.n_chains, a.n_iters), dim3(64), 0, st, a);
  return hipGetLastError();
}

// normal-score transform, elementwise (gsm.h: gsm_qt_transform); the two tables are staged in LDS when they fit
constexpr int kQtLds = 4096;
__global__ __launch_bounds__(256) void qt_kernel(const double* __restrict__ quantiles, const double* __restrict__ references, int nq,
                                                 double clip_min, double clip_max, const double* x, double* out, int64_t n, int inverse) {
  __shared__ double tab[2 * kQtLds];
  const double* q = quantiles;
  const double* ref = references;
  if (nq <= kQtLds) {
    for (int i = threadIdx.x; i < nq; i += 256) { tab[i] = quantiles[i]; tab[kQtLds + i] = references[i]; }
    __syncthreads();
    q = tab; ref = tab + kQtLds;
  }
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    out[i] = inverse ? ns::qt_inverse(x[i], q, ref, nq) : ns::qt_forward(x[i], q, ref, nq, clip_min, clip_max);
}
hipError_t launch_qt(const double* quantiles, const double* references, int nq, double clip_min, double clip_max, const double* x,
                     double* out, int64_t n, int inverse, hipStream_t st) {
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(qt_kernel, dim3(blocks), dim3(256), 0, st, quantiles, references, nq, clip_min, clip_max, x, out, n, inverse);
  return hipGetLastError();
}

// the same for chains in groups: chain blockIdx.y with the tables of its group (the same functions on the same table values, LDS or not
// by the same rule: an element's result is the one qt_kernel gives with that group's tables)
__global__ __launch_bounds__(256) void qt_groups_kernel(const double* __restrict__ quantiles, const double* __restrict__ references, int nq,
                                                        double clip_min, double clip_max, const double* x, double* out, int plane,
                                                        const int32_t* __restrict__ group, int inverse) {
  __shared__ double tab[2 * kQtLds];
  const int chain = blockIdx.y;
  const double* q = quantiles + (size_t)group[chain] * nq;
  const double* ref = references + (size_t)group[chain] * nq;
  if (nq <= kQtLds) {
    for (int i = threadIdx.x; i < nq; i += 256) { tab[i] = q[i]; tab[kQtLds + i] = ref[i]; }
    __syncthreads();
    q = tab; ref = tab + kQtLds;
  }
  const size_t base = (size_t)chain * plane;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < plane; i += gridDim.x * 256)
    out[base + i] = inverse ? ns::qt_inverse(x[base + i], q, ref, nq) : ns::qt_forward(x[base + i], q, ref, nq, clip_min, clip_max);
}
hipError_t launch_qt_groups(const double* quantiles, const double* references, int nq, double clip_min, double clip_max, const double* x,
                            double* out, int n_chains, int plane, const int32_t* group, int inverse, hipStream_t st) {
  const int blocks = std::max(1, std::min((plane + 255) / 256, 4096 / std::max(1, std::min(n_chains, 4096))));
  hipLaunchKernelGGL(qt_groups_kernel, dim3(blocks, n_chains), dim3(256), 0, st, quantiles, references, nq, clip_min, clip_max, x, out, plane,
                     group, inverse);
  return hipGetLastError();
}

// gsm_sgs_commit_map: an accepted chain takes the whole proposed plane
__global__ __launch_bounds__(256) void sgs_commit_map_kernel(int H, int W, double* cur, const double* proposed, uint32_t* resampled,
                                                             const int32_t* win, const uint8_t* accept) {
  const int chain = blockIdx.x;
  if (!accept[chain]) return;
  const size_t base = (size_t)chain * H * W;
  for (int p = threadIdx.x; p < H * W; p += 256) cur[base + p] = proposed[base + p];
  bump_window(resampled + base, BlockWin(win, chain, W), threadIdx.x, 256);
}
hipError_t launch_sgs_commit_map(int H, int W, int n_chains, double* cur, const double* proposed, uint32_t* resampled, const int32_t* win,
                                 const uint8_t* accept, hipStream_t st) {
  hipLaunchKernelGGL(sgs_commit_map_kernel, dim3(n_chains), dim3(256), 0, st, H, W, cur, proposed, resampled, win, accept);
  return hipGetLastError();
}

// accept[c] != 0: the block of chain c goes from `next` to `cur` and its resampled counts are bumped (MCMC.py:1803-1812);
// else the block of `next` is restored from `cur`, so that next == cur everywhere again.
__global__ __launch_bounds__(64) void sgs_commit_kernel(int H, int W, double* cur, double* next, uint32_t* resampled, const int32_t* win,
                                                        const uint8_t* accept) {
  const int chain = blockIdx.x;
  const size_t base = (size_t)chain * H * W;
  commit_window(accept[chain] != 0, cur + base, next + base, resampled + base, BlockWin(win, chain, W), threadIdx.x, 64);
}

hipError_t launch_sgs_commit(int H, int W, int n_chains, double* cur, double* next, uint32_t* resampled, const int32_t* win,
                             const uint8_t* accept, hipStream_t st) {
  hipLaunchKernelGGL(sgs_commit_kernel, dim3(n_chains), dim3(64), 0, st, H, W, cur, next, resampled, win, accept);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// The end of an iteration of gsm_sgs_iterate in ONE launch: loss parts as sgs_loss_kernel; the workgroup of a chain that
// finishes last (a ticket per chain, device-scope fences) adds the parts in order (= sgs_loss_finish_kernel), takes the
// decision (= sgs_decide_kernel) and commits (mode 1 = sgs_commit_map_kernel: `beds` is the proposed plane; mode 2 =
// sgs_commit_kernel: `beds` is `next`).  Four launches of ~5 us each at 4 chains become one.  The ticket resets itself.
// ---------------------------------------------------------------------------------------------------------------------
// QT (mode 1 only; tables of <= kTailQt entries, parts of <= kTailTile cells with their two halo rows): `beds` (the proposed plane) is not
// read but MADE here -- every workgroup inverse-transforms its part of `next` and one row either side into LDS (qt_kernel's arithmetic:
// the same functions on the same table values), stores its own part, and scores from LDS -- and so is the NEXT iteration's forward transform:
// the part's T(proposed) goes to `next_acc`; the chain's last workgroup copies it to `next` if the proposal is accepted (cur = proposed,
// so T(cur) = T(proposed)) and otherwise re-transforms the block window of `cur` (everything else of `next` still is T(cur)).  Two
// elementwise launches per iteration less (MCMC.py:1766, :1777 stay where they are in the arithmetic).
constexpr int kTailQt = 1024, kTailTile = 2048;
template <bool QT, bool G>
__global__ __launch_bounds__(256) void sgs_loss_tail_kernel(const StaticFields S, const SgsTailArgs a) {
  __shared__ double red[8];
  __shared__ int redb[4];
  __shared__ int s_last, s_acc;
  __shared__ double qtab[QT ? 2 * kTailQt : 1];
  __shared__ double tile[QT ? kTailTile : 1];
  const int chain = blockIdx.x, part = blockIdx.y, tid = threadIdx.x;
  const int H = S.H, W = S.W, plane = H * W, parts = a.parts;
  const int per = (plane + parts - 1) / parts, g_lo = part * per, g_hi = min(plane, g_lo + per);
  const size_t base = (size_t)chain * plane;
  const double* bed = a.beds + base;
  const double* trend = group_plane<G>(a.trend, a.group, chain, plane);
  int off = 0;
  if (QT) {
    const double* tq = group_plane<G>(a.qt_q, a.group, chain, a.qt_n);
    const double* tref = group_plane<G>(a.qt_ref, a.group, chain, a.qt_n);
    for (int i = tid; i < a.qt_n; i += 256) { qtab[i] = tq[i]; qtab[kTailQt + i] = tref[i]; }
    __syncthreads();
    const int lo_h = max(0, g_lo - W), hi_h = min(plane, g_hi + W);
    for (int idx = lo_h + tid; idx < hi_h; idx += 256) {
      const double v = ns::qt_inverse(a.next[base + idx], qtab, qtab + kTailQt, a.qt_n);
      tile[idx - lo_h] = v;
      if (idx >= g_lo && idx < g_hi) {
        a.beds[base + idx] = v;
        a.next_acc[base + idx] = ns::qt_forward(v, qtab, qtab + kTailQt, a.qt_n, a.clip_min, a.clip_max);
      }
    }
    __syncthreads();
    bed = tile; off = lo_h;
  }
  double t; int nb;
  sgs_loss_part(S, bed, off, trend, g_lo, g_hi, tid, red, redb, t, nb);
  if (tid == 0) {
    __hip_atomic_store(&a.part_sum[chain * parts + part], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&a.part_bad[chain * parts + part], nb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int ticket = __hip_atomic_fetch_add(&a.ticket[chain], 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    s_last = ticket == parts - 1;
  }
  __syncthreads();
  if (!s_last) return;
  if (tid == 0) {
    double s = 0.0;
    int nbad = 0;
    for (int p = 0; p < parts; ++p) {
      s += __hip_atomic_load(&a.part_sum[chain * parts + p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      nbad += __hip_atomic_load(&a.part_bad[chain * parts + p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    a.ticket[chain] = 0;
    const double loss = s / S.two_sigma2;
    a.loss[chain] = loss; a.bad[chain] = nbad;
    const double ln = (nbad > 0) ? INFINITY : loss;
    const double lp = a.loss_prev[chain];
    const bool acc = metropolis_accept(lp, ln, a.u[chain]);
    const double l = acc ? ln : lp;
    a.loss_prev[chain] = l;
    a.accept[chain] = acc ? 1 : 0;
    if (a.loss_rec) a.loss_rec[(int64_t)chain * a.rec_stride] = l;
    if (a.acc_rec) a.acc_rec[(int64_t)chain * a.rec_stride] = acc ? 1 : 0;
    s_acc = acc ? 1 : 0;
  }
  __syncthreads();
  const bool acc = s_acc != 0;
  const BlockWin bw(a.win, chain, W);
  if (QT) {
    // the other workgroups' parts of `beds` and `next_acc` were stored before their tickets (release); thread 0 took the last ticket (acquire)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (acc) {
      for (int p = tid; p < plane; p += 256) { a.cur[base + p] = a.beds[base + p]; a.next[base + p] = a.next_acc[base + p]; }
      bump_window(a.resampled + base, bw, tid, 256);
    } else {
      for (int p = tid; p < bw.cells(); p += 256) {
        const size_t q = base + bw.flat(p);
        a.next[q] = ns::qt_forward(a.cur[q], qtab, qtab + kTailQt, a.qt_n, a.clip_min, a.clip_max);
      }
    }
  } else if (a.mode == 1) {
    if (!acc) return;
    for (int p = tid; p < plane; p += 256) a.cur[base + p] = a.beds[base + p];
    bump_window(a.resampled + base, bw, tid, 256);
  } else {
    commit_window(acc, a.cur + base, a.beds + base, a.resampled + base, bw, tid, 256);
  }
}
// whether the tail launch can make the two transforms of an iteration as well (sgs_loss_tail_kernel<true>)
bool sgs_tail_takes_qt(const StaticFields& S, int nq) {
  const int plane = S.H * S.W, parts = sgs_loss_parts(S), per = (plane + parts - 1) / parts;
  return nq >= 1 && nq <= kTailQt && per + 2 * S.W <= kTailTile;
}
hipError_t launch_sgs_loss_tail(const StaticFields& S, int n_chains, const SgsTailArgs& args, hipStream_t st) {
  SgsTailArgs a = args;
  a.parts = sgs_loss_parts(S);
  if (a.qt_q) {
    if (a.mode != 1 || !sgs_tail_takes_qt(S, a.qt_n) || !a.next || !a.next_acc) return hipErrorInvalidValue;
    if (a.group) hipLaunchKernelGGL((sgs_loss_tail_kernel<true, true>), dim3(n_chains, a.parts), dim3(256), 0, st, S, a);
    else hipLaunchKernelGGL((sgs_loss_tail_kernel<true, false>), dim3(n_chains, a.parts), dim3(256), 0, st, S, a);
  } else if (a.group)
    hipLaunchKernelGGL((sgs_loss_tail_kernel<false, true>), dim3(n_chains, a.parts), dim3(256), 0, st, S, a);
  else
    hipLaunchKernelGGL((sgs_loss_tail_kernel<false, false>), dim3(n_chains, a.parts), dim3(256), 0, st, S, a);
  return hipGetLastError();
}

}  // namespace gsm
