// interpolate.sgs on gfx950: sequential Gaussian simulation of whole grids, many realisations per call.
//
// Replaces, for a batch of realisations:
//   sgs                       gstatsMCMC/gstatsim_custom/interpolate.py:92-191 (cell loop :132-189, radius widening :150-157,
//                             truncated-normal draw :173-187)
//   neighbors (octant search) gstatsMCMC/gstatsim_custom/neighbors.py:4-64
//   ok_solve / sk_solve       gstatsMCMC/gstatsim_custom/_krige.py:5-81
//
// The random numbers are the caller's (NumPy on the host, in the reference's order): each realisation's visiting order
// (rng.shuffle) and one number per path cell -- a standard normal (rng.normal(est, sd) = est + sd * z) or, with bounds, a
// uniform (truncnorm.rvs = truncnorm.ppf(u, a, b) * scale + est, truncnorm.h).
//
// The block kernels' split (sgs_kernel.hip) carries over: a cell's neighbour set and kriging weights depend only on WHICH
// cells hold a value when it is visited, never on the values.
//   sgs_grid_rank_kernel / sgs_grid_slot_kernel  per realisation the visiting rank of every cell, int32 [R][H*W]: -1 for a
//                        conditioning value, the slot for a path cell, INT32_MAX for a NaN cell that is never filled (outside
//                        sim_mask);
//   sgs_grid_weights_kernel  one wavefront per (realisation, path slot) of a segment, all side by side: the ring search with its
//                        radius widening (a cell qualifies when its rank is below the slot), then the kriging system and its
//                        Gauss-Jordan solve -- both sgs_search.h's, shared with the block kernel -> a record per cell.
//                        sgs_grid_weights_local_kernel is the same pass with a variogram per cell (interpolate.py:141-147).
//                        A neighbour is either a value (conditioning data, or a path cell whose bounds coincide) or an
//                        earlier path cell, NaN-boxed (slot << 25 | cell); no simulated value is read, so a segment's
//                        records do not wait for the values before it;
//   sgs_grid_values_kernel   one workgroup of four waves per realisation walks the segment's slots in 64-cell chunks, as
//                        sgs_sequence_kernel does: the four waves gather each cell's known part (values of earlier chunks come
//                        from the realisation's grid in global memory, written by wave 0 of the same workgroup before the
//                        chunk's barrier); coefficients of cells of the same chunk go to a 64 x 64 LDS tile; wave 0 then
//                        finishes the cells one by one -- cell k's estimate is complete once cells < k are, its draw is
//                        applied (est + sd z, or the truncated-normal ppf evaluated by every lane on lane k's numbers) and
//                        broadcast to the lanes that list it.
// Segments bound the records in memory: the caller picks the slots per segment (a multiple of 64, so that the chunks and
// therefore every rounding are the same whatever the segment size).
// Limits: num_points <= 48, H * W <= 2^25 cells (25-bit slot and cell fields in a record).
#include "gsm_internal.h"
#include "device_util.h"
#include "sgs_search.h"
#include "truncnorm.h"
#include <math.h>

namespace gsm {

constexpr int32_t kGridNever = 0x7fffffff;
constexpr uint64_t kGridPendingTag = 0xFFFC000000000000ull;     // bits 50..63 set: a negative quiet NaN no arithmetic produces
constexpr int kGridFieldBits = 25;
constexpr uint32_t kGridFieldMask = (1u << kGridFieldBits) - 1u;

// a value written by another wave of this workgroup: read from L2, past this CU's L1
__device__ __forceinline__ double load_l2(const double* p) {
  return __builtin_bit_cast(double, __hip_atomic_load((unsigned long long*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// ---------------------------------------------------------------------------------------------------------------------
// ranks: every cell of every realisation, then the path slots (a path cell must be NaN and listed once)
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sgs_grid_rank_kernel(const SgsGridArgs a) {
  const int r = blockIdx.y;
  const int HW = a.K.H * a.K.W;
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= HW) return;
  a.rank[(size_t)r * HW + c] = isnan(a.grid[(size_t)r * HW + c]) ? kGridNever : -1;
}
__global__ __launch_bounds__(256) void sgs_grid_slot_kernel(const SgsGridArgs a) {
  const int r = blockIdx.y;
  const int HW = a.K.H * a.K.W;
  const int64_t p0 = a.path_off[r];
  const int cnt = (int)(a.path_off[r + 1] - p0);
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= cnt) return;
  const int cell = a.path[p0 + k];
  if (cell < 0 || cell >= HW) { atomicOr(a.K.err, kSgsFlagCell); return; }
  if (atomicCAS(&a.rank[(size_t)r * HW + cell], kGridNever, k) != kGridNever) atomicOr(a.K.err, kSgsFlagCell);   // not NaN, or listed twice
}

// ---------------------------------------------------------------------------------------------------------------------
// sgs_grid_weights_kernel: one 64-lane workgroup per (slot of the segment, realisation).  kLocal: a variogram per cell
// (sgs_grid_weights_local_kernel) -- a.K.local [H*W][6] and a.K.vtype as sgs_search.h's LocalCov takes them, a.K.lag and a.K.sill unused
// ---------------------------------------------------------------------------------------------------------------------
template <bool kLocal>
__device__ __forceinline__ void sgs_grid_weights_cell(const SgsGridArgs& a, SgsSearchLds& L) {
  const int r = blockIdx.y, lane = threadIdx.x;
  const int slot = a.seg0 + blockIdx.x;
  const int64_t p0 = a.path_off[r];
  const int cnt = (int)(a.path_off[r + 1] - p0);
  if (slot >= cnt) return;
  const int H = a.K.H, W = a.K.W, HW = H * W;
  const size_t rec = (size_t)r * a.seg_cap + blockIdx.x;
  const int cell = a.path[p0 + slot];
  const int32_t* rank = a.rank + (size_t)r * HW;
  if (cell < 0 || cell >= HW || rank[cell] != slot) {            // flagged by sgs_grid_slot_kernel
    if (lane == 0) { a.rec_hdr[rec].n = -2; a.rec_hdr[rec].cell = 0; }
    return;
  }
  if (a.lo && a.lo[cell] == a.hi[cell]) {                        // interpolate.py:181-182: the lower bound, nothing drawn
    if (lane == 0) { a.rec_hdr[rec].n = -3; a.rec_hdr[rec].cell = cell; }
    return;
  }
  const double* __restrict__ g = a.grid + (size_t)r * HW;
  const int i0 = cell / W, j0 = cell - i0 * W;
  // rank: -1 = conditioning data, < slot = filled before this cell
  const int n = octant_ring_search(L, [rank, slot, W](int ic, int jc) { return rank[ic * W + jc] < slot; }, i0, j0, H, W, a.K.xs, a.K.ys,
                                   a.K.radius, a.K.hw, a.K.num_points / 8, lane);
  // a cell that fails gets no value: n = 0 in its record
  auto give_up = [&](int32_t flag) {
    if (lane == 0) { atomicOr(a.K.err, flag); a.rec_hdr[rec].n = 0; a.rec_hdr[rec].cell = cell; }
  };
  if (n == 0) { give_up(kSgsFlagNoValue); return; }                            // no value anywhere on the grid: the reference would loop forever
  const bool lagr = a.K.ktype == 0;
  double w_l, rho_l, sill;
  int my_i, my_j;                                                // the neighbour's (row, column): only the block kernel's record needs it
  if (const int e = krige_solve_at<kLocal, false>(L, a.K, cell, n, i0, j0, lagr, lane, w_l, rho_l, my_i, my_j, sill)) { give_up(e); return; }
  double var = sill - dev::wave64_sum(w_l * rho_l);
  var = fabs(var);                                               // interpolate.py:168
  const double sw = dev::wave64_sum(w_l);
  if (lane < kSgsMaxPts) {
    double2 vw = make_double2(0.0, 0.0);
    if (lane < n) {
      const int gg = L.nb_g[lane];
      vw.y = w_l;
      const int rk = rank[gg];
      if (rk < 0) vw.x = g[gg];                                   // conditioning value
      else if (a.lo && a.lo[gg] == a.hi[gg]) vw.x = a.lo[gg];     // a path cell whose value is its bound
      else vw.x = __builtin_bit_cast(double, kGridPendingTag | ((uint64_t)(uint32_t)rk << kGridFieldBits) | (uint64_t)(uint32_t)gg);
    }
    a.rec_vw[((rec >> 6) * kSgsMaxPts + lane) * 64 + (rec & 63)] = vw;
  }
  if (lane == 0) {
    SgsGridHdr hd;
    hd.n = n; hd.cell = cell; hd.sd = sqrt(var); hd.var = var;
    hd.c1 = lagr ? (1.0 - sw) / (double)n : a.K.gmean[r] * (1.0 - sw);
    a.rec_hdr[rec] = hd;
  }
}
__global__ __launch_bounds__(64) void sgs_grid_weights_kernel(const SgsGridArgs a) {
  __shared__ SgsSearchLds L;
  sgs_grid_weights_cell<false>(a, L);
}
__global__ __launch_bounds__(64) void sgs_grid_weights_local_kernel(const SgsGridArgs a) {
  __shared__ SgsSearchLds L;
  sgs_grid_weights_cell<true>(a, L);
}

// ---------------------------------------------------------------------------------------------------------------------
// sgs_grid_values_kernel: one workgroup of four waves per realisation, the segment's slots 64 at a time
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kGridSeqWaves = 4;
// the bounded draw of interpolate.py:183-187 for one cell: truncnorm.rvs(a, b, loc=est, scale=sd) = ppf(u, a, b) * sd + est;
// scale == 0 (scipy returns est without drawing) and a >= b (scipy raises) are domain errors
__device__ __noinline__ double grid_truncnorm_draw(double est, double sd, double lo, double hi, double u, int32_t* err) {
  if (!(sd > 0.0)) { atomicOr(err, kSgsFlagTruncnorm); return NAN; }
  const double ta = (lo - est) / sd, tb = (hi - est) / sd;
  if (!(ta < tb)) { atomicOr(err, kSgsFlagTruncnorm); return NAN; }
  return tn::ppf(u, ta, tb) * sd + est;
}

__global__ __launch_bounds__(64 * kGridSeqWaves) void sgs_grid_values_kernel(const SgsGridArgs a) {
  __shared__ double tile[64 * 64];                               // [chunk cell the value comes from][lane = cell that uses it]
  __shared__ double2 part[kGridSeqWaves][64];                    // per wave and cell: (sum v, sum w v) over the wave's entries
  __shared__ uint64_t mpart[kGridSeqWaves][64];
  const int r = blockIdx.x, lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int HW = a.K.H * a.K.W;
  double* __restrict__ g = a.grid + (size_t)r * HW;
  const int64_t p0 = a.path_off[r];
  const int k_end = min((int)(a.path_off[r + 1] - p0), a.seg0 + a.seg_len);
  const bool ok_k = a.K.ktype == 0, bounded = a.draw_kind == 1;
  for (int kc = a.seg0; kc < k_end; kc += 64) {
    __syncthreads();                                             // wave 0's values of the chunks before have been stored
    const int j = kc + lane;
    const size_t rec = (size_t)r * a.seg_cap + (size_t)(kc - a.seg0) + lane;
    SgsGridHdr hd;
    hd.n = -4; hd.cell = 0; hd.sd = 0.0; hd.var = 0.0; hd.c1 = 0.0;
    if (j < k_end) hd = a.rec_hdr[rec];
    const int n = hd.n;
    const double2* __restrict__ vw = a.rec_vw + (((size_t)r * a.seg_cap + (size_t)(kc - a.seg0)) >> 6) * kSgsMaxPts * 64;
    // ---- gather: entries wave, wave + 4, ... of every cell's list ----
    double sv = 0.0, swv = 0.0;
    uint64_t mask = 0;
    for (int e = wave; e < kSgsMaxPts; e += kGridSeqWaves) {
      if (e < n) {
        const double2 rr = vw[e * 64 + lane];
        const uint64_t bits = __builtin_bit_cast(uint64_t, rr.x);
        if ((bits >> 50) == (kGridPendingTag >> 50)) {
          const int s = (int)((bits >> kGridFieldBits) & kGridFieldMask), c = (int)(bits & kGridFieldMask);
          if (s < kc) {                                          // an earlier chunk: final, in the grid
            const double v = load_l2(g + (c < HW ? c : 0));
            sv += v; swv += rr.y * v;
          } else if (s - kc < 64) {                              // this chunk (s < j): through the tile
            tile[(s - kc) * 64 + lane] = ok_k ? rr.y + hd.c1 : rr.y;
            mask |= 1ull << (s - kc);
          }
        } else {
          sv += rr.x; swv += rr.y * rr.x;
        }
      }
    }
    part[wave][lane] = make_double2(sv, swv);
    mpart[wave][lane] = mask;
    __syncthreads();
    if (wave != 0) continue;
    // ---- sequence (wave 0) ----
    sv = 0.0; swv = 0.0; mask = 0;
#pragma unroll
    for (int w = 0; w < kGridSeqWaves; ++w) { const double2 q = part[w][lane]; sv += q.x; swv += q.y; mask |= mpart[w][lane]; }
    // est = sum w v + sum v (1 - sum w) / n (ordinary, _krige.py:42) or sum w v + global mean (1 - sum w) (simple, :79)
    double est = (n > 0) ? swv + (ok_k ? sv * hd.c1 : hd.c1) : 0.0;
    const double dr = (n > 0) ? a.draw[p0 + j] : 0.0;
    double lo_c = 0.0, hi_c = 0.0;
    if (bounded && (n > 0 || n == -3)) { lo_c = a.lo[hd.cell]; hi_c = a.hi[hd.cell]; }
    double fin = 0.0;
    const int kend = min(64, k_end - kc);
    double t_next = tile[lane];
    for (int k = 0; k < kend; ++k) {
      const double t = t_next;
      if (k + 1 < kend) t_next = tile[(k + 1) * 64 + lane];
      const int nk = __builtin_amdgcn_readlane(n, k);
      double vk = 0.0;
      if (nk > 0) {                                              // cell k's estimate is complete: every cell it lists came before
        const double ek = dev::readlane_f64(est, k), sk = dev::readlane_f64(hd.sd, k), dk = dev::readlane_f64(dr, k);
        if (bounded) vk = grid_truncnorm_draw(ek, sk, dev::readlane_f64(lo_c, k), dev::readlane_f64(hi_c, k), dk, a.K.err);
        else vk = ek + sk * dk;                                  // rng.normal(est, sqrt(var), 1), interpolate.py:174
      } else if (nk == -3) {
        vk = dev::readlane_f64(lo_c, k);
      } else if (nk == 0) {
        vk = NAN;                                                // error flagged by the weights pass
      }
      if (lane == k) fin = vk;
      if ((mask >> k) & 1ull) est = __fma_rn(t, vk, est);
    }
    if (j < k_end && (n > 0 || n == -3 || n == 0)) g[hd.cell] = fin;
    if (a.trace && j < k_end) {
      double* tr = a.trace + 3 * (p0 + j);
      tr[0] = (n > 0) ? (double)n : -1.0; tr[1] = (n > 0) ? est : fin; tr[2] = (n > 0) ? hd.var : 0.0;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // the stores have reached L2 before the next chunk's barrier
  }
}

// test hook (gsm_debug_special): the scalar functions behind the bounded draw, the normal-score transform and the per-cell
// variogram, exactly as the kernels of this file and sgs_search.h call them -- one thread per element
__global__ __launch_bounds__(256) void debug_special_kernel(int which, int vtype, int64_t n, const double* __restrict__ x0,
                                                            const double* __restrict__ x1, const double* __restrict__ x2,
                                                            const double* __restrict__ x3, const double* __restrict__ x4,
                                                            double* __restrict__ out, int32_t* err) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double a = x0[i];
  double r;
  switch (which) {
    case GSM_SPECIAL_NDTR: r = ns::ndtr(a); break;
    case GSM_SPECIAL_NDTRI: r = ns::ndtri(a); break;
    case GSM_SPECIAL_ERFC: r = ns::erfc_c(a); break;
    case GSM_SPECIAL_LOG_NDTR: r = tn::log_ndtr(a); break;
    case GSM_SPECIAL_NDTRI_EXP: r = tn::ndtri_exp(a); break;
    case GSM_SPECIAL_ERFCX_POS: r = tn::erfcx_pos(a); break;
    case GSM_SPECIAL_LOG_GAUSS_MASS: r = tn::log_gauss_mass(a, x1[i]); break;
    case GSM_SPECIAL_TRUNCNORM_PPF: r = tn::ppf(a, x1[i], x2[i]); break;
    case GSM_SPECIAL_TRUNCNORM_DRAW: r = grid_truncnorm_draw(a, x1[i], x2[i], x3[i], x4[i], err); break;
    default: r = local_cov_of(a, x1[i], x2[i], vtype); break;     // GSM_SPECIAL_LOCAL_COV
  }
  out[i] = r;
}
hipError_t launch_debug_special(int which, int vtype, int64_t n, const double* x0, const double* x1, const double* x2, const double* x3,
                                const double* x4, double* out, int32_t* err, hipStream_t st) {
  static const int n_args[GSM_SPECIAL_COUNT] = {1, 1, 1, 1, 1, 1, 2, 3, 5, 3};
  const double* x[5] = {x0, x1, x2, x3, x4};
  if (which < 0 || which >= GSM_SPECIAL_COUNT || n < 1 || n >= ((int64_t)1 << 31) - 256 || !out || !err) return hipErrorInvalidValue;
  for (int k = 0; k < n_args[which]; ++k)
    if (!x[k]) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(err, 0, sizeof(int32_t), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(debug_special_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, which, vtype, n, x0, x1, x2, x3, x4, out, err);
  return hipGetLastError();
}

static bool grid_args_ok(const SgsGridArgs& a) {
  return krige_search_ok(a.K) && !((int64_t)a.K.H * a.K.W > (int64_t)kGridFieldMask + 1 || a.n_real < 1 || a.n_real > 65535 ||
                                   a.seg_cap % 64 != 0 || a.seg_len < 1 || a.seg_len > a.seg_cap);
}
hipError_t launch_sgs_grid_ranks(const SgsGridArgs& a, int max_path, hipStream_t st) {
  if (!grid_args_ok(a)) return hipErrorInvalidValue;
  const int HW = a.K.H * a.K.W;
  hipLaunchKernelGGL(sgs_grid_rank_kernel, dim3((HW + 255) / 256, a.n_real), dim3(256), 0, st, a);
  if (max_path > 0) hipLaunchKernelGGL(sgs_grid_slot_kernel, dim3((max_path + 255) / 256, a.n_real), dim3(256), 0, st, a);
  return hipGetLastError();
}
hipError_t launch_sgs_grid_segment(const SgsGridArgs& a, hipStream_t st) {
  if (!grid_args_ok(a)) return hipErrorInvalidValue;
  if (a.K.local) hipLaunchKernelGGL(sgs_grid_weights_local_kernel, dim3(a.seg_len, a.n_real), dim3(64), 0, st, a);
  else hipLaunchKernelGGL(sgs_grid_weights_kernel, dim3(a.seg_len, a.n_real), dim3(64), 0, st, a);
  hipLaunchKernelGGL(sgs_grid_values_kernel, dim3(a.n_real), dim3(64 * kGridSeqWaves), 0, st, a);
  return hipGetLastError();
}

}  // namespace gsm
