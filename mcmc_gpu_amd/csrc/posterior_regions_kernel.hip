// Non-linear functionals of every chain's bed per region: ice volume, volume above flotation, area below sea level, the deepest
// and the highest point and the hypsometric curve of up to 8 regions that may overlap (include/gsm.h, gsm_posterior_regions).  None
// of them follows from the per-cell moments or from a projection; the reference reaches them only through the whole-bed host cache
// of one chain (bed_cache of chain_crf.run, MCMC.py:1198, :1363).
//
// Shape.  The workgroup grid of post_project_kernel: workgroup (plane part, chain), a lane walks the 256 * V-cell blocks of its
// part of the plane, V cells (16 bytes of bed where the plane allows it) per lane and trip.  A bed value is loaded once and serves
// every region whose bit is set in the cell's byte of the bit plane; the bit plane and surf are re-read by every chain, 9 bytes
// per cell (576 KiB at 256^2), and are expected to be served by L2.  Only the beds come from HBM.
//
// Per cell and region.  x = (double)bed, s = surf; valid = both finite.  h = s - x, t_thick = max(h, 0) by a compare and a
// select; b = x - sea_level, p = density_ratio * min(b, 0), q = h + p, t_haf = max(q, 0): separate fp64 operations (the library is
// built with -ffp-contract=off), so that the terms are the bits of the same expressions in NumPy.  The terms do not depend on the
// region and are formed once; per region a lane keeps three fp64 sums, three int32 counts, a minimum and a
// maximum in registers, each updated through a select on `the cell is valid and in the region` -- no branch on the bits, and a
// NaN cell adds an exact 0.  The kernel is instantiated by the region count's ceiling kMax (1, 4, 8): a call with one region does
// not carry the registers of eight.  Bits at or above n_regions are masked off.
//
// Sums.  A lane adds its cells in trip order; the lanes of a wave are summed by a shuffle tree (offsets 32 .. 1), the four waves
// in wave order through LDS, and the workgroup writes its 8 slots per region to slab[((chain * pparts + part) * K + k) * 8 + f];
// post_regions_sum_kernel adds the parts in part order (counts are exact integers in fp64, min and max are taken over the parts).
// No atomics touch a floating-point value: the same call gives the same bits.
//
// Hypsometry.  kf = floor((x - lo) * inv_width) in double, slot 0 below the range, n_bins + 1 at or above it, else (int)kf + 1
// (the slot rule of post_hist_kernel).  A workgroup counts in LDS, int32, one histogram of K * (n_bins + 2) counters in kCopies
// copies: a lane adds to copy (lane mod kCopies), counter-major, so that the lanes of a wave that fall into the same bin -- the
// usual case on a smooth bed -- land on different banks instead of queueing on one address.  The copies are summed and the
// non-zero totals added to `hyps` with integer atomics: exact in any order.
#include "posterior_device.h"
#include <type_traits>

namespace gsm {
namespace {

constexpr int kWaves = kPostBlock / 64;
constexpr int kRegSlots = 8;            // the slots of func per chain and region
constexpr int kRegLdsInts = 8192;       // 32 KiB of LDS counters per workgroup at most

// copies of the LDS histogram: the largest power of two <= 32 that keeps K * (n_bins + 2) * copies within kRegLdsInts
inline int regions_hist_copies(int n_regions, int n_bins) {
  int copies = 32;
  while (copies > 1 && n_regions * (n_bins + 2) * copies > kRegLdsInts) copies >>= 1;
  return copies;
}

struct RegionArgs {
  double sea_level, density_ratio, hyps_lo, hyps_inv_w;
  int n_regions, n_bins, copies;
};

template <typename T, int V, int kMax>
__global__ __launch_bounds__(kPostBlock) void post_regions_kernel(const T* __restrict__ beds, const double* __restrict__ surf,
                                                                  const uint8_t* __restrict__ bits, double* __restrict__ slab,
                                                                  int32_t* __restrict__ hyps, RegionArgs a, int64_t plane, int64_t blocks,
                                                                  int bpp) {
  using PT = Pack<T, V>;
  extern __shared__ int32_t hist[];                                  // [K * (n_bins + 2)][copies]; empty without hypsometry
  __shared__ double wave_part[kWaves][kMax][kRegSlots];
  const int c = blockIdx.y;
  const int K = a.n_regions, B = a.n_bins, slots = B + 2;
  const unsigned live = (1u << K) - 1u;
  const int64_t b0 = (int64_t)blockIdx.x * bpp, b1 = b0 + bpp < blocks ? b0 + bpp : blocks;
  if (B) {
    for (int i = threadIdx.x; i < K * slots * a.copies; i += kPostBlock) hist[i] = 0;
    __syncthreads();
  }
  const int copy = threadIdx.x & (a.copies - 1);
  const double inf = __builtin_inf(), bins = (double)B;
  double sx[kMax], sth[kMax], shaf[kMax], mn[kMax], mx[kMax];
  int nv[kMax], nb[kMax], ng[kMax];
#pragma unroll
  for (int k = 0; k < kMax; ++k) {
    sx[k] = sth[k] = shaf[k] = 0.0;
    mn[k] = inf;
    mx[k] = -inf;
    nv[k] = nb[k] = ng[k] = 0;
  }
  for (int64_t b = b0; b < b1; ++b) {
    const int64_t cell = (b * kPostBlock + threadIdx.x) * V;
    if (cell < plane) {                                              // plane is a multiple of V: the whole pack is inside
      const PT xp = *reinterpret_cast<const PT*>(beds + (int64_t)c * plane + cell);
      double sv[V];
      unsigned bv[V];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        sv[j] = surf[cell + j];
        bv[j] = bits[cell + j] & live;
      }
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const double x = (double)xp.v[j], s = sv[j];
        const bool valid = isfinite(x) && isfinite(s);
        const unsigned m = valid ? bv[j] : 0u;
        const double h = s - x;
        const double t_thick = h > 0.0 ? h : 0.0;
        const double bb = x - a.sea_level;
        const double p = a.density_ratio * (bb < 0.0 ? bb : 0.0);
        const double q = h + p;
        const double t_haf = q > 0.0 ? q : 0.0;
        const int below = bb < 0.0 ? 1 : 0, marine = (bb < 0.0 && t_haf > 0.0) ? 1 : 0;
#pragma unroll
        for (int k = 0; k < kMax; ++k) {
          const bool in = (m >> k) & 1u;
          sx[k] += in ? x : 0.0;
          sth[k] += in ? t_thick : 0.0;
          shaf[k] += in ? t_haf : 0.0;
          nv[k] += in ? 1 : 0;
          nb[k] += in ? below : 0;
          ng[k] += in ? marine : 0;
          mn[k] = in && x < mn[k] ? x : mn[k];
          mx[k] = in && x > mx[k] ? x : mx[k];
        }
        if (B && m) {
          const double kf = floor((x - a.hyps_lo) * a.hyps_inv_w);
          const int slot = kf < 0.0 ? 0 : (kf >= bins ? B + 1 : (int)kf + 1);
          for (unsigned r = m; r; r &= r - 1u) {
            const int k = __builtin_ctz(r);
            atomicAdd(&hist[(k * slots + slot) * a.copies + copy], 1);
          }
        }
      }
    }
  }
  // lanes -> wave (a fixed shuffle tree), waves -> workgroup in wave order
#pragma unroll
  for (int k = 0; k < kMax; ++k)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      sx[k] += __shfl_down(sx[k], off, 64);
      sth[k] += __shfl_down(sth[k], off, 64);
      shaf[k] += __shfl_down(shaf[k], off, 64);
      nv[k] += __shfl_down(nv[k], off, 64);
      nb[k] += __shfl_down(nb[k], off, 64);
      ng[k] += __shfl_down(ng[k], off, 64);
      const double on = __shfl_down(mn[k], off, 64), ox = __shfl_down(mx[k], off, 64);
      mn[k] = on < mn[k] ? on : mn[k];
      mx[k] = ox > mx[k] ? ox : mx[k];
    }
  const int wave = threadIdx.x / 64;
  if (threadIdx.x % 64 == 0) {
#pragma unroll
    for (int k = 0; k < kMax; ++k) {
      double* o = wave_part[wave][k];
      o[0] = (double)nv[k]; o[1] = sx[k]; o[2] = sth[k]; o[3] = shaf[k];
      o[4] = (double)nb[k]; o[5] = (double)ng[k]; o[6] = mn[k]; o[7] = mx[k];
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < K * kRegSlots) {
    const int k = threadIdx.x / kRegSlots, f = threadIdx.x % kRegSlots;
    double s = wave_part[0][k][f];
    for (int w = 1; w < kWaves; ++w) {
      const double v = wave_part[w][k][f];
      s = f == 6 ? (v < s ? v : s) : f == 7 ? (v > s ? v : s) : s + v;
    }
    slab[(((int64_t)c * gridDim.x + blockIdx.x) * K + k) * kRegSlots + f] = s;
  }
  if (B) {                                                           // the barrier above also orders the LDS counters
    int32_t* out = hyps + (int64_t)c * K * slots;
    for (int i = threadIdx.x; i < K * slots; i += kPostBlock) {
      int n = 0;
      for (int j = 0; j < a.copies; ++j) n += hist[i * a.copies + j];
      if (n) atomicAdd(out + i, n);
    }
  }
}

// func[i] over the plane parts in part order, i = (c * K + k) * 8 + f: a sum, or the minimum (f == 6) / maximum (f == 7)
__global__ __launch_bounds__(kPostBlock) void post_regions_sum_kernel(const double* __restrict__ slab, double* __restrict__ func, int64_t n,
                                                                      int n_regions, int pparts) {
  const int64_t i = (int64_t)blockIdx.x * kPostBlock + threadIdx.x;
  if (i >= n) return;
  const int per_chain = n_regions * kRegSlots;
  const int64_t c = i / per_chain;
  const int r = (int)(i % per_chain), f = r % kRegSlots;
  const double* p = slab + c * pparts * per_chain + r;
  double s = p[0];
  for (int q = 1; q < pparts; ++q) {
    const double v = p[(int64_t)q * per_chain];
    s = f == 6 ? (v < s ? v : s) : f == 7 ? (v > s ? v : s) : s + v;
  }
  func[i] = s;
}

// f(kMax as an integral constant): the instantiation that holds n_regions
template <typename F>
void dispatch_regions(int n_regions, F&& f) {
  if (n_regions <= 1) f(std::integral_constant<int, 1>{});
  else if (n_regions <= 4) f(std::integral_constant<int, 4>{});
  else f(std::integral_constant<int, kRegMaxRegions>{});
}

}  // namespace

int posterior_regions_parts(int64_t plane, int n_chains, int f32_state, int n_cu) {
  const int64_t blocks = posterior_cell_blocks(plane, posterior_vec(plane, f32_state));
  const int64_t want = ((int64_t)n_cu * 8 + n_chains - 1) / n_chains;
  return (int)std::max<int64_t>(1, std::min<int64_t>(want, blocks));
}

hipError_t launch_posterior_regions(const void* beds, const double* surf, const uint8_t* bits, int n_regions, double sea_level,
                                    double density_ratio, double* slab, double* func, double hyps_lo, double hyps_inv_w, int n_bins,
                                    int32_t* hyps, int64_t plane, int n_chains, int f32_state, int n_cu, hipStream_t st) {
  const int vec = posterior_vec(plane, f32_state);
  const int64_t blocks = posterior_cell_blocks(plane, vec);
  const int want = posterior_regions_parts(plane, n_chains, f32_state, n_cu);
  const int bpp = (int)((blocks + want - 1) / want);                 // 256 * vec-cell blocks per plane part
  const int pparts = (int)((blocks + bpp - 1) / bpp);                // <= want: no part is empty
  RegionArgs a{sea_level, density_ratio, hyps_lo, hyps_inv_w, n_regions, n_bins, n_bins ? regions_hist_copies(n_regions, n_bins) : 1};
  const size_t lds = n_bins ? (size_t)n_regions * (n_bins + 2) * a.copies * sizeof(int32_t) : 0;
  const dim3 grid((unsigned)pparts, (unsigned)n_chains);
  dispatch_state_vec(f32_state, vec, [&](auto tag) {
    using T = typename decltype(tag)::T;
    dispatch_regions(n_regions, [&](auto kmax) {
      hipLaunchKernelGGL((post_regions_kernel<T, decltype(tag)::V, decltype(kmax)::value>), grid, dim3(kPostBlock), lds, st, (const T*)beds, surf,
                         bits, slab, hyps, a, plane, blocks, bpp);
    });
  });
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int64_t n = (int64_t)n_chains * n_regions * kRegSlots;
  hipLaunchKernelGGL(post_regions_sum_kernel, dim3((unsigned)((n + kPostBlock - 1) / kPostBlock)), dim3(kPostBlock), 0, st, slab, func, n,
                     n_regions, pparts);
  return hipGetLastError();
}

}  // namespace gsm
