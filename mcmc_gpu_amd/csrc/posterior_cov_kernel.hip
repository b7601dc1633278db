// Posterior covariance of the bed with linear functionals: for K <= 15 weight fields ("probes") Omega_k of the grid's shape, per
// snapshot the projection p[c, k] = sum over the cells with Omega_k != 0 of Omega_k[cell] * d_c[cell] of every chain c, d_c = bed_c - g,
// and the cross sum Y[k, cell] += sum_c d_c[cell] * p[c, k] (include/gsm.h, gsm_posterior_project, gsm_posterior_cross).  With
// the pooled first moments these give C Omega^T, the posterior covariance matrix applied to the probes, on the host
// (posterior.py).  The reference can reach a covariance across cells only through the whole-bed host cache of one chain
// (bed_cache of chain_crf.run, MCMC.py:1198, :1363).
//
// Project.  Workgroup (plane part, chain): a lane walks the 256 * V-cell blocks of its part of the plane, V = 2 cells per lane
// and trip where the plane is even (16 bytes of g and of every probe per lane and load), and adds select(Omega != 0, Omega * d,
// 0) to kMax accumulators in registers -- a select on the product, so a lane never branches on its weights and a NaN bed
// under a zero weight adds an exact 0.  The accumulators are summed over the wave by a shuffle tree (offsets 32, 16, .. 1), over the
// four waves in wave order through LDS, and written to slab[(chain * pparts + part) * K + k]; post_project_sum_kernel adds the
// parts in part order.  All lanes stay in the kernel to the end (the tree needs them).
// What is assumed about the probes: every chain's workgroups re-read all of Omega and g, (K + 1) * plane * 8 bytes (8 MiB at
// 256^2 x 15).  That is more than one XCD's 4 MiB L2 holds at K = 15 and less at K <= 7, so the re-reads are assumed to be served
// by L2 where the probes fit it and otherwise by the 256 MiB Infinity Cache, which Omega, g and one snapshot's streamed beds (512
// MiB at 1024 chains of 256^2 fp64, each byte read once) leave it room for.  Only the beds are expected to come from HBM.  The
// pass is then bound by the cache-side traffic, (K + 1) * 8 bytes per chain-cell, not by HBM (DESIGN section 5 has the rates).
//
// Cross.  A stream in the style of post_lag_kernel: no LDS, no atomics, V cells (16 bytes of bed) per lane, workgroup
// (cell block, part) walks the chains of its part of the chain axis (posterior_parts) in index order.  Per chain a lane loads its
// bed pack -- kCovChains chains' loads are issued together -- and the wave reads the K projections of that chain through scalar
// loads (c and k are wave-uniform, proj is const __restrict__), all of them issued before the first use, then does kMax x V fp64
// fused multiply-adds into accumulators that live in registers; they are indexed by the unrolled probe only, hence the
// instantiation by the probe count's ceiling kMax (3, 7, 15): a call with 3 probes does not carry the registers of 15.  The
// chain loop is straight-line code: a call with fewer than kMax probes repeats its last projection into accumulators that are
// never stored rather than branch around them.  Each part writes [K, plane] to its slab and post_combine_kernel
// (posterior_kernel.hip) adds the slabs in part order onto `cross`.  A part without chains writes zeros.
//
// Sums.  Differences, products and sums are fp64 whatever the state type; every sum is taken in a fixed order (cells of a lane in
// trip order, the shuffle tree, waves, parts; chains in index order, parts), so the same calls give the same bits.  Every kernel
// argument is wave-uniform.
#include "posterior_device.h"
#include <type_traits>

namespace gsm {
namespace {

constexpr int kCovChains = 4;      // chains whose bed loads are in flight together in the cross kernel
constexpr int kWaves = kPostBlock / 64;

template <typename T, int V, int kMax>
__global__ __launch_bounds__(kPostBlock) void post_project_kernel(const T* __restrict__ beds, const double* __restrict__ g,
                                                                  const double* __restrict__ probes, double* __restrict__ slab, int64_t plane,
                                                                  int n_probes, int64_t blocks, int bpp) {
  using PT = Pack<T, V>;
  __shared__ double wave_sum[kWaves][kMax];
  const int c = blockIdx.y;
  const int64_t b0 = (int64_t)blockIdx.x * bpp, b1 = b0 + bpp < blocks ? b0 + bpp : blocks;
  double acc[kMax];
#pragma unroll
  for (int k = 0; k < kMax; ++k) acc[k] = 0.0;
  for (int64_t b = b0; b < b1; ++b) {
    const int64_t cell = (b * kPostBlock + threadIdx.x) * V;
    if (cell < plane) {
      const PT x = *reinterpret_cast<const PT*>(beds + (int64_t)c * plane + cell);
      double gv[V], w[kMax][V];
#pragma unroll
      for (int j = 0; j < V; ++j) gv[j] = g[cell + j];
#pragma unroll
      for (int k = 0; k < kMax; ++k)
        if (k < n_probes) {
#pragma unroll
          for (int j = 0; j < V; ++j) w[k][j] = probes[(int64_t)k * plane + cell + j];
        }
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const double d = (double)x.v[j] - gv[j];
#pragma unroll
        for (int k = 0; k < kMax; ++k)
          if (k < n_probes) {
            const double prod = w[k][j] * d;
            acc[k] += w[k][j] != 0.0 ? prod : 0.0;
          }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kMax; ++k)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc[k] += __shfl_down(acc[k], off, 64);
  const int wave = threadIdx.x / 64;
  if (threadIdx.x % 64 == 0) {
#pragma unroll
    for (int k = 0; k < kMax; ++k) wave_sum[wave][k] = acc[k];
  }
  __syncthreads();
  if ((int)threadIdx.x < n_probes) {
    double s = wave_sum[0][threadIdx.x];
    for (int w = 1; w < kWaves; ++w) s += wave_sum[w][threadIdx.x];
    slab[((int64_t)c * gridDim.x + blockIdx.x) * n_probes + threadIdx.x] = s;
  }
}

// proj[i] = sum over the plane parts, in part order, of slab[(c * pparts + p) * K + k], i = c * K + k
__global__ __launch_bounds__(kPostBlock) void post_project_sum_kernel(const double* __restrict__ slab, double* __restrict__ proj, int n_chains,
                                                                      int n_probes, int pparts) {
  const int64_t i = (int64_t)blockIdx.x * kPostBlock + threadIdx.x;
  if (i >= (int64_t)n_chains * n_probes) return;
  const int64_t c = i / n_probes, k = i % n_probes;
  double s = 0.0;
  for (int p = 0; p < pparts; ++p) s += slab[(c * pparts + p) * n_probes + k];
  proj[i] = s;
}

template <typename T, int V, int kMax>
__global__ __launch_bounds__(kPostBlock) void post_cross_kernel(const T* __restrict__ beds, const double* __restrict__ g,
                                                                const double* __restrict__ proj, double* __restrict__ slab, int64_t plane,
                                                                int n_chains, int cpp, int n_probes) {
  using PT = Pack<T, V>;
  const int64_t cell = ((int64_t)blockIdx.x * kPostBlock + threadIdx.x) * V;
  if (cell >= plane) return;
  const auto [c0, c1] = chain_range(cpp, n_chains);
  double gv[V], acc[kMax][V];
#pragma unroll
  for (int j = 0; j < V; ++j) gv[j] = g[cell + j];
#pragma unroll
  for (int k = 0; k < kMax; ++k)
#pragma unroll
    for (int j = 0; j < V; ++j) acc[k][j] = 0.0;
  // one chain: its K projections are wave-uniform values, each used for the V cells of the lane.  An instantiation serves
  // n_probes in [kMin, kMax]: the first kMin loads are adjacent, the others read probe min(k, n_probes - 1) -- in bounds, and no
  // branch stands between the loads or between the multiply-adds, so that all of a chain's projections are in flight together
  // and the next chain's can be fetched under this chain's arithmetic.  Accumulators k >= n_probes are never stored.
  constexpr int kMin = kMax == 3 ? 1 : (kMax + 1) / 2;
  auto fold = [&](const PT& b, int c) {
    double d[V], p[kMax];
#pragma unroll
    for (int j = 0; j < V; ++j) d[j] = (double)b.v[j] - gv[j];
    const double* __restrict__ pc = proj + (int64_t)c * n_probes;
#pragma unroll
    for (int k = 0; k < kMax; ++k) p[k] = pc[k < kMin ? k : (k < n_probes ? k : n_probes - 1)];
#pragma unroll
    for (int k = 0; k < kMax; ++k)
#pragma unroll
      for (int j = 0; j < V; ++j) acc[k][j] = __builtin_fma(d[j], p[k], acc[k][j]);
  };
  int c = c0;
  for (; c + kCovChains <= c1; c += kCovChains) {
    PT b[kCovChains];
#pragma unroll
    for (int i = 0; i < kCovChains; ++i) b[i] = *reinterpret_cast<const PT*>(beds + (int64_t)(c + i) * plane + cell);
#pragma unroll
    for (int i = 0; i < kCovChains; ++i) fold(b[i], c + i);
  }
  for (; c < c1; ++c) fold(*reinterpret_cast<const PT*>(beds + (int64_t)c * plane + cell), c);
#pragma unroll
  for (int k = 0; k < kMax; ++k)
    if (k < n_probes) {
      double* o = slab + ((int64_t)blockIdx.y * n_probes + k) * plane + cell;
#pragma unroll
      for (int j = 0; j < V; ++j) o[j] = acc[k][j];
    }
}

// f(StateVec<T, V>{}) for the project kernel's widths: 2 cells per lane or 1, with either state type
template <typename F>
void dispatch_project(int f32_state, int vec, F&& f) {
  if (f32_state) { if (vec == 2) f(StateVec<float, 2>{}); else f(StateVec<float, 1>{}); }
  else { if (vec == 2) f(StateVec<double, 2>{}); else f(StateVec<double, 1>{}); }
}

// f(kMax as an integral constant): the instantiation that holds n_probes
template <typename F>
void dispatch_probes(int n_probes, F&& f) {
  if (n_probes <= 3) f(std::integral_constant<int, 3>{});
  else if (n_probes <= 7) f(std::integral_constant<int, 7>{});
  else f(std::integral_constant<int, kLagMaxLags>{});
}

}  // namespace

int posterior_project_parts(int64_t plane, int n_chains, int n_cu) {
  const int64_t blocks = posterior_cell_blocks(plane, posterior_project_vec(plane));
  const int64_t want = ((int64_t)n_cu * 8 + n_chains - 1) / n_chains;
  return (int)std::max<int64_t>(1, std::min<int64_t>(want, blocks));
}

hipError_t launch_posterior_project(const void* beds, const double* g, const double* probes, double* slab, double* proj, int64_t plane,
                                    int n_chains, int n_probes, int f32_state, int n_cu, hipStream_t st) {
  const int vec = posterior_project_vec(plane);
  const int64_t blocks = posterior_cell_blocks(plane, vec);
  const int want = posterior_project_parts(plane, n_chains, n_cu);
  const int bpp = (int)((blocks + want - 1) / want);                 // 256 * vec-cell blocks per plane part
  const int pparts = (int)((blocks + bpp - 1) / bpp);                // <= want: no part is empty
  const dim3 grid((unsigned)pparts, (unsigned)n_chains);
  dispatch_project(f32_state, vec, [&](auto tag) {
    using T = typename decltype(tag)::T;
    dispatch_probes(n_probes, [&](auto kmax) {
      hipLaunchKernelGGL((post_project_kernel<T, decltype(tag)::V, decltype(kmax)::value>), grid, dim3(kPostBlock), 0, st, (const T*)beds, g, probes,
                         slab, plane, n_probes, blocks, bpp);
    });
  });
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int64_t n = (int64_t)n_chains * n_probes;
  hipLaunchKernelGGL(post_project_sum_kernel, dim3((unsigned)((n + kPostBlock - 1) / kPostBlock)), dim3(kPostBlock), 0, st, slab, proj, n_chains,
                     n_probes, pparts);
  return hipGetLastError();
}

hipError_t launch_posterior_cross(const void* beds, const double* g, const double* proj, double* slab, double* cross, int64_t plane,
                                  int n_chains, int parts, int n_probes, int f32_state, int n_cu, hipStream_t st) {
  const int vec = posterior_vec(plane, f32_state);
  const dim3 grid((unsigned)posterior_cell_blocks(plane, vec), (unsigned)parts);
  dispatch_state_vec(f32_state, vec, [&](auto tag) {
    using T = typename decltype(tag)::T;
    dispatch_probes(n_probes, [&](auto kmax) {
      hipLaunchKernelGGL((post_cross_kernel<T, decltype(tag)::V, decltype(kmax)::value>), grid, dim3(kPostBlock), 0, st, (const T*)beds, g, proj,
                         slab, plane, n_chains, chains_per_part(n_chains, parts), n_probes);
    });
  });
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  PostOut out{};
  for (int k = 0; k < n_probes; ++k) out.f[k] = cross + (int64_t)k * plane;
  return launch_posterior_combine(slab, parts, n_probes, plane, out, 1, n_cu, st);
}

}  // namespace gsm
