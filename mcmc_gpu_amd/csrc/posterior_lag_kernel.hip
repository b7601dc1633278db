// Posterior lagged differences: per cell and lag t = 1 .. K the sum over all chains of (bed - bed t snapshots ago)^2, from a
// ring of the last K snapshots of every chain that stays on the device (include/gsm.h, gsm_posterior_lagged).  The sums are the
// variogram form of the autocorrelation, from which the effective sample size follows on the host (posterior.py).  The reference
// can reach an autocorrelation only through the whole-bed host cache of one chain (bed_cache of chain_crf.run, MCMC.py:1198, :1363).
//
// Shape.  A stream without reuse, in the style of post_pooled_kernel: no LDS, no atomics, consecutive lanes on consecutive
// addresses, V cells (16 bytes where plane % V == 0) per lane and load.  Workgroup (cell block, part) walks the chains of its
// part of the chain axis (posterior_parts) in index order.  Per chain a lane loads the bed and the n_valid <= K ring values of
// its chain-cells -- all of them issued before the first use --, adds (bed - ring value)^2 to K x V accumulators that live in
// registers, and stores the bed into ring slot `head` from the registers that already hold it.  Lag t reads slot
// (head - t) mod K; lag K reads the very slot that is overwritten: same lane, read before write, and no other lane touches
// those cells.  n_lags, head and n_valid are kernel arguments, so every test on them is wave-uniform; the accumulators are
// indexed by the unrolled lag only, hence the instantiation by the lag count's ceiling kMax (3, 7, 15): a call with 7 lags
// does not carry the registers of 15.
//
// Sums.  Differences, squares and sums are fp64 whatever the state type.  Each part writes [n_valid, plane] sums to its slab
// and post_lag_combine_kernel adds the slabs in part order onto lag_sqdiff: nothing depends on scheduling, the same calls
// give the same bits.  A part without chains writes zeros.
#include "gsm_internal.h"
#include <algorithm>

namespace gsm {
namespace {

constexpr int kLagBlock = 256;

template <typename T, int V>
struct alignas(sizeof(T) * V) LagPack { T v[V]; };

template <typename T, int V, int kMax>
__global__ __launch_bounds__(kLagBlock) void post_lag_kernel(const T* __restrict__ beds, T* ring, double* __restrict__ slab, int64_t plane,
                                                             int n_chains, int cpp, int n_lags, int head, int n_valid) {
  using PT = LagPack<T, V>;
  const int64_t cell = ((int64_t)blockIdx.x * kLagBlock + threadIdx.x) * V;
  if (cell >= plane) return;
  const int c0 = blockIdx.y * cpp, c1 = min(n_chains, c0 + cpp);
  // where lag t + 1 lies: slot (head - (t + 1)) mod n_lags
  int slot[kMax];
#pragma unroll
  for (int t = 0; t < kMax; ++t) {
    const int s = head - (t + 1);
    slot[t] = t < n_valid ? (s < 0 ? s + n_lags : s) : 0;
  }
  double acc[kMax][V];
#pragma unroll
  for (int t = 0; t < kMax; ++t)
#pragma unroll
    for (int k = 0; k < V; ++k) acc[t][k] = 0.0;
  for (int c = c0; c < c1; ++c) {
    const PT b = *reinterpret_cast<const PT*>(beds + (int64_t)c * plane + cell);
    PT r[kMax];
#pragma unroll
    for (int t = 0; t < kMax; ++t)
      if (t < n_valid) r[t] = *reinterpret_cast<const PT*>(ring + ((int64_t)slot[t] * n_chains + c) * plane + cell);
#pragma unroll
    for (int t = 0; t < kMax; ++t)
      if (t < n_valid) {
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const double d = (double)b.v[k] - (double)r[t].v[k];
          acc[t][k] += d * d;
        }
      }
    *reinterpret_cast<PT*>(ring + ((int64_t)head * n_chains + c) * plane + cell) = b;
  }
#pragma unroll
  for (int t = 0; t < kMax; ++t)
    if (t < n_valid) {
      double* o = slab + ((int64_t)blockIdx.y * n_valid + t) * plane + cell;
#pragma unroll
      for (int k = 0; k < V; ++k) o[k] = acc[t][k];
    }
}

// out[f * plane + cell] += sum over parts, in part order, of slab[(p * n_fields + f) * plane + cell]
__global__ __launch_bounds__(kLagBlock) void post_lag_combine_kernel(const double* __restrict__ slab, int parts, int n_fields, int64_t plane,
                                                                     double* __restrict__ out) {
  for (int64_t cell = (int64_t)blockIdx.x * kLagBlock + threadIdx.x; cell < plane; cell += (int64_t)gridDim.x * kLagBlock)
    for (int f = 0; f < n_fields; ++f) {
      double s = 0.0;
      for (int p = 0; p < parts; ++p) s += slab[((int64_t)p * n_fields + f) * plane + cell];
      out[(int64_t)f * plane + cell] += s;
    }
}

template <typename T, int V>
void lag_t(const void* beds, void* ring, double* slab, int64_t plane, int n_chains, int parts, int cpp, int n_lags, int head, int n_valid,
           hipStream_t st) {
  const dim3 grid((unsigned)((plane / V + kLagBlock - 1) / kLagBlock), (unsigned)parts);
  if (n_lags <= 3)
    hipLaunchKernelGGL((post_lag_kernel<T, V, 3>), grid, dim3(kLagBlock), 0, st, (const T*)beds, (T*)ring, slab, plane, n_chains, cpp, n_lags, head, n_valid);
  else if (n_lags <= 7)
    hipLaunchKernelGGL((post_lag_kernel<T, V, 7>), grid, dim3(kLagBlock), 0, st, (const T*)beds, (T*)ring, slab, plane, n_chains, cpp, n_lags, head, n_valid);
  else
    hipLaunchKernelGGL((post_lag_kernel<T, V, kLagMaxLags>), grid, dim3(kLagBlock), 0, st, (const T*)beds, (T*)ring, slab, plane, n_chains, cpp, n_lags, head, n_valid);
}

}  // namespace

// cells per lane: 16 bytes where the plane allows it, so that every chain's row of a lane starts on its own vector boundary
int posterior_lag_vec(int64_t plane, int f32_state) {
  if (f32_state) return plane % 4 == 0 ? 4 : plane % 2 == 0 ? 2 : 1;
  return plane % 2 == 0 ? 2 : 1;
}

hipError_t launch_posterior_lagged(const void* beds, void* ring, double* slab, double* lag_sqdiff, int64_t plane, int n_chains, int parts,
                                   int n_lags, int head, int n_valid, int f32_state, int n_cu, hipStream_t st) {
  if (n_lags < 1 || n_lags > kLagMaxLags || head < 0 || head >= n_lags || n_valid < 0 || n_valid > n_lags) return hipErrorInvalidValue;
  const int cpp = (n_chains + parts - 1) / parts;
  const int vec = posterior_lag_vec(plane, f32_state);
  if (f32_state) {
    if (vec == 4) lag_t<float, 4>(beds, ring, slab, plane, n_chains, parts, cpp, n_lags, head, n_valid, st);
    else if (vec == 2) lag_t<float, 2>(beds, ring, slab, plane, n_chains, parts, cpp, n_lags, head, n_valid, st);
    else lag_t<float, 1>(beds, ring, slab, plane, n_chains, parts, cpp, n_lags, head, n_valid, st);
  } else {
    if (vec == 2) lag_t<double, 2>(beds, ring, slab, plane, n_chains, parts, cpp, n_lags, head, n_valid, st);
    else lag_t<double, 1>(beds, ring, slab, plane, n_chains, parts, cpp, n_lags, head, n_valid, st);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || n_valid == 0) return e;
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((plane + kLagBlock - 1) / kLagBlock, (int64_t)n_cu * 8));
  hipLaunchKernelGGL(post_lag_combine_kernel, dim3(grid), dim3(kLagBlock), 0, st, slab, parts, n_valid, plane, lag_sqdiff);
  return hipGetLastError();
}

}  // namespace gsm
