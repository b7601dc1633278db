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
// and post_combine_kernel (posterior_kernel.hip) adds the slabs in part order onto lag_sqdiff: nothing depends on scheduling, the same calls
// give the same bits.  A part without chains writes zeros.
#include "posterior_device.h"

namespace gsm {
namespace {

template <typename T, int V, int kMax>
__global__ __launch_bounds__(kPostBlock) void post_lag_kernel(const T* __restrict__ beds, T* ring, double* __restrict__ slab, int64_t plane,
                                                             int n_chains, int cpp, int n_lags, int head, int n_valid) {
  using PT = Pack<T, V>;
  const int64_t cell = ((int64_t)blockIdx.x * kPostBlock + threadIdx.x) * V;
  if (cell >= plane) return;
  const auto [c0, c1] = chain_range(cpp, n_chains);
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

template <typename T, int V>
void lag_t(const void* beds, void* ring, double* slab, int64_t plane, int n_chains, int parts, int cpp, int n_lags, int head, int n_valid,
           hipStream_t st) {
  const dim3 grid((unsigned)posterior_cell_blocks(plane, V), (unsigned)parts);
  if (n_lags <= 3)
    hipLaunchKernelGGL((post_lag_kernel<T, V, 3>), grid, dim3(kPostBlock), 0, st, (const T*)beds, (T*)ring, slab, plane, n_chains, cpp, n_lags, head, n_valid);
  else if (n_lags <= 7)
    hipLaunchKernelGGL((post_lag_kernel<T, V, 7>), grid, dim3(kPostBlock), 0, st, (const T*)beds, (T*)ring, slab, plane, n_chains, cpp, n_lags, head, n_valid);
  else
    hipLaunchKernelGGL((post_lag_kernel<T, V, kLagMaxLags>), grid, dim3(kPostBlock), 0, st, (const T*)beds, (T*)ring, slab, plane, n_chains, cpp, n_lags, head, n_valid);
}

}  // namespace

hipError_t launch_posterior_lagged(const void* beds, void* ring, double* slab, double* lag_sqdiff, int64_t plane, int n_chains, int parts,
                                   int n_lags, int head, int n_valid, int f32_state, int n_cu, hipStream_t st) {
  dispatch_state_vec(f32_state, posterior_vec(plane, f32_state), [&](auto tag) {
    lag_t<typename decltype(tag)::T, decltype(tag)::V>(beds, ring, slab, plane, n_chains, parts, chains_per_part(n_chains, parts), n_lags, head,
                                                       n_valid, st);
  });
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || n_valid == 0) return e;
  PostOut out{};
  for (int t = 0; t < n_valid; ++t) out.f[t] = lag_sqdiff + (int64_t)t * plane;
  return launch_posterior_combine(slab, parts, n_valid, plane, out, 1, n_cu, st);
}

}  // namespace gsm
