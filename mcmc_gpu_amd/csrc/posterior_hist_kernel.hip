// Posterior histogram: per-cell counts of every chain's bed about a common field, and of the beds below fixed levels
// (include/gsm.h, gsm_posterior_histogram).  The reference can reach quantiles and exceedance probabilities only through
// whole-bed host caches (bed_cache of chain_crf.run, MCMC.py:1198, :1362-1363).
//
// Shape.  One cell per lane, consecutive lanes on consecutive cells, 256 lanes per workgroup; blockIdx.y is a part of the chain
// axis (posterior_parts, as in post_pooled_kernel) and a part walks its chains with kHistChains loads in flight.  A lane owns
// one column of LDS counters and nobody else touches it: no barrier anywhere in the kernel, and dead lanes of the last
// workgroup simply leave.
//
// LDS counters.  16 bits wide, two slots to a dword: slot s of lane l is half (s & 1) of lds[(s >> 1) * 256 + l], so a wave's
// 64 lanes fall on 64 consecutive dwords whatever their slots are (bank = l mod 32: conflict-free in both 32-lane groups).  The
// increment is ONE non-returning LDS add of 1 << 16 (s & 1) to the lane's own dword: used as a fire-and-forget
// read-modify-write, not for atomicity -- there is no second writer -- so that a value costs one LDS instruction and no wait,
// where a load / add / store of a 16-bit counter would serialise on the previous value's store.  A half never carries into
// its neighbour because a part counts at most kHistMaxCpp = 65535 chains (the launcher raises the part count to keep that).
// The level counters (at most 8) are registers: `bed < level` is a compare and an add, the levels are kernel arguments
// (SGPRs), unused ones are -inf, below which nothing lies.  The pass is bound by these fp64 compares more than by its loads, so
// the kernel is instantiated for 2 and for 8 level counters and a call with at most 2 levels does not pay for 8.
//
// LDS and occupancy.  (B + 4) / 2 rows of 1 KiB per workgroup: 34 KiB at B = 64 and 66 KiB at B = 128, against 67 and 131 KiB
// with 32-bit counters.  The kernel is instantiated for 18, 34 and 66 rows (B <= 32, 64, 128) with static LDS; the compiler
// reports 8, 4 and 2 waves per SIMD (at most 50 VGPRs; LDS-limited above 32 bins), i.e. 8, 4 and 2 workgroups or 32, 16 and
// 8 waves per CU, each lane with 8 loads in flight.
//
// Flush.  Each part adds its non-zero counters to `counts` with the ordinary HIP atomicAdd on int (a vector global atomic
// without return, consecutive lanes on consecutive ints).  Chosen over slabs and a combine pass because integer addition is
// exact in any order -- the result is bit-reproducible either way -- and because the slabs would be parts * (B + 3 + L) *
// H * W ints written and read again per snapshot (72 MiB at 256 x 256, 4 parts, B = 64, L = 2) where most counters of a
// part are zero and are skipped here.  The call adds to `counts`, so accumulation over snapshots needs nothing else.
#include "posterior_device.h"

namespace gsm {
namespace {

constexpr int kHistChains = 8;          // chains whose loads are in flight together
constexpr int kHistMaxCpp = 65535;      // chains per part that a 16-bit counter holds

struct HistLevels { double v[kHistMaxLevels]; };

// slot of d = bed - g: 0 underflow, 1 .. B the bins, B + 1 overflow, B + 2 NaN.  The product and the difference are separate
// operations (the library is built with -ffp-contract=off and there is no add after the multiply), compared in double.
__device__ __forceinline__ int hist_slot(double d, double inv_w, double half, double bins, int B) {
  const double kf = floor(d * inv_w) + half;
  if (kf != kf) return B + 2;
  if (kf < 0.0) return 0;
  if (kf >= bins) return B + 1;
  return (int)kf + 1;
}

template <typename T, int kRows, int kLev>
__global__ __launch_bounds__(kPostBlock) void post_hist_kernel(const T* __restrict__ beds, const double* __restrict__ g, double inv_w, int B,
                                                               HistLevels lev, int n_levels, int32_t* __restrict__ counts, int64_t plane,
                                                               int n_chains, int cpp) {
  __shared__ uint32_t lds[kRows * kPostBlock];
  const int64_t cell = (int64_t)blockIdx.x * kPostBlock + threadIdx.x;
  const auto [c0, c1] = chain_range(cpp, n_chains);
  if (cell >= plane || c0 >= c1) return;
  const int rows = (B + 4) / 2;                          // B + 3 slots, two to a dword
  uint32_t* col = lds + threadIdx.x;
  for (int r = 0; r < rows; ++r) col[r * kPostBlock] = 0u;
  const double gv = g[cell], half = (double)(B / 2), bins = (double)B;
  int below[kLev];
#pragma unroll
  for (int l = 0; l < kLev; ++l) below[l] = 0;
  const T* p = beds + cell;
  auto count = [&](T b) {
    const double x = (double)b;
    const int s = hist_slot(x - gv, inv_w, half, bins, B);
    atomicAdd(&col[(s >> 1) * kPostBlock], 1u << ((s & 1) * 16));
#pragma unroll
    for (int l = 0; l < kLev; ++l) below[l] += x < lev.v[l] ? 1 : 0;
  };
  int c = c0;
  for (; c + kHistChains <= c1; c += kHistChains) {
    T b[kHistChains];
#pragma unroll
    for (int j = 0; j < kHistChains; ++j) b[j] = p[(int64_t)(c + j) * plane];
#pragma unroll
    for (int j = 0; j < kHistChains; ++j) count(b[j]);
  }
  for (; c < c1; ++c) count(p[(int64_t)c * plane]);
  int32_t* out = counts + cell;
  for (int r = 0; r < rows; ++r) {
    const uint32_t v = col[r * kPostBlock];
    const int lo = (int)(v & 0xffffu), hi = (int)(v >> 16);      // slot 2r + 1 == B + 3 does not exist and is never counted
    if (lo) atomicAdd(out + (int64_t)(2 * r) * plane, lo);
    if (hi) atomicAdd(out + (int64_t)(2 * r + 1) * plane, hi);
  }
#pragma unroll
  for (int l = 0; l < kLev; ++l)
    if (l < n_levels && below[l]) atomicAdd(out + (int64_t)(B + 3 + l) * plane, below[l]);
}

template <typename T, int kLev>
void hist_t(const void* beds, const double* g, double inv_w, int B, const HistLevels& lev, int n_levels, int32_t* counts, int64_t plane,
            int n_chains, int parts, int cpp, hipStream_t st) {
  const dim3 grid((unsigned)posterior_cell_blocks(plane, 1), (unsigned)parts);
  if (B <= 32)
    hipLaunchKernelGGL((post_hist_kernel<T, 18, kLev>), grid, dim3(kPostBlock), 0, st, (const T*)beds, g, inv_w, B, lev, n_levels, counts, plane, n_chains, cpp);
  else if (B <= 64)
    hipLaunchKernelGGL((post_hist_kernel<T, 34, kLev>), grid, dim3(kPostBlock), 0, st, (const T*)beds, g, inv_w, B, lev, n_levels, counts, plane, n_chains, cpp);
  else
    hipLaunchKernelGGL((post_hist_kernel<T, 66, kLev>), grid, dim3(kPostBlock), 0, st, (const T*)beds, g, inv_w, B, lev, n_levels, counts, plane, n_chains, cpp);
}

// parts of the chain axis for the histogram: posterior_parts, raised where a part would hold more chains than a 16-bit counter counts
int posterior_hist_parts(int64_t cell_blocks, int n_chains, int n_cu) {
  return std::max(posterior_parts(cell_blocks, n_chains, n_cu), (n_chains + kHistMaxCpp - 1) / kHistMaxCpp);
}

}  // namespace

hipError_t launch_posterior_histogram(const void* beds, const double* g, double inv_w, int n_bins, const double* levels, int n_levels,
                                      int32_t* counts, int64_t plane, int n_chains, int f32_state, int n_cu, hipStream_t st) {
  HistLevels lev;
  for (int l = 0; l < kHistMaxLevels; ++l) lev.v[l] = l < n_levels ? levels[l] : -__builtin_inf();
  const int parts = posterior_hist_parts(posterior_cell_blocks(plane, 1), n_chains, n_cu);
  const int cpp = chains_per_part(n_chains, parts);
  dispatch_state(f32_state, [&](auto tag) {
    using T = typename decltype(tag)::T;
    if (n_levels <= 2) hist_t<T, 2>(beds, g, inv_w, n_bins, lev, n_levels, counts, plane, n_chains, parts, cpp, st);
    else hist_t<T, kHistMaxLevels>(beds, g, inv_w, n_bins, lev, n_levels, counts, plane, n_chains, parts, cpp, st);
  });
  return hipGetLastError();
}

}  // namespace gsm
