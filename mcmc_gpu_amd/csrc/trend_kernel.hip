// Batched Gaussian trend filter on gfx950 (gsm.h: gsm_gaussian_filter): scipy.ndimage.gaussian_filter(x, sigma, mode='reflect') of n
// fields [n, H, W] at once, fp64, two separable passes -- axis 0 (down the rows) first, then axis 1 (along a row) on its result, as
// scipy orders them.  The weights are the caller's (two host arrays made in NumPy's arithmetic): no exponential is evaluated here, and
// they travel in the kernel arguments, so that every weight of a wavefront is a scalar operand.
//
// Replaces, for a stack of beds:
//   trend = sp.ndimage.gaussian_filter(initial_bed, sigma=10)      smallScaleChain_multiprocessing.py:486
//   (scipy/ndimage/_filters.py gaussian_filter -> gaussian_filter1d -> correlate1d per axis, _ni_support.c NI_EXTEND_REFLECT)
//
// Arithmetic of BOTH passes, the same for every cell of every field:
//   acc = 0;  for k = 0, 1, .. 2 lw in this order:  acc = fma(w[k], x[refl(i + k - lw)], acc)
// one fused multiply-add per tap, one accumulator, refl the half-sample-symmetric reflection of period 2 n (d c b a | a b c d | d c b a).
// Nothing of a cell's sum depends on the batch, on the tiling or on the lane that computes it: field r of a batch has the bits of the
// one-field call.  No atomics.  NaN and infinities propagate by this arithmetic alone: a tap is never skipped and no zero is ever
// multiplied in from outside the 2 lw + 1 taps.
#include "gsm_internal.h"

namespace gsm {

// index i of an axis of n cells under mode='reflect'; any i, n >= 1 (folds as often as it takes; n = 1 gives 0)
__host__ __device__ __forceinline__ int trend_refl(int i, int n) {
  const int p = 2 * n;
  int m = i % p;
  if (m < 0) m += p;
  return m < n ? m : p - 1 - m;
}

// ---- axis 0: a lane owns a column, a wavefront 64 adjacent columns (coalesced rows of 512 bytes) and kTrendRun consecutive output
// rows.  It walks down the 2 lw + kTrendRun input rows once; each value is used from its register for the up to kTrendRun outputs whose
// window holds it (output r takes input row j with tap k = j - r: k ascends with j, the order stated above).  Input rows overlap
// between neighbouring wavefronts and are served by the caches; there is no LDS tile.  Every row index comes from refl and the column is
// clamped to W - 1: no read leaves the field.
constexpr int kTrendRun = 16, kTrendRows = 8;
__global__ __launch_bounds__(256) void trend_axis0_kernel(const TrendTaps T, const double* __restrict__ x, double* __restrict__ out,
                                                          int H, int W, int col_tiles, int row_chunks) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int b = blockIdx.x;
  const int ct = b % col_tiles; b /= col_tiles;
  const int rc = b % row_chunks;
  const int field = b / row_chunks;
  const int i0 = (rc * 4 + wave) * kTrendRun;                 // first output row of this wavefront
  if (i0 >= H) return;
  const int c = ct * 64 + lane;
  const int cc = min(c, W - 1);                               // lanes past the last column read it and store nothing
  const double* xf = x + (size_t)field * H * W + cc;
  const int taps = 2 * T.lw + 1, p = 2 * H;
  int m = (i0 - T.lw) % p;                                    // (i0 - lw + j) mod 2 H, kept by increments
  if (m < 0) m += p;
  double acc[kTrendRun];
#pragma unroll
  for (int r = 0; r < kTrendRun; ++r) acc[r] = 0.0;
  // one input row into the outputs whose window holds it (taps k = j - r outside [0, taps) skipped): the ramps at both ends of the walk
  auto one_row = [&](int j) {
    const int row = m < H ? m : p - 1 - m;
    if (++m == p) m = 0;
    const double v = xf[(size_t)row * W];
#pragma unroll
    for (int r = 0; r < kTrendRun; ++r) {
      const int k = j - r;
      if (k >= 0 && k < taps) acc[r] = fma(T.w[k], v, acc[r]);
    }
  };
  int j = 0;
  for (; j < min(kTrendRun - 1, taps + kTrendRun - 1); ++j) one_row(j);
  // while every output's window holds the row: kTrendRows rows at a time -- their loads and the kTrendRun - 1 + kTrendRows weights they
  // meet are requested together, then kTrendRows x kTrendRun multiply-adds run on registers (a row at a time left every load's latency
  // exposed: this pass took 0.90 ms at 1024 x 256^2, the whole call 1.29 ms; it takes 0.89 ms now).  Each output still takes its taps in
  // ascending order.
  for (; j + kTrendRows <= taps; j += kTrendRows) {
    double wv[kTrendRun - 1 + kTrendRows], xv[kTrendRows];
#pragma unroll
    for (int t = 0; t < kTrendRun - 1 + kTrendRows; ++t) wv[t] = T.w[j - (kTrendRun - 1) + t];
#pragma unroll
    for (int u = 0; u < kTrendRows; ++u) {
      const int row = m < H ? m : p - 1 - m;
      if (++m == p) m = 0;
      xv[u] = xf[(size_t)row * W];
    }
#pragma unroll
    for (int u = 0; u < kTrendRows; ++u)
#pragma unroll
      for (int r = 0; r < kTrendRun; ++r) acc[r] = fma(wv[u + kTrendRun - 1 - r], xv[u], acc[r]);      // tap (j + u) - r
  }
  for (; j < taps + kTrendRun - 1; ++j) one_row(j);
  if (c >= W) return;
  double* of = out + (size_t)field * H * W + c;
#pragma unroll
  for (int r = 0; r < kTrendRun; ++r)
    if (i0 + r < H) of[(size_t)(i0 + r) * W] = acc[r];
}

// ---- axis 1: a workgroup of 128 threads takes 256 adjacent cells of one row with a halo of lw either side into LDS (reflected on the
// way in), and a thread computes the two adjacent outputs 2 t and 2 t + 1 from 16-byte LDS reads (lanes read consecutive 16-byte slots:
// no bank conflict): lw + 1 reads for 2 (2 lw + 1) multiply-adds.  Output 2 t takes pair m's .x as tap 2 m and .y as tap 2 m + 1; output
// 2 t + 1 takes pair m's .y as tap 2 m and pair m + 1's .x as tap 2 m + 1: both in the order stated above.
constexpr int kTrendSeg = 256;
__global__ __launch_bounds__(kTrendSeg / 2) void trend_axis1_kernel(const TrendTaps T, const double* __restrict__ x, double* __restrict__ out,
                                                                    int W, int segs) {
  __shared__ double2 seg2[(kTrendSeg + 2 * kTrendMaxLw + 2) / 2];
  double* seg = (double*)seg2;
  const int tid = threadIdx.x;
  const size_t rowi = blockIdx.x / segs;                       // row of the stack, field * H + i
  const int c0 = (int)(blockIdx.x % segs) * kTrendSeg;
  const int lw = T.lw;
  const double* xr = x + rowi * W;
  for (int q = tid; q < kTrendSeg + 2 * lw + 1; q += kTrendSeg / 2) seg[q] = xr[trend_refl(c0 - lw + q, W)];   // one cell past the last window: pair lw of an odd output
  __syncthreads();
  double a0 = 0.0, a1 = 0.0;
  double2 prev = seg2[tid];
  for (int mm = 0; mm < lw; ++mm) {
    const double2 cur = seg2[tid + mm + 1];
    const double wa = T.w[2 * mm], wb = T.w[2 * mm + 1];
    a0 = fma(wa, prev.x, a0); a0 = fma(wb, prev.y, a0);
    a1 = fma(wa, prev.y, a1); a1 = fma(wb, cur.x, a1);
    prev = cur;
  }
  a0 = fma(T.w[2 * lw], prev.x, a0);
  a1 = fma(T.w[2 * lw], prev.y, a1);
  const int c = c0 + 2 * tid;
  double* orow = out + rowi * W;
  if (c < W) orow[c] = a0;
  if (c + 1 < W) orow[c + 1] = a1;
}

hipError_t launch_gaussian_filter(const TrendTaps& t0, const TrendTaps& t1, const double* x, double* tmp, double* out, int n, int H, int W,
                                  hipStream_t st) {
  const int col_tiles = (W + 63) / 64, row_chunks = (H + 4 * kTrendRun - 1) / (4 * kTrendRun), segs = (W + kTrendSeg - 1) / kTrendSeg;
  const int64_t g0 = (int64_t)n * col_tiles * row_chunks, g1 = (int64_t)n * H * segs;
  if (g0 > INT32_MAX || g1 > INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(trend_axis0_kernel, dim3((unsigned)g0), dim3(256), 0, st, t0, x, tmp, H, W, col_tiles, row_chunks);
  hipLaunchKernelGGL(trend_axis1_kernel, dim3((unsigned)g1), dim3(kTrendSeg / 2), 0, st, t1, tmp, out, W, segs);
  return hipGetLastError();
}

}  // namespace gsm
