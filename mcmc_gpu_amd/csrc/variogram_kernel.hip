// Variogram map of gridded fields (gsm_variogram_map): per field and integer offset (di, dj) of the half plane di in [0, mi],
// dj in [-mj, mj], the sum of (z[i, j] - z[i + di, j + dj])^2 over the pairs with both cells inside the grid, finite and unmasked,
// and the number of those pairs.  On a uniform axis-aligned grid the separation of two cells is a function of their offset alone,
// so every experimental variogram (isotropic or directional, any bin edges) is host arithmetic on this table.
//
// One wavefront per workgroup.  A workgroup owns one field, kVarDi consecutive row offsets, 64 consecutive column offsets (one
// per lane) and the rows [row0, row1) of one part.  Per row i and per tile of kVarJt columns it stages z[i, j0 ..] and the
// kVarDi rows z[i + di, j0 + dj_lo ..] in LDS, a missing cell (outside the grid, not finite, masked) as NaN; then lane l walks
// the tile: a[j] is one address for the whole wave (a broadcast), b[k][j + l] is consecutive across the lanes (no bank
// conflict), and one a feeds kVarDi pairs.  A pair counts when its difference is not NaN.  Sum and count of a lane stay in its
// registers over the whole row range, in the order (i, j) ascending: no cross-lane step, no atomics, and nothing that depends on
// the number of fields or on the device.  With several parts each writes its partial and variogram_combine_kernel adds them in
// part order.
#include "gsm_internal.h"
#include <algorithm>

namespace gsm {

constexpr int kVarDi = 4;                      // row offsets per workgroup (register block: one a[j] read feeds this many pairs)
constexpr int kVarJt = 128;                    // columns of a[] per LDS tile
constexpr int kVarBw = kVarJt + 63;            // columns of b[][] per tile: lane l reads b[.][jj + l], jj < kVarJt, l < 64

// a cell's value as the pair loop takes it: NaN when it is missing (not finite, or masked out)
__device__ __forceinline__ double variogram_cell(const double* __restrict__ z, const uint8_t* __restrict__ mask, int64_t c) {
  const double v = z[c];
  return (fabs(v) <= 1.79769313486231570815e308) && (!mask || mask[c]) ? v : __builtin_nan("");
}

int variogram_default_rows_per_part(int H, int W, int mi, int mj) {
  // enough workgroups for every CU when there is one field, at least 16 rows per part; a function of the shape only
  const int64_t units = (int64_t)((std::min(mi, H - 1) + kVarDi) / kVarDi) * ((2 * (int64_t)std::min(mj, W - 1) + 1 + 63) / 64);
  const int64_t want = (2048 + units - 1) / units;
  const int64_t rpp = std::max<int64_t>(16, (H + want - 1) / want);
  return (int)std::min<int64_t>(rpp, H);
}

__global__ __launch_bounds__(64) void variogram_map_kernel(const double* __restrict__ fields, const uint8_t* __restrict__ mask, int H, int W,
                                                           int mi, int mj, int rows_per_part, int parts, int n_djt,
                                                           double* __restrict__ sum, long long* __restrict__ count) {
  __shared__ double sa[kVarJt];
  __shared__ double sb[kVarDi][kVarBw];
  const int lane = threadIdx.x;
  const int djt = blockIdx.x % n_djt, dib = blockIdx.x / n_djt;
  const int part = blockIdx.y;
  const int64_t r = blockIdx.z;
  const int ndj = 2 * mj + 1;
  const int di0 = dib * kVarDi;
  const int dj_lo = djt * 64 - mj;             // column offset of lane 0
  const double* z = fields + r * (int64_t)H * W;
  const double nan = __builtin_nan("");
  const int row0 = part * rows_per_part;
  const int row1 = min(row0 + rows_per_part, H - di0);      // rows i with i + di0 < H: the others have no pair in this block
  double s[kVarDi];
  long long n[kVarDi];
#pragma unroll
  for (int k = 0; k < kVarDi; ++k) { s[k] = 0.0; n[k] = 0; }
  // columns j with a partner j + dj inside the grid for some lane of this workgroup: j + dj_lo + 63 >= 0, j + dj_lo < W
  const int jbeg = max(0, -(dj_lo + 63)) / kVarJt * kVarJt;
  const int jend = (int)min((int64_t)W, (int64_t)W - dj_lo);
  for (int i = row0; i < row1; ++i) {
    for (int j0 = jbeg; j0 < jend; j0 += kVarJt) {
      __syncthreads();
      for (int x = lane; x < kVarJt; x += 64) {
        const int j = j0 + x;
        sa[x] = j < W ? variogram_cell(z, mask, (int64_t)i * W + j) : nan;
      }
#pragma unroll
      for (int k = 0; k < kVarDi; ++k) {
        const int ib = i + di0 + k;
        for (int x = lane; x < kVarBw; x += 64) {
          const int64_t j = (int64_t)j0 + dj_lo + x;
          sb[k][x] = ib < H && di0 + k <= mi && j >= 0 && j < W ? variogram_cell(z, mask, (int64_t)ib * W + j) : nan;
        }
      }
      __syncthreads();
      int c[kVarDi];
#pragma unroll
      for (int k = 0; k < kVarDi; ++k) c[k] = 0;
#pragma unroll 4
      for (int jj = 0; jj < kVarJt; ++jj) {
        const double a = sa[jj];
#pragma unroll
        for (int k = 0; k < kVarDi; ++k) {
          const double d = a - sb[k][jj + lane];
          const bool ok = d == d;
          s[k] += ok ? d * d : 0.0;
          c[k] += ok;
        }
      }
#pragma unroll
      for (int k = 0; k < kVarDi; ++k) n[k] += c[k];
    }
  }
  const int t = djt * 64 + lane;               // index of this lane's column offset, dj = t - mj
  if (t >= ndj) return;
#pragma unroll
  for (int k = 0; k < kVarDi; ++k) {
    const int di = di0 + k;
    if (di > mi) break;
    const bool defined = di > 0 || t > mj;     // (0, dj <= 0) is the mirror image of (0, -dj): defined as zero
    const int64_t o = ((r * parts + part) * (mi + 1) + di) * ndj + t;
    sum[o] = defined ? s[k] : 0.0;
    count[o] = defined ? n[k] : 0;
  }
}

// sum[r][o] = partial[r][0][o] + partial[r][1][o] + ... in part order
__global__ __launch_bounds__(256) void variogram_combine_kernel(const double* __restrict__ psum, const long long* __restrict__ pcount, int64_t n_off,
                                                                int parts, double* __restrict__ sum, long long* __restrict__ count) {
  const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t r = blockIdx.y;
  if (o >= n_off) return;
  const int64_t base = r * parts * n_off + o;
  double s = psum[base];
  long long n = pcount[base];
  for (int p = 1; p < parts; ++p) {
    s += psum[base + p * n_off];
    n += pcount[base + p * n_off];
  }
  sum[r * n_off + o] = s;
  count[r * n_off + o] = n;
}

int variogram_parts(int H, int rows_per_part) { return (H + rows_per_part - 1) / rows_per_part; }
int64_t variogram_workgroups(int mi, int mj) { return (int64_t)((mi + kVarDi) / kVarDi) * ((2 * (int64_t)mj + 1 + 63) / 64); }

hipError_t launch_variogram_map(const double* fields, int n_fields, const uint8_t* mask, int H, int W, int mi, int mj, int rows_per_part,
                                double* psum, int64_t* pcount, double* sum, int64_t* count, hipStream_t st) {
  const int parts = variogram_parts(H, rows_per_part);
  const int n_djt = (2 * mj + 1 + 63) / 64;
  const int64_t n_off = (int64_t)(mi + 1) * (2 * mj + 1);
  dim3 grid((unsigned)variogram_workgroups(mi, mj), (unsigned)parts, (unsigned)n_fields);
  if (parts == 1) {
    variogram_map_kernel<<<grid, 64, 0, st>>>(fields, mask, H, W, mi, mj, rows_per_part, 1, n_djt, sum, (long long*)count);
    return hipGetLastError();
  }
  variogram_map_kernel<<<grid, 64, 0, st>>>(fields, mask, H, W, mi, mj, rows_per_part, parts, n_djt, psum, (long long*)pcount);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  variogram_combine_kernel<<<dim3((unsigned)((n_off + 255) / 256), (unsigned)n_fields), 256, 0, st>>>(psum, (const long long*)pcount, n_off, parts, sum,
                                                                                                      (long long*)count);
  return hipGetLastError();
}

}  // namespace gsm
