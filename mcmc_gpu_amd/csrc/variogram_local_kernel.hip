// Local variogram maps (gsm_variogram_local): the variogram map of variogram_kernel.hip per TILE of T x T cells, and per WINDOW of
// (2 k + 1) x (2 k + 1) tiles.  A pair (i, j), (i + di, j + dj) of the half plane belongs to the tile that holds its midpoint,
//   ti = (2 i + di) / (2 T),  tj = (2 j + dj) / (2 T)
// (numerators >= 0 inside the grid), so every pair belongs to exactly one tile, the tile tables add up to the global table, and a
// window is the sum of its tiles' tables: no pair is visited twice however much the windows overlap.
//
// Tile pass, variogram_tile_kernel: one wavefront per workgroup.  A workgroup owns one field, one tile row ti, kVarLocalNt
// consecutive tile columns, kVarLocalDi consecutive row offsets and 64 consecutive column offsets dj = e0 .. e0 + 63, e0 even:
// the even ones in lanes 0 .. 31 (dj = e0 + 2 l), the odd ones in lanes 32 .. 63 (dj = e0 + 1 + 2 (l - 32)).  With the doubled
// midpoint column of the even half, m2 = 2 j + dj = 2 jc + e0, as the loop variable, lane l (l' = l mod 32) pairs a[jc - l'] with
// b[jc + e0 + l'] in the even half and with b[jc + e0 + l' + 1] in the odd half: within each half of the wave -- the unit of LDS
// bank conflicts for 8-byte reads -- both run through consecutive addresses, and one a feeds kVarLocalDi pairs.  The tile column
// tj = m2 / (2 T) is the same for all lanes: m2 is even and 2 T is even, so the odd half's m2 + 1 never crosses a multiple of
// 2 T that m2 has not reached.  The whole wave enters and leaves a tile in the same iteration, and the jc of a tile column are
// one segment [seg[u], seg[u + 1]) for every lane.  The other form -- lane = dj, loop over j, a broadcast -- lets every lane cross
// a tile border at its own iteration and needs per-lane predicates.
// The workgroup walks the rows of its tile row (for row offset di the rows i with (2 i + di) / (2 T) == ti: a b row that is out of
// this range is staged as missing) and per row the jc of its tile columns in chunks of kVarLocalJt, each cell staged once per use
// through LDS (the nj + 31 and nj + 32 cells of a row that the chunk's nj midpoint columns reach), a missing cell (outside the
// grid, not finite, masked) as NaN.  A lane's sum and count of one (tile, offset) stay in its registers, in the order (i, jc) ascending, and
// are stored once: no atomics, no cross-lane step, nothing that depends on the number of fields or on the device.
//
// Window pass, variogram_window_kernel: one thread per (window, offset) adds the tiles' entries in ascending (ti, tj).
#include "gsm_internal.h"
#include <algorithm>

namespace gsm {

constexpr int kVarLocalDi = 4;                        // row offsets per workgroup (register block)
constexpr int kVarLocalNt = 4;                        // tile columns per workgroup (register block: one staged row feeds this many tiles)
constexpr int kVarLocalJt = 64;                       // midpoint columns jc per LDS chunk
constexpr int kVarLocalLw = kVarLocalJt + 32;         // cells of a[] and of b[][] per chunk: lane l reads a[31 + jj - l'] and b[.][jj + l' + (l >= 32)]

__device__ __forceinline__ double variogram_local_cell(const double* __restrict__ z, const uint8_t* __restrict__ mask, int64_t c) {
  const double v = z[c];
  return (fabs(v) <= 1.79769313486231570815e308) && (!mask || mask[c]) ? v : __builtin_nan("");
}

// ceil(x / 2) for any sign
__device__ __forceinline__ int64_t ceil_half(int64_t x) { return (x + 1) >> 1; }
__device__ __forceinline__ int64_t clamp64(int64_t x, int64_t lo, int64_t hi) { return x < lo ? lo : x > hi ? hi : x; }

// groups of 64 consecutive column offsets from the even offset -mj or -mj - 1 on (with mj odd, lane 0 of the first group is idle)
static int lane_groups(int mj) { return (2 * mj + 1 + (mj & 1) + 63) / 64; }

int64_t variogram_local_workgroups(int mi, int mj, int Tx) {
  return (int64_t)((mi + kVarLocalDi) / kVarLocalDi) * lane_groups(mj) * ((Tx + kVarLocalNt - 1) / kVarLocalNt);
}

__global__ __launch_bounds__(64) void variogram_tile_kernel(const double* __restrict__ fields, const uint8_t* __restrict__ mask, int H, int W,
                                                            int mi, int mj, int T, int Tx, int n_lg, int units,
                                                            double* __restrict__ sum, long long* __restrict__ count) {
  __shared__ double sa[kVarLocalLw];
  __shared__ double sb[kVarLocalDi][kVarLocalLw];
  const int lane = threadIdx.x, lh = lane & 31, odd = lane >> 5;
  const int unit = blockIdx.x % units, tj0 = blockIdx.x / units * kVarLocalNt;
  const int lg = unit % n_lg, dib = unit / n_lg;
  const int ti = blockIdx.y;
  const int Ty = gridDim.y;
  const int64_t r = blockIdx.z;
  const int ndj = 2 * mj + 1;
  const int di0 = dib * kVarLocalDi;
  const int dj_lo = 64 * lg - (mj + (mj & 1));      // e0: the even column offset of lane 0
  const double* z = fields + r * (int64_t)H * W;
  const double nan = __builtin_nan("");
  // rows of this tile row per row offset: (2 i + di) / (2 T) == ti and i + di < H
  int rlo[kVarLocalDi], rhi[kVarLocalDi];
  int row0 = H, row1 = 0;
#pragma unroll
  for (int k = 0; k < kVarLocalDi; ++k) {
    const int di = di0 + k;
    rlo[k] = (int)clamp64(ceil_half(2 * (int64_t)T * ti - di), 0, H);
    rhi[k] = di <= mi ? (int)clamp64(ceil_half(2 * (int64_t)T * (ti + 1) - di), 0, max(H - di, 0)) : 0;
    if (rlo[k] < rhi[k]) { row0 = min(row0, rlo[k]); row1 = max(row1, rhi[k]); }
  }
  // midpoint columns jc with a pair inside the grid for some lane: 0 <= 2 jc + dj_lo <= 2 W - 2 (the odd half's m2 + 1 lies
  // within the same limits); jc - l' >= 0 and jc + dj_lo + l' < W for some l' < 32.  A wider range would only meet missing cells.
  const int64_t jc_beg = max((int64_t)0, ceil_half(-(int64_t)dj_lo));
  const int64_t jc_end = max(jc_beg, min(min((int64_t)W + 31, (int64_t)W - dj_lo), ((2 * (int64_t)W - 2 - dj_lo) >> 1) + 1));
  // tile column tj0 + u holds the jc of [seg[u], seg[u + 1]): 2 T tj <= 2 jc + dj_lo < 2 T (tj + 1)
  int64_t seg[kVarLocalNt + 1];
#pragma unroll
  for (int u = 0; u <= kVarLocalNt; ++u) seg[u] = clamp64(ceil_half(2 * (int64_t)T * (tj0 + u) - dj_lo), jc_beg, jc_end);
  double s[kVarLocalNt][kVarLocalDi];
  int n[kVarLocalNt][kVarLocalDi];                   // an entry of one lane: at most the cells of a tile, below 2^31 (checked by the caller)
#pragma unroll
  for (int u = 0; u < kVarLocalNt; ++u)
#pragma unroll
    for (int k = 0; k < kVarLocalDi; ++k) { s[u][k] = 0.0; n[u][k] = 0; }
  for (int i = row0; i < row1; ++i) {
    for (int64_t c0 = seg[0]; c0 < seg[kVarLocalNt]; c0 += kVarLocalJt) {
      const int nj = (int)min((int64_t)kVarLocalJt, seg[kVarLocalNt] - c0), lw = nj + 32;
      __syncthreads();
      for (int x = lane; x < lw - 1; x += 64) {
        const int64_t j = c0 - 31 + x;               // a[x] = z[i, c0 - 31 + x]
        sa[x] = j >= 0 && j < W ? variogram_local_cell(z, mask, (int64_t)i * W + j) : nan;
      }
#pragma unroll
      for (int k = 0; k < kVarLocalDi; ++k) {
        const int64_t ib = (int64_t)i + di0 + k;
        const bool row_ok = i >= rlo[k] && i < rhi[k];
        for (int x = lane; x < lw; x += 64) {
          const int64_t j = c0 + dj_lo + x;          // b[k][x] = z[i + di, c0 + dj_lo + x]
          sb[k][x] = row_ok && j >= 0 && j < W ? variogram_local_cell(z, mask, ib * W + j) : nan;
        }
      }
      __syncthreads();
#pragma unroll
      for (int u = 0; u < kVarLocalNt; ++u) {
        const int j0 = (int)(max(seg[u], c0) - c0), j1 = (int)(min(seg[u + 1], c0 + nj) - c0);     // this tile's jc of the chunk
#pragma unroll 4
        for (int jj = j0; jj < j1; ++jj) {
          const double a = sa[31 + jj - lh];
#pragma unroll
          for (int k = 0; k < kVarLocalDi; ++k) {
            const double d = a - sb[k][jj + lh + odd];
            const bool ok = d == d;
            s[u][k] += ok ? d * d : 0.0;
            n[u][k] += ok;
          }
        }
      }
    }
  }
  const int t = dj_lo + 2 * lh + odd + mj;           // index of this lane's column offset, dj = t - mj
  if (t < 0 || t >= ndj) return;
#pragma unroll
  for (int u = 0; u < kVarLocalNt; ++u) {
    const int tj = tj0 + u;
    if (tj >= Tx) break;
#pragma unroll
    for (int k = 0; k < kVarLocalDi; ++k) {
      const int di = di0 + k;
      if (di > mi) break;
      const bool defined = di > 0 || t > mj;         // (0, dj <= 0) is the mirror image of (0, -dj): defined as zero
      const int64_t o = (((r * Ty + ti) * Tx + tj) * (mi + 1) + di) * ndj + t;
      sum[o] = defined ? s[u][k] : 0.0;
      count[o] = defined ? n[u][k] : 0;
    }
  }
}

// out[r][wi][wj][o] = sum of tile[r][ti][tj][o] over |ti - wi| <= k, |tj - wj| <= k inside the lattice, in ascending (ti, tj)
__global__ __launch_bounds__(256) void variogram_window_kernel(const double* __restrict__ tsum, const long long* __restrict__ tcount, int64_t n_off,
                                                               int Ty, int Tx, int k, double* __restrict__ sum, long long* __restrict__ count) {
  const int nb = (int)((n_off + 255) / 256);         // blocks per window
  const int w = blockIdx.x / nb, wi = w / Tx, wj = w % Tx;
  const int64_t o = (int64_t)(blockIdx.x % nb) * 256 + threadIdx.x;
  const int64_t r = blockIdx.z;
  if (o >= n_off) return;
  const int64_t base = r * Ty * Tx;
  double s = 0.0;
  long long n = 0;
  for (int ti = max(0, wi - k); ti <= min(Ty - 1, wi + k); ++ti)
    for (int tj = max(0, wj - k); tj <= min(Tx - 1, wj + k); ++tj) {
      const int64_t e = (base + (int64_t)ti * Tx + tj) * n_off + o;
      s += tsum[e];
      n += tcount[e];
    }
  const int64_t e = (base + (int64_t)wi * Tx + wj) * n_off + o;
  sum[e] = s;
  count[e] = n;
}

hipError_t launch_variogram_local(const double* fields, int n_fields, const uint8_t* mask, int H, int W, int mi, int mj, int T, int k,
                                  double* tsum, int64_t* tcount, double* sum, int64_t* count, hipStream_t st) {
  const int Ty = (H + T - 1) / T, Tx = (W + T - 1) / T;
  const int n_lg = lane_groups(mj);
  const int units = (mi + kVarLocalDi) / kVarLocalDi * n_lg;
  dim3 grid((unsigned)variogram_local_workgroups(mi, mj, Tx), (unsigned)Ty, (unsigned)n_fields);
  variogram_tile_kernel<<<grid, 64, 0, st>>>(fields, mask, H, W, mi, mj, T, Tx, n_lg, units, k ? tsum : sum,
                                             (long long*)(k ? tcount : count));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !k) return e;
  const int64_t n_off = (int64_t)(mi + 1) * (2 * mj + 1);
  variogram_window_kernel<<<dim3((unsigned)((n_off + 255) / 256 * Ty * Tx), 1, (unsigned)n_fields), 256, 0, st>>>(
      tsum, (const long long*)tcount, n_off, Ty, Tx, k, sum, (long long*)count);
  return hipGetLastError();
}

}  // namespace gsm
