// Posterior covariance of every cell with its neighbours: per snapshot, for reach R in 1 .. 4 and the K = 2 R^2 + 2 R offsets of
// the upper half plane -- (0, 1) .. (0, R), then for di = 1 .. R: (di, -R) .. (di, R) --
//   cross[k, i, j] += sum_c d_c[i, j] * d_c[i + di_k, j + dj_k],   d_c = (double)bed_c - g,
// where the partner lies inside the grid (include/gsm.h, gsm_posterior_local).  The reference can reach a covariance across cells
// only through the whole-bed host cache of one chain (bed_cache of chain_crf.run, MCMC.py:1198, :1363).
//
// Tile.  A workgroup of 256 lanes owns kLocRows = 8 rows x kLocCols = 64 columns of the grid, 32 lanes across and 2 cells of one
// row per lane, whatever the state type and the width's parity (no lane loads its own cells: see Staging).  Workgroup (tile, part)
// walks the chains of its part of the chain axis in index order; the workgroup id is remapped (xcd_contiguous) so that the
// workgroups sharing an L2 hold consecutive tiles of one part, the tiles whose halos they read.  Placement changes the speed only.
//
// Staging.  Each state value is used in up to 2 K fused multiply-adds (as a cell and as a partner), so it is fetched once, turned
// into d once and shared through LDS: per chain the workgroup stages d of its tile and the halo -- R rows below, R columns on
// both sides -- as (8 + R) x (64 + 2 R) doubles, 0 outside the grid.  A lane stages the same nStage positions for every chain
// (position e = i * 256 + lane of the halo'd tile, row-major) and keeps g at them in registers: g is read once per workgroup and
// subtracted once per value.  kChains chains are staged together and the stage buffer is double: the global loads of the next
// kChains chains are issued before the arithmetic on the present ones and written to the other buffer after it, one barrier per
// kChains chains.
//
// Arithmetic.  Per chain and di a lane reads the row segment [c - R, c + 2 + R) of row r + di from LDS into registers, 1 + R reads
// of 16 bytes at a lane stride of 16 bytes (conflict-free, 256 B per clock), and slides its two cells over it: (2 R + 1) x 2
// multiply-adds per 2 + 2 R values read.  Taking every partner with a read of its own would cost K reads of 8 bytes per value and
// put the pass an LDS-bound factor of two behind the fp64 multiply-add rate.  The 2 K accumulators stay in
// registers across the chain loop, indexed by unrolled offsets only: hence one instantiation per reach.
//
// Sums.  fp64 whatever the state type, fused multiply-adds, no atomics; chains in index order within a part, each part to its
// own slab, post_combine_kernel (posterior_kernel.hip) adds the slabs in part order onto `cross`.  An entry whose partner is outside
// the grid is written as 0 to the slab, whatever the halo held (a NaN d times the halo's 0 is not stored).  A part without chains
// writes zeros.  The slab holds the offsets in groups of G <= 15 (one PostOut each): offset k of part p is plane
// ((k / G) * parts + p) * G + k % G.
#include "posterior_device.h"
#include <type_traits>

namespace gsm {
namespace {

constexpr int kLocLanesX = 32, kLocVec = 2;
constexpr int kLocRows = kPostBlock / kLocLanesX, kLocCols = kLocLanesX * kLocVec;

__host__ __device__ constexpr int loc_offsets(int R) { return 2 * R * R + 2 * R; }
// offsets per group of the slab: all of them up to 15, else the largest divisor of K that one PostOut holds (24: 12, 40: 10)
__host__ __device__ constexpr int loc_group(int R) { return R <= 2 ? loc_offsets(R) : R == 3 ? 12 : 10; }
// chains staged together: their loads are in flight together; fewer where the accumulators leave fewer registers (staging four at
// reach 4 fits, 246 VGPRs, and measured no different: DESIGN 5.4.4)
__host__ __device__ constexpr int loc_chains(int R) { return R <= 2 ? 4 : 2; }

struct alignas(16) D2 { double v[2]; };

template <typename T, int R>
__global__ __launch_bounds__(kPostBlock) void post_local_kernel(const T* __restrict__ beds, const double* __restrict__ g,
                                                                double* __restrict__ slab, int H, int W, int n_chains, int cpp, int parts,
                                                                int tiles_x, int tiles) {
  constexpr int K = loc_offsets(R), G = loc_group(R), kChains = loc_chains(R);
  constexpr int LH = kLocRows + R, LW = kLocCols + 2 * R, kStageCells = LH * LW;
  constexpr int nStage = (kStageCells + kPostBlock - 1) / kPostBlock;
  __shared__ D2 stage[2][kChains][kStageCells / 2];                  // LW is even: a row starts on 16 bytes
  const int item = xcd_contiguous(blockIdx.x, gridDim.x);
  const int part = item / tiles, tile = item % tiles;
  const int lx = threadIdx.x % kLocLanesX, ly = threadIdx.x / kLocLanesX;
  const int r0 = (tile / tiles_x) * kLocRows, c0 = (tile % tiles_x) * kLocCols;
  const int64_t plane = (int64_t)H * W;
  const int ch0 = part * cpp, ch1 = min(n_chains, ch0 + cpp);

  // what this lane stages of every chain: nStage positions of the halo'd tile, g at them, -1 for a position outside the grid
  int s_off[nStage];
  double s_g[nStage];
#pragma unroll
  for (int i = 0; i < nStage; ++i) {
    const int e = i * kPostBlock + threadIdx.x;
    const int rr = r0 + e / LW, cc = c0 - R + e % LW;
    const bool in = e < kStageCells && rr < H && cc >= 0 && cc < W;
    s_off[i] = in ? rr * W + cc : -1;
    s_g[i] = in ? g[s_off[i]] : 0.0;
  }
  T s_bed[kChains][nStage];
  auto fetch = [&](int chain) __attribute__((always_inline)) {    // chain .. chain + kChains - 1, those below ch1
#pragma unroll
    for (int q = 0; q < kChains; ++q)
      if (chain + q < ch1) {
        const T* __restrict__ b = beds + (int64_t)(chain + q) * plane;
#pragma unroll
        for (int i = 0; i < nStage; ++i) s_bed[q][i] = s_off[i] >= 0 ? b[s_off[i]] : (T)0;
      }
  };
  auto put = [&](int chain, int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < kChains; ++q)
      if (chain + q < ch1) {
        double* s = &stage[buf][q][0].v[0];
#pragma unroll
        for (int i = 0; i < nStage; ++i) {
          const int e = i * kPostBlock + threadIdx.x;
          if (e < kStageCells) s[e] = s_off[i] >= 0 ? (double)s_bed[q][i] - s_g[i] : 0.0;
        }
      }
  };

  double acc[K][kLocVec];
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int j = 0; j < kLocVec; ++j) acc[k][j] = 0.0;

  // one staged chain: row ly + di of the stage, columns lx * 2 .. lx * 2 + 2 + 2 R (stage column s is grid column c - R + s)
  auto fold = [&](const D2* __restrict__ s) __attribute__((always_inline)) {
    double own[kLocVec];
#pragma unroll
    for (int di = 0; di <= R; ++di) {
      const D2* __restrict__ row = s + ((ly + di) * LW) / 2 + lx;
      double seg[2 + 2 * R];
#pragma unroll
      for (int i = 0; i < 1 + R; ++i) {
        if (di == 0 && 2 * i + 1 < R) continue;                      // left of the lane's own cells: the row of the cell pairs to the right only
        const D2 v = row[i];
        seg[2 * i] = v.v[0];
        seg[2 * i + 1] = v.v[1];
      }
      if (di == 0) {
#pragma unroll
        for (int j = 0; j < kLocVec; ++j) own[j] = seg[R + j];
#pragma unroll
        for (int dj = 1; dj <= R; ++dj)
#pragma unroll
          for (int j = 0; j < kLocVec; ++j) acc[dj - 1][j] = __builtin_fma(own[j], seg[R + j + dj], acc[dj - 1][j]);
      } else {
#pragma unroll
        for (int dj = -R; dj <= R; ++dj)
#pragma unroll
          for (int j = 0; j < kLocVec; ++j) {
            constexpr int kRow = 2 * R + 1;
            const int k = R + (di - 1) * kRow + dj + R;
            acc[k][j] = __builtin_fma(own[j], seg[R + j + dj], acc[k][j]);
          }
      }
    }
  };

  if (ch0 < ch1) {
    fetch(ch0);
    put(ch0, 0);
  }
  __syncthreads();
  int buf = 0;
  for (int chain = ch0; chain < ch1; chain += kChains, buf ^= 1) {
    const int next = chain + kChains;
    if (next < ch1) fetch(next);
#pragma unroll
    for (int q = 0; q < kChains; ++q)
      if (chain + q < ch1) fold(&stage[buf][q][0]);
    if (next < ch1) put(next, buf ^ 1);
    __syncthreads();                                                 // the other buffer is full, and this one has been read by all
  }

  const int r = r0 + ly, c = c0 + lx * kLocVec;
  if (r >= H) return;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    constexpr int kRow = 2 * R + 1;
    const int di = k < R ? 0 : 1 + (k - R) / kRow, dj = k < R ? k + 1 : (k - R) % kRow - R;
    double* o = slab + ((int64_t)((k / G) * parts + part) * G + k % G) * plane + (int64_t)r * W;
#pragma unroll
    for (int j = 0; j < kLocVec; ++j) {
      const int cj = c + j;
      if (cj < W) o[cj] = (r + di < H && cj + dj >= 0 && cj + dj < W) ? acc[k][j] : 0.0;
    }
  }
}

// f(R as an integral constant)
template <typename F>
void dispatch_reach(int reach, F&& f) {
  if (reach == 1) f(std::integral_constant<int, 1>{});
  else if (reach == 2) f(std::integral_constant<int, 2>{});
  else if (reach == 3) f(std::integral_constant<int, 3>{});
  else f(std::integral_constant<int, 4>{});
}

}  // namespace

int64_t posterior_local_tiles(int H, int W) {
  return (int64_t)((H + kLocRows - 1) / kLocRows) * ((W + kLocCols - 1) / kLocCols);
}

int posterior_local_parts(int H, int W, int reach, int n_chains, int n_cu) {
  const int K = loc_offsets(reach);
  const int64_t plane = (int64_t)H * W;
  if ((int64_t)K * plane > kLocalMaxSlabDoubles) return 0;
  const int64_t fill = posterior_parts(posterior_local_tiles(H, W), n_chains, n_cu);
  return (int)std::max<int64_t>(1, std::min<int64_t>({fill, (int64_t)(kLocalSlabPlanes / K), kLocalMaxSlabDoubles / (K * plane)}));
}

hipError_t launch_posterior_local(const void* beds, const double* g, double* slab, double* cross, int H, int W, int n_chains, int parts,
                                  int reach, int f32_state, int n_cu, hipStream_t st) {
  const int tiles_x = (W + kLocCols - 1) / kLocCols;
  const int tiles = (int)posterior_local_tiles(H, W);
  const int64_t plane = (int64_t)H * W;
  const int cpp = chains_per_part(n_chains, parts);
  dispatch_reach(reach, [&](auto rc) {
    constexpr int R = decltype(rc)::value;
    if (f32_state)
      hipLaunchKernelGGL((post_local_kernel<float, R>), dim3((unsigned)(tiles * parts)), dim3(kPostBlock), 0, st, (const float*)beds, g, slab, H, W,
                         n_chains, cpp, parts, tiles_x, tiles);
    else
      hipLaunchKernelGGL((post_local_kernel<double, R>), dim3((unsigned)(tiles * parts)), dim3(kPostBlock), 0, st, (const double*)beds, g, slab, H,
                         W, n_chains, cpp, parts, tiles_x, tiles);
  });
  hipError_t e = hipGetLastError();
  const int K = loc_offsets(reach), G = loc_group(reach);
  for (int grp = 0; grp < K / G && e == hipSuccess; ++grp) {
    PostOut out{};
    for (int f = 0; f < G; ++f) out.f[f] = cross + (int64_t)(grp * G + f) * plane;
    e = launch_posterior_combine(slab + (int64_t)grp * parts * G * plane, parts, G, plane, out, 1, n_cu, st);
  }
  return e;
}

}  // namespace gsm
