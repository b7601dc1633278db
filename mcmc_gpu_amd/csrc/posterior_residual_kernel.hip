// Posterior mass-conservation residual maps: per snapshot, for every chain c of the handle the residual r_c = cell_residual of
// (double)bed_c (residual_device.h: the function gsm_residual evaluates, so r_c has gsm_residual's bits) and, per cell over the
// chains with finite r_c, cnt += 1, S1 += d, S2 += d * d with d = r_c - rg, and per level A_l += (|r_c| > level_l)
// (include/gsm.h, gsm_posterior_residual).  Stencil and accumulation in one pass: no per-chain residual is stored.  The reference
// draws the residual map of one bed (Topography.get_mass_conservation_residual, Topography.py:592-612, in visualization.ipynb).
//
// Tile.  A workgroup of 256 lanes owns ly rows x lx * V columns of the grid, lx = min(32, the power of two that holds W / V)
// lanes across and ly = 256 / lx rows, V cells of one row per lane: 16 bytes of bed where W allows it (fp64: 2, fp32: 4), so
// 8 rows x 64 columns (fp64) or 8 x 128 (fp32) on a grid of 256 columns -- 512-byte row segments.  A grid narrower than the
// tile gives taller tiles (64 x 64 fp64: 8 rows of the full width; 70 x 3: 64 rows x 4 lanes).  Workgroup (tile, part) walks the
// chains of its part of the chain axis in index order.  Per chain a lane loads its own 16 bytes, the 16 bytes above and below
// and the one value left and right of them -- five loads, kResChains chains' worth issued together; rows and columns past a
// border are clamped onto the lane's own cells, which is also what np.gradient's one-sided differences read.  The neighbours'
// loads are the loads other lanes of the workgroup make for themselves (L1), except a tile's halo: one row above and below and
// one 128-byte line left and right per row.  The workgroup id is remapped (xcd_contiguous) so that the workgroups sharing an L2
// hold consecutive tiles of one part -- the tiles whose halos they read -- at the same time; placement changes the speed only.
//
// Registers.  Everything that does not depend on the chain is loaded once per workgroup and kept across the chain loop: per
// cell velx / surf left and right, vely / surf above and below, dhdt, smb (the operands cell_residual reads; the loop holds no
// store, so their loads are hoisted out of it), rg, and the accumulators S1, S2 (fp64) and cnt, A_0 .. A_3 (int32: a part holds
// fewer than 2^31 chains).  The four levels are kernel arguments; a level that was not asked for is +inf and counts nothing.
//
// Sums.  fp64 whatever the state type, no fused multiply-add, no atomics; chains in index order within a part, each part to its
// own slab, post_combine_kernel (posterior_kernel.hip) adds the slabs in part order onto `sums`.  A part without chains writes zeros.
#include "posterior_device.h"
#include "residual_device.h"
#include <cmath>

namespace gsm {
namespace {

constexpr int kResChains = 4;      // chains whose five loads per lane are in flight together

struct ResLevels { double v[kResMaxLevels]; };

// what a lane reads of one chain: its V cells, the V cells above and below, the cell left of the first and right of the last
template <typename T, int V>
struct ResWindow { Pack<T, V> mid, up, dn; T left, right; };

template <typename T, int V>
__global__ __launch_bounds__(kPostBlock) void post_residual_kernel(const StaticFields S, const T* __restrict__ beds,
                                                                   const double* __restrict__ rg, const ResLevels lev,
                                                                   double* __restrict__ slab, int n_chains, int cpp, int n_fields, int lx_log2,
                                                                   int tiles_x, int tiles) {
  using PT = Pack<T, V>;
  const int item = xcd_contiguous(blockIdx.x, gridDim.x);
  const int part = item / tiles, tile = item % tiles;
  const int lx = threadIdx.x & ((1 << lx_log2) - 1), ly = threadIdx.x >> lx_log2;
  const int H = S.H, W = S.W;
  const int r = (tile / tiles_x) * (kPostBlock >> lx_log2) + ly;
  const int c = (((tile % tiles_x) << lx_log2) + lx) * V;
  if (r >= H || c >= W) return;                                  // W % V == 0: a lane's V cells are inside the row or all outside
  const int64_t plane = (int64_t)H * W;
  const int ru = r == 0 ? 0 : r - 1, rd = r == H - 1 ? r : r + 1;
  const int o_mid = r * W + c, o_up = ru * W + c, o_dn = rd * W + c;
  const int o_left = r * W + (c == 0 ? 0 : c - 1), o_right = r * W + (c + V > W - 1 ? W - 1 : c + V);
  const int c0 = part * cpp, c1 = min(n_chains, c0 + cpp);

  double rgv[V], s1[V], s2[V];
  int cnt[V], above[kResMaxLevels][V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    rgv[j] = rg[o_mid + j]; s1[j] = 0.0; s2[j] = 0.0; cnt[j] = 0;
#pragma unroll
    for (int l = 0; l < kResMaxLevels; ++l) above[l][j] = 0;
  }
  auto load = [&](int chain) __attribute__((always_inline)) {
    const T* __restrict__ b = beds + (int64_t)chain * plane;
    ResWindow<T, V> w;
    w.mid = *reinterpret_cast<const PT*>(b + o_mid);
    w.up = *reinterpret_cast<const PT*>(b + o_up);
    w.dn = *reinterpret_cast<const PT*>(b + o_dn);
    w.left = b[o_left];
    w.right = b[o_right];
    return w;
  };
  auto fold = [&](const ResWindow<T, V>& w) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int cj = c + j;
      // cell_residual asks for (r, cj +- 1) and (r +- 1, cj), or for the cell itself where a border clamps the neighbour onto it
      const double self = (double)w.mid.v[j], up = (double)w.up.v[j], dn = (double)w.dn.v[j];
      const double left = (double)(j > 0 ? w.mid.v[j > 0 ? j - 1 : 0] : w.left);
      const double right = (double)(j < V - 1 ? w.mid.v[j < V - 1 ? j + 1 : 0] : w.right);
      // (all five captures are read before any of them is chosen, and chosen by value: a choice between the captures themselves
      // becomes a choice between their addresses, which keeps the closure in private memory)
      auto bed_at = [=](int rr, int cc) __attribute__((always_inline)) -> double {
        const double v_self = +self, v_left = +left, v_right = +right, v_up = +up, v_dn = +dn;
        return rr < r ? +v_up : rr > r ? +v_dn : cc < cj ? +v_left : cc > cj ? +v_right : +v_self;
      };
      const double res = cell_residual(S, r, cj, bed_at);
      const double mag = fabs(res);
      const bool finite = mag < INFINITY;                        // false for a NaN
      const double d = res - rgv[j];
      const double dd = d * d;
      s1[j] += finite ? d : 0.0;
      s2[j] += finite ? dd : 0.0;
      cnt[j] += finite ? 1 : 0;
#pragma unroll
      for (int l = 0; l < kResMaxLevels; ++l) above[l][j] += (finite && mag > lev.v[l]) ? 1 : 0;
    }
  };
  int chain = c0;
  for (; chain + kResChains <= c1; chain += kResChains) {
    ResWindow<T, V> w[kResChains];
#pragma unroll
    for (int i = 0; i < kResChains; ++i) w[i] = load(chain + i);
#pragma unroll
    for (int i = 0; i < kResChains; ++i) fold(w[i]);
  }
  for (; chain < c1; ++chain) fold(load(chain));

  double* o = slab + (int64_t)part * n_fields * plane + o_mid;
#pragma unroll
  for (int j = 0; j < V; ++j) {
    o[j] = (double)cnt[j];
    o[plane + j] = s1[j];
    o[2 * plane + j] = s2[j];
  }
#pragma unroll
  for (int l = 0; l < kResMaxLevels; ++l)
    if (3 + l < n_fields) {
#pragma unroll
      for (int j = 0; j < V; ++j) o[(3 + l) * plane + j] = (double)above[l][j];
    }
}

}  // namespace

ResTile posterior_residual_tile(int H, int W, int f32_state) {
  ResTile t;
  t.vec = f32_state ? (W % 4 == 0 ? 4 : W % 2 == 0 ? 2 : 1) : (W % 2 == 0 ? 2 : 1);
  const int lanes = W / t.vec;
  t.lx_log2 = 0;
  while (t.lx_log2 < kResMaxLanesXLog2 && (1 << t.lx_log2) < lanes) ++t.lx_log2;
  const int lx = 1 << t.lx_log2, ly = kPostBlock >> t.lx_log2;
  t.tiles_x = (lanes + lx - 1) / lx;
  t.tiles_y = (H + ly - 1) / ly;
  return t;
}

int posterior_residual_parts(const ResTile& t, int n_chains, int n_cu) {
  const int fill = posterior_parts((int64_t)t.tiles_x * t.tiles_y, n_chains, n_cu);
  return std::max(1, std::min(fill, n_chains / kResMinChains));
}

hipError_t launch_posterior_residual(const StaticFields& S, const void* beds, const double* rg, const double* levels, int n_levels,
                                     double* slab, double* sums, int n_chains, int parts, int f32_state, int n_cu, hipStream_t st) {
  const ResTile t = posterior_residual_tile(S.H, S.W, f32_state);
  const int tiles = t.tiles_x * t.tiles_y, n_fields = 3 + n_levels;
  const int64_t plane = (int64_t)S.H * S.W;
  ResLevels lev;
  for (int l = 0; l < kResMaxLevels; ++l) lev.v[l] = l < n_levels ? levels[l] : INFINITY;
  dispatch_state_vec(f32_state, t.vec, [&](auto tag) {
    using T = typename decltype(tag)::T;
    hipLaunchKernelGGL((post_residual_kernel<T, decltype(tag)::V>), dim3((unsigned)(tiles * parts)), dim3(kPostBlock), 0, st, S, (const T*)beds, rg,
                       lev, slab, n_chains, chains_per_part(n_chains, parts), n_fields, t.lx_log2, t.tiles_x, tiles);
  });
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  PostOut out{};
  for (int f = 0; f < n_fields; ++f) out.f[f] = sums + (int64_t)f * plane;
  return launch_posterior_combine(slab, parts, n_fields, plane, out, 1, n_cu, st);
}

}  // namespace gsm
