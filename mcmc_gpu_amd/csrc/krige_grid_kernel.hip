// interpolate.krige on gfx950: the kriging estimate and its variance at every listed cell of a grid, in normal-score space.
//
// Replaces:
//   krige                     gstatsMCMC/gstatsim_custom/interpolate.py:13-89 (cell loop :46-81, radius widening :65-71)
//   neighbors (octant search) gstatsMCMC/gstatsim_custom/neighbors.py:4-64
//   ok_solve / sk_solve       gstatsMCMC/gstatsim_custom/_krige.py:5-81
//
// Kriging is sequential Gaussian simulation without the sequence: the reference writes out_grid[i, j] = est and never sets
// cond_msk[i, j], and neighbors takes cells of cond_msk only, so every cell conditions on the measured values alone.  One
// wavefront per cell, all side by side: the ring search with its radius widening (a cell qualifies when the grid holds a
// value there), then the kriging system and its Gauss-Jordan solve -- both sgs_search.h's, shared with the SGS kernels --,
// and, the neighbours' values being known, the estimate and the variance in the same kernel.  No records, no value pass,
// no segments.
// Equidistant candidates in ascending (distance, row, column), as in the SGS kernels.
// Limits: num_points <= 48, H and W <= 32767 ((row << 16) | column in an int32).
#include "gsm_internal.h"
#include "device_util.h"
#include "sgs_search.h"
#include <math.h>
#include <algorithm>

namespace gsm {

// ---------------------------------------------------------------------------------------------------------------------
// krige_grid_kernel: one 64-lane workgroup per listed cell.  kLocal: a variogram per cell (krige_grid_local_kernel,
// interpolate.py:56-62) -- a.K.local [H*W][6] and a.K.vtype as sgs_search.h's LocalCov takes them, a.K.lag and a.K.sill unused
// ---------------------------------------------------------------------------------------------------------------------
template <bool kLocal>
__device__ __forceinline__ void krige_grid_cell(const KrigeGridArgs& a, SgsSearchLds& L) {
  const int lane = threadIdx.x;
  const int k = a.cell0 + blockIdx.x;
  if (k >= a.n_cells) return;
  const int H = a.K.H, W = a.K.W, HW = H * W;
  const double* __restrict__ g = a.grid;
  // an erroring cell writes NaN / 0; the others still complete
  auto give_up = [&](int32_t flag) {
    if (lane == 0) { atomicOr(a.K.err, flag); a.est[k] = NAN; a.var[k] = NAN; a.n[k] = 0; }
  };
  const int cell = a.cells[k];
  if (cell < 0 || cell >= HW || !isnan(g[cell])) { give_up(kSgsFlagCell); return; }
  const int i0 = cell / W, j0 = cell - i0 * W;
  const int n = octant_ring_search(L, [g, W](int ic, int jc) { return !isnan(g[ic * W + jc]); }, i0, j0, H, W, a.K.xs, a.K.ys, a.K.radius,
                                   a.K.hw, a.K.num_points / 8, lane);
  if (n == 0) { give_up(kSgsFlagNoValue); return; }                            // no value anywhere on the grid: the reference would loop for ever
  const bool lagr = a.K.ktype == 0;
  double w_l, rho_l, sill;
  int my_i, my_j;                                                // the neighbour's (row, column): only the block kernel's record needs it
  if (const int e = krige_solve_at<kLocal, false>(L, a.K, cell, n, i0, j0, lagr, lane, w_l, rho_l, my_i, my_j, sill)) { give_up(e); return; }
  // ---- estimate and variance (_krige.py:38-43, :76-80) ----
  const double v_l = (lane < n) ? g[L.nb_g[lane]] : 0.0;
  const double var = sill - dev::wave64_sum(w_l * rho_l);       // signed: interpolate.py:83 clips at zero afterwards
  const double sw = dev::wave64_sum(w_l);
  const double swv = dev::wave64_sum(w_l * v_l);
  // ordinary: around the local mean of the neighbours; simple: around the global mean of the data
  const double mean = lagr ? dev::wave64_sum(v_l) / (double)n : a.K.gmean[0];
  if (lane == 0) { a.est[k] = swv + (1.0 - sw) * mean; a.var[k] = var; a.n[k] = n; }
}
__global__ __launch_bounds__(64) void krige_grid_kernel(const KrigeGridArgs a) {
  __shared__ SgsSearchLds L;
  krige_grid_cell<false>(a, L);
}
__global__ __launch_bounds__(64) void krige_grid_local_kernel(const KrigeGridArgs a) {
  __shared__ SgsSearchLds L;
  krige_grid_cell<true>(a, L);
}

hipError_t launch_krige_grid(const KrigeGridArgs& a, hipStream_t st) {
  if (!krige_search_ok(a.K) || a.n_cells < 0) return hipErrorInvalidValue;
  constexpr int kCellsPerLaunch = 1 << 24;                       // 2^30 threads per launch
  KrigeGridArgs b = a;
  for (b.cell0 = 0; b.cell0 < a.n_cells; b.cell0 += kCellsPerLaunch) {
    const dim3 cells(std::min(kCellsPerLaunch, a.n_cells - b.cell0));
    if (a.K.local) hipLaunchKernelGGL(krige_grid_local_kernel, cells, dim3(64), 0, st, b);
    else hipLaunchKernelGGL(krige_grid_kernel, cells, dim3(64), 0, st, b);
  }
  return hipGetLastError();
}

}  // namespace gsm
