// interpolate.cross_validate on gfx950: every listed DATA cell of a grid kriged from the other data under a hold-out, in
// normal-score space -- leave-one-out, a buffer around the target, folds -- for up to eight candidate variograms at once.
//
// The reference has no cross-validation; this is gstat's krige.cv / GSLIB's jackknife with the reference's kriging:
//   neighbors (octant search) gstatsMCMC/gstatsim_custom/neighbors.py:4-64
//   ok_solve / sk_solve       gstatsMCMC/gstatsim_custom/_krige.py:5-81
//   radius widening           gstatsMCMC/gstatsim_custom/interpolate.py:65-71
//
// krige_grid_kernel.hip with another predicate in the neighbour search and a loop around the solve.  One wavefront per target.
// A candidate cell c conditions target t when it holds a value, is not of t's fold (t in a fold at all) and lies beyond the
// exclusion radius; the search skips t itself.  What a hold-out leaves is what gsm_krige_grid finds on a copy of the grid with
// the held-out cells set to NaN, cell for cell and bit for bit (tests/test_gpu_krige_cv.py) -- but the buffered hold-out has
// another held-out set per target, and leave-one-out as many sets as data, so no grid copy expresses either in one call.
// The neighbour set depends on the geometry and the hold-out only, not on the covariance model: ONE search per target, then
// per model the system, its solve, the estimate and the variance.  octant_ring_search leaves the set in L.nb_g, and
// krige_solve rebuilds everything else it keeps in LDS from that, so the loop needs no LDS of its own.
// Limits: krige_grid_kernel.hip's, and n_models <= kKrigeCvMaxModels.
#include "gsm_internal.h"
#include "device_util.h"
#include "sgs_search.h"
#include <math.h>
#include <algorithm>

namespace gsm {

// ---------------------------------------------------------------------------------------------------------------------
// krige_cv_kernel: one 64-lane workgroup per listed cell.  kLocal: per model a variogram per cell (krige_cv_local_kernel),
// model m's table a.model_stride doubles after model m - 1's, its vtype in a.vtype[m]
// ---------------------------------------------------------------------------------------------------------------------
template <bool kLocal>
__device__ __forceinline__ void krige_cv_cell(const KrigeCvArgs& a, SgsSearchLds& L) {
  const int lane = threadIdx.x;
  const int k = a.cell0 + blockIdx.x;
  if (k >= a.n_cells) return;
  const int H = a.K.H, W = a.K.W, HW = H * W;
  const int M = a.n_models;
  const size_t nc = (size_t)a.n_cells;
  const double* __restrict__ g = a.grid;
  // an erroring cell writes NaN / 0 for every model; the other cells still complete
  auto give_up = [&](int32_t flag) {
    if (lane == 0) {
      atomicOr(a.K.err, flag);
      for (int m = 0; m < M; ++m) { a.est[m * nc + k] = NAN; a.var[m * nc + k] = NAN; }
      a.n[k] = 0;
    }
  };
  const int cell = a.cells[k];
  if (cell < 0 || cell >= HW || isnan(g[cell])) { give_up(kSgsFlagCell); return; }
  const int i0 = cell / W, j0 = cell - i0 * W;
  // ---- the hold-out: fold_t < 0 and ex <= 0 switch their clauses off (leave-one-out: both) ----
  const int32_t* __restrict__ fold = a.fold;
  const int fold_t = fold ? fold[cell] : -1;
  const double ex = a.exclude_radius;
  const double* __restrict__ xs = a.K.xs;
  const double* __restrict__ ys = a.K.ys;
  const double x0 = xs[j0], y0 = ys[i0];
  auto qualifies = [=](int ic, int jc) {
    const int c = ic * W + jc;
    bool ok = !isnan(g[c]);
    if (fold_t >= 0) ok = ok && fold[c] != fold_t;               // wave-uniform
    if (ex > 0.0) {                                              // wave-uniform; the probe's own expression of the distance
      const double ddx = x0 - xs[jc], ddy = y0 - ys[ic];
      ok = ok && !(sqrt(ddx * ddx + ddy * ddy) <= ex);
    }
    return ok;
  };
  const int n = octant_ring_search(L, qualifies, i0, j0, H, W, xs, ys, a.K.radius, a.K.hw, a.K.num_points / 8, lane);
  if (n == 0) { give_up(kSgsFlagNoValue); return; }              // nothing qualifies anywhere on the grid
  const bool lagr = a.K.ktype == 0;
  if (lane == 0) a.n[k] = n;
#pragma unroll 1
  for (int m = 0; m < M; ++m) {
    KrigeSearch Km = a.K;
    if constexpr (kLocal) { Km.local = a.K.local + (size_t)m * (size_t)a.model_stride; Km.vtype = a.vtype[m]; }
    else { Km.lag = a.K.lag + (size_t)m * (size_t)a.model_stride; Km.sill = a.sill[m]; }
    double w_l, rho_l, sill;
    int my_i, my_j;
    double est = NAN, var = NAN;
    // The neighbour count, opaque to the compiler in every trip.  krige_solve's fill loop is unrolled 48 times over `j < n`, and
    // what a row holds where it loads no covariance (0, or 1 in the Lagrange row) does not depend on the model: with n
    // loop-invariant, LLVM hoists those 48 values out of the model loop into 96 VGPRs that live across it (226 VGPRs against
    // krige_grid_kernel's 116, 2 waves per SIMD against 4).
    int nm = __builtin_amdgcn_readfirstlane(n);
    asm volatile("" : "+s"(nm));
    // a model that fails (a singular system, a lag beyond the table) fails alone
    if (const int e = krige_solve_at<kLocal, false>(L, Km, cell, nm, i0, j0, lagr, lane, w_l, rho_l, my_i, my_j, sill)) {
      if (lane == 0) atomicOr(a.K.err, e);
    } else {
      // ---- estimate and variance (_krige.py:38-43, :76-80), krige_grid_cell's arithmetic ----
      // (the neighbours' values and their mean are the same for every model: read again per trip, a few cached loads and one
      // wave sum beside a solve, they cost no registers across the loop)
      const double v_l = (lane < nm) ? g[L.nb_g[lane]] : 0.0;
      var = sill - dev::wave64_sum(w_l * rho_l);                 // signed
      const double sw = dev::wave64_sum(w_l);
      const double swv = dev::wave64_sum(w_l * v_l);
      // ordinary: around the local mean of the neighbours; simple: around the global mean of ALL data, the target's included
      const double mean = lagr ? dev::wave64_sum(v_l) / (double)nm : a.K.gmean[0];
      est = swv + (1.0 - sw) * mean;
    }
    if (lane == 0) { a.est[m * nc + k] = est; a.var[m * nc + k] = var; }
    __syncthreads();                                             // the next model's solve rewrites L.nb_rc / L.list_d
  }
}
__global__ __launch_bounds__(64) void krige_cv_kernel(const KrigeCvArgs a) {
  __shared__ SgsSearchLds L;
  krige_cv_cell<false>(a, L);
}
__global__ __launch_bounds__(64) void krige_cv_local_kernel(const KrigeCvArgs a) {
  __shared__ SgsSearchLds L;
  krige_cv_cell<true>(a, L);
}

hipError_t launch_krige_cv(const KrigeCvArgs& a, hipStream_t st) {
  if (!krige_search_ok(a.K) || a.n_cells < 0 || a.n_models < 1 || a.n_models > kKrigeCvMaxModels || !(a.exclude_radius >= 0.0))
    return hipErrorInvalidValue;
  constexpr int kCellsPerLaunch = 1 << 24;                       // 2^30 threads per launch
  KrigeCvArgs b = a;
  for (b.cell0 = 0; b.cell0 < a.n_cells; b.cell0 += kCellsPerLaunch) {
    const dim3 cells(std::min(kCellsPerLaunch, a.n_cells - b.cell0));
    if (a.K.local) hipLaunchKernelGGL(krige_cv_local_kernel, cells, dim3(64), 0, st, b);
    else hipLaunchKernelGGL(krige_cv_kernel, cells, dim3(64), 0, st, b);
  }
  return hipGetLastError();
}

}  // namespace gsm
