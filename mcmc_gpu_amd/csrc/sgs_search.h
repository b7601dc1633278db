// The per-cell work that the block SGS kernel (sgs_kernel.hip), the whole-grid SGS kernel (sgs_grid_kernel.hip) and the kriging
// kernel (krige_grid_kernel.hip) share, one wavefront per cell: the octant ring search with the reference's radius widening
// (octant_ring_search; a kernel says which cells qualify) and the kriging system with its Gauss-Jordan solve in registers
// (krige_solve), its covariances from the lag table of the call's one variogram (LagTableCov) or evaluated from the variogram of
// the cell that is solved (LocalCov: the whole-grid kernels' non-stationary form).  sgs_kernel.hip's header comment describes the
// search and the solve.
#pragma once
#include "gsm_internal.h"
#include "device_util.h"
#include <math.h>

namespace gsm {

// candidates kept per sector between prunings (a scan pass appends at most 64; a list is pruned to its k8 nearest when it holds more than
// kSgsListCap - 64 = 16).  The search structure's LDS bounds the kernel's occupancy: 128 -> 80 entries, 64 rings of 16-bit certification
// counters instead of 128 of 32 bits took it from 17 KiB to 9.7 KiB per workgroup = 9 -> 16 wavefronts per CU (the register budget's
// four per SIMD): +14 % per iteration at 256 chains, the extra prunings included (same-box A/B of 128 / 112 / 96 / 88 / 80 entries)
constexpr int kSgsListCap = 80;
constexpr int kSgsCertMax = 64;           // rings with certification counters (the driver's 30 km at 500 m = 60 rings); beyond, a sector
                                          // completes by exhaustion only

// sector b + 4 in 0..7 of atan2(dy, dx) in (b pi/4, (b+1) pi/4]
__device__ __forceinline__ int octant(double dy, double dx) {
  // the same case analysis as selects (no divergent branches in the search pass):
  //   dy == 0: angle pi -> b = 3 (sector 7), angle 0 -> b = -1 (sector 3)
  //   dy > 0:  dx > 0: (0, pi/4] 4 | (pi/4, pi/2) 5;   dx == 0: 5;   dx < 0: (pi/2, 3pi/4] 6 | (3pi/4, pi) 7
  //   dy < 0:  dx > 0: (-pi/4, 0) 3 | (-pi/2, -pi/4] 2;  dx == 0: 1 (-pi/2 -> (-3pi/4, -pi/2]);  dx < 0: (-3pi/4, -pi/2) 1 | (-pi, -3pi/4] 0
  const double ay = fabs(dy), ax = fabs(dx);
  const bool right = dx > 0.0, xz = dx == 0.0;
  const int s_up = right ? ((ay <= ax) ? 4 : 5) : (xz ? 5 : ((ay >= ax) ? 6 : 7));
  const int s_dn = right ? ((ay < ax) ? 3 : 2) : (xz ? 1 : ((ay > ax) ? 1 : 0));
  return (dy == 0.0) ? ((dx < 0.0) ? 7 : 3) : ((dy > 0.0) ? s_up : s_dn);
}

struct SgsSearchLds {
  double list_d[8][kSgsListCap];
  int32_t list_g[8][kSgsListCap];
  int32_t len[8];
  int32_t cum[8];
  uint32_t cert[8][kSgsCertMax / 2];      // candidates of a sector by certification ring: 16-bit counters, two per word (a ring holds
                                          // at most 8 x 127 cells).  The kernel's occupancy is bounded by this structure's size.
  int32_t nb_g[kSgsMaxPts];
  int32_t nb_rc[kSgsMaxPts];            // (row << 16) | col
  double tmp_d[kSgsMaxPts];
  int32_t tmp_g[kSgsMaxPts];
};

// keeps the `keep` smallest (distance, cell) of sector s, in ascending order, at the head of its list; all lanes call it
__device__ __forceinline__ void sgs_prune_sector(SgsSearchLds& L, int s, int keep, int lane) {
  const int len = L.len[s];
  __syncthreads();
  for (int e = lane; e < len; e += 64) {
    const double d = L.list_d[s][e];
    const int g = L.list_g[s][e];
    int r = 0;
    for (int q = 0; q < len; ++q) {
      const double dq = L.list_d[s][q];
      const int gq = L.list_g[s][q];
      r += (dq < d || (dq == d && gq < g)) ? 1 : 0;
    }
    if (r < keep) { L.tmp_d[r] = d; L.tmp_g[r] = g; }
  }
  __syncthreads();
  const int n = min(len, keep);
  if (lane < n) { L.list_d[s][lane] = L.tmp_d[lane]; L.list_g[s][lane] = L.tmp_g[lane]; }
  if (lane == 0) L.len[s] = n;
  __syncthreads();
}

// cell `p` (0 <= p < R) of arc `g` (0..7) of the square ring of Chebyshev radius R around a cell, as (row, column) offsets: the ring's
// 8 R cells in the order top row left to right, right column downwards, bottom row right to left, left column upwards; each side
// is two arcs of R cells, the first starting at a corner (p = 0), the second at the cell on the axis
__device__ __forceinline__ void ring_cell(int R, int g, int p, int& di, int& dj) {
  const int side = g >> 1, e = ((g & 1) ? 0 : -R) + p;
  di = (side == 0) ? -R : (side == 2) ? R : (side == 1) ? e : -e;
  dj = (side == 1) ? R : (side == 3) ? -R : (side == 0) ? e : -e;
}

// The octant search around cell (i0, j0) with the reference's radius widening: the k8 nearest cells of every 45-degree sector that
// `qualifies` ((row, column) -> bool, always called at indices inside the grid) within the radius and the +-hw-cell window, widened
// by 100 km until a search finds something or covers the grid.  All 64 lanes call it; it returns the number of neighbours and leaves
// their flat indices in L.nb_g (sector by sector, ascending (distance, cell)).
template <class Qualifies>
__device__ __forceinline__ int octant_ring_search(SgsSearchLds& L, const Qualifies qualifies, int i0, int j0, int H, int W,
                                                  const double* __restrict__ xs, const double* __restrict__ ys, double radius, int hw,
                                                  int k8, int lane) {
  const double x0 = xs[j0], y0 = ys[i0];
  const double sx = xs[1] - xs[0], sy = ys[1] - ys[0];
  const double adx = fabs(sx), ady = fabs(sy), dmin = fmin(adx, ady);
  const double inv_cert = 1.0 / (dmin * (1.0 - 1e-6));          // certification ring of a distance: floor(d * inv_cert)
  const double fac_x = fmin(1.0, ady / adx), fac_y = fmin(1.0, adx / ady);
  int n = 0;
  for (;;) {                                                     // radius widening (MCMC.py:150-156, interpolate.py:65-71, :150-157): usually one trip
    const int ilo = max(0, i0 - hw), ihi = min(H - 1, i0 + hw), jlo = max(0, j0 - hw), jhi = min(W - 1, j0 + hw);
    // cells towards smaller / larger row and column that the window holds
    const int e_up = i0 - ilo, e_dn = ihi - i0, e_lf = j0 - jlo, e_rt = jhi - j0;
    const int r_max = max(max(e_up, e_dn), max(e_lf, e_rt));
    // sector s: extent (in cells) along its primary axis on its side.  dy = y0 - y > 0 <=> rows with smaller y.
    const int e_ypos = (sy > 0.0) ? e_up : e_dn, e_yneg = (sy > 0.0) ? e_dn : e_up;
    const int e_xpos = (sx > 0.0) ? e_lf : e_rt, e_xneg = (sx > 0.0) ? e_rt : e_lf;
    for (int q = lane; q < 8 * kSgsCertMax / 2; q += 64) (&L.cert[0][0])[q] = 0u;
    if (lane < 8) { L.len[lane] = 0; L.cum[lane] = 0; }
    __syncthreads();
    int my_ext = 0;
    double my_fac = 1.0;
    if (lane < 8) {
      const bool xprim = (lane == 3 || lane == 4 || lane == 7 || lane == 0);
      my_fac = xprim ? fac_x : fac_y;
      my_ext = (lane == 3 || lane == 4) ? e_xpos : (lane == 7 || lane == 0) ? e_xneg : (lane == 5 || lane == 6) ? e_ypos : e_yneg;
    }
    unsigned done_mask = 0;                                      // wave-uniform: sectors complete or exhausted
    int R = 0;
    bool long_list = false;
    // one candidate cell per lane: everything is computed for every lane at clamped (always valid) indices; ONE predicate guards the insertion
    auto probe = [&](int di, int dj, bool ok) {
      const int i = i0 + di, j = j0 + dj;
      ok = ok && i >= ilo && i <= ihi && j >= jlo && j <= jhi;
      const int ic = min(max(i, ilo), ihi), jc = min(max(j, jlo), jhi);
      const bool has = qualifies(ic, jc);
      const double ddx = x0 - xs[jc], ddy = y0 - ys[ic];
      const double d = sqrt(ddx * ddx + ddy * ddy);
      const int s = octant(ddy, ddx);
      const bool ins = ok && has && d < radius && !((done_mask >> s) & 1u);
      if (ins) {
        const int pos = atomicAdd(&L.len[s], 1);
        long_list |= pos + 1 > kSgsListCap - 64;
        L.list_d[s][pos] = d; L.list_g[s][pos] = i * W + j;
        const double qf = d * inv_cert;
        if (qf < (double)kSgsCertMax) { const int qi = (int)qf; atomicAdd(&L.cert[s][qi >> 1], 1u << (16 * (qi & 1))); }
      }
      __syncthreads();
      // a list that could not take another full pass is cut back to the k8 nearest (nothing beyond them can be selected); the lane
      // whose insertion took a list over that mark knows: the eight lengths are only looked at then
      if (__ballot(long_list)) {
        for (int s = 0; s < 8; ++s)
          if (L.len[s] > kSgsListCap - 64) sgs_prune_sector(L, s, k8, lane);
        long_list = false;
      }
    };
    while (R < r_max && done_mask != 0xFFu) {
      // one pass = rings R+1 .. R_hi: the 7 x 7 window first (rings 1-3 = 48 cells), then ring by ring
      const int R_lo = R + 1;
      int R_hi;
      if (R == 0) {
        R_hi = min(3, r_max);
        const int side_w = 2 * R_hi + 1, cells_in_pass = side_w * side_w;
        for (int t0 = 0; t0 < cells_in_pass; t0 += 64) {
          const int t = t0 + lane;
          const int di = t / side_w - R_hi, dj = t % side_w - R_hi;
          probe(di, dj, t < cells_in_pass && !(di == 0 && dj == 0));
        }
      } else {
        R_hi = R_lo;
        const int cells_in_pass = 8 * R_hi;
        const float inv_side = 1.0f / (float)(2 * R_hi);
        for (int t0 = 0; t0 < cells_in_pass; t0 += 64) {
          const int t = t0 + lane;
          // t / (2 R_hi) without an integer division: (t + 1/2) / (2 R_hi) is at least 1 / (4 R_hi) away from an integer, fp32 is exact enough
          const int side = (int)(((float)t + 0.5f) * inv_side), o = t - side * 2 * R_hi;
          int di, dj;
          ring_cell(R_hi, 2 * side + (o >= R_hi ? 1 : 0), o >= R_hi ? o - R_hi : o, di, dj);
          probe(di, dj, t < cells_in_pass);
        }
      }
      R = R_hi;
      bool fin = false;
      if (lane < 8) {
        int c = L.cum[lane];
        for (int q = R_lo; q <= R && q < kSgsCertMax; ++q) c += (int)((L.cert[lane][q >> 1] >> (16 * (q & 1))) & 0xFFFFu);
        L.cum[lane] = c;
        fin = c >= k8 || (double)my_ext <= floor((double)R * my_fac + 1e-6);
      }
      done_mask |= (unsigned)(__ballot(fin) & 0xFFull);
      __syncthreads();
    }
    // selection: per sector the k8 nearest in ascending (distance, cell); sectors concatenated in angle order
    // all eight sectors at once, eight lanes each (a sector's list rarely holds more than a few dozen candidates: one sector after
    // the other left most lanes idle): lane = 8 * sector + e mod 8 ranks its candidates against the whole list of its sector
    {
      const int my_s = lane >> 3;
      int tot = 0, my_base = 0, my_len = 0;
      for (int s = 0; s < 8; ++s) {
        const int len = L.len[s];
        if (s == my_s) { my_base = tot; my_len = len; }
        tot += min(len, k8);
      }
      for (int e = lane & 7; e < my_len; e += 8) {
        const double d = L.list_d[my_s][e];
        const int gg = L.list_g[my_s][e];
        int r = 0;
        for (int q = 0; q < my_len; ++q) {
          const double dq = L.list_d[my_s][q];
          const int gq = L.list_g[my_s][q];
          r += (dq < d || (dq == d && gq < gg)) ? 1 : 0;
        }
        if (r < k8) L.nb_g[my_base + r] = gg;
      }
      n = tot;
    }
    __syncthreads();
    if (n > 0) break;
    // nothing within the radius: the reference adds 100 km and rebuilds the stencil (window = ceil(radius / |dx|) cells)
    if (ilo == 0 && jlo == 0 && ihi == H - 1 && jhi == W - 1 &&
        radius * radius > ((double)(W - 1) * adx) * ((double)(W - 1) * adx) + ((double)(H - 1) * ady) * ((double)(H - 1) * ady)) break;
    radius += 100e3;
    hw = (int)fmin(ceil(radius / adx), 1.0e6);
  }
  return n;
}

template <int K>
struct GjStep {
  // one Gauss-Jordan step on pivot K: r[] is this lane's row of [A | b] (columns 0..47 neighbours, 48 the Lagrange column,
  // 49 the right-hand side)
  static __device__ __forceinline__ void run(double (&r)[50], int lane, int n, bool lagr, double tol, double tol_l, double& mypiv, bool& singular) {
    if (K < n || (K == 48 && lagr)) {                            // wave-uniform: rows n..47 do not exist; no Lagrange row in simple kriging
      const double pv = dev::readlane_f64(r[K], K);
      if (!(fabs(pv) > (K == 48 ? tol_l : tol))) singular = true;
      // 1 / pivot: hardware estimate + two Newton steps (every lane computes the same value), then the fma-corrected quotient
      double rp = __builtin_amdgcn_rcp(pv);
      rp = __fma_rn(__fma_rn(-pv, rp, 1.0), rp, rp);
      rp = __fma_rn(__fma_rn(-pv, rp, 1.0), rp, rp);
      double f = dev::exact_div(r[K], pv, rp);
      if (lane == K) { f = 0.0; mypiv = pv; }
#pragma unroll
      for (int j = K + 1; j < 50; ++j) r[j] = __fma_rn(-f, dev::readlane_f64(r[j], K), r[j]);
    }
    GjStep<K + 1>::run(r, lane, n, lagr, tol, tol_l, mypiv, singular);
  }
};
template <>
struct GjStep<49> {
  static __device__ __forceinline__ void run(double (&)[50], int, int, bool, double, double, double&, bool&) {}
};

// ---- where krige_solve takes its covariances from -------------------------------------------------------------------------------
// One variogram for the whole call: `lag`, (2 mi + 1) x (2 mj + 1) covariances indexed by the integer lag between two cells.
// kWholeGridTable compiles the row loads of a table that spans every lag of the grid.
template <bool kWholeGridTable>
struct LagTableCov {
  static constexpr bool kLocal = false, kWholeGrid = kWholeGridTable;
  const double* __restrict__ lag;
  int mi, mj;
};
// A variogram per cell (the reference's local_vario, interpolate.py:56-62, :141-147): `p` points at the six numbers of the cell
// that is being solved -- R00, R01, R10, R11 of make_rotation_matrix (_krige.py:83-103, computed on the host), sill, nugget --
// and every covariance is evaluated from the two points' coordinates.  vtype: GSM_VTYPE_EXPONENTIAL / _GAUSSIAN / _SPHERICAL.
struct LocalCov {
  static constexpr bool kLocal = true;
  // The row is read through the constant address space (step_common.h does the same with its records): no kernel writes the table and
  // the cell is the wavefront's, so the six numbers are scalar loads into SGPRs.  As a plain pointer out of the kernel's argument
  // struct they are vector loads (the compiler cannot rule out the kernel's own stores): 12 VGPRs, 122 -> 134 in the per-cell kernels.
  typedef const __attribute__((address_space(4))) double* row_t;
  row_t p;
  const double* __restrict__ xs;
  const double* __restrict__ ys;
  int vtype;
};

// covariance.py:4-15 on the squared normalised lag h2 (c0 = sill - nugget), the reference's oddities included: its "nugget" only
// scales the model, and the spherical model is sill - 1 beyond the range.  Not inlined: krige_fill_local calls it from a loop that is
// unrolled 48 times over a row held in registers, and 48 copies of exp's polynomial push that row into scratch.
__device__ __noinline__ double local_cov_of(double h2, double c0, double sill, int vtype) {
  const double h = sqrt(h2);
  if (vtype == 0) return c0 * exp(-3.0 * h);
  if (vtype == 1) return c0 * exp(-3.0 * (h * h));
  const double c = c0 - 1.5 * h + 0.5 * (h * h * h);
  return (h > 1.0) ? sill - 1.0 : c;
}

// This lane's row of [Sigma 1 | rho] (r[0..47], r[48], r[49]) from the cell's own variogram.  A pair's lag is taken from the
// coordinates (either axis may descend, the cells need not be square), rotated and scaled by R: u = dx R00 + dy R10, v = dx R01 + dy R11, h2 = u u + v v.  The reference multiplies
// the absolute coordinates by R and subtracts afterwards (make_sigma / make_rho, _krige.py:105-144); subtracting first loses
// fewer digits.  L.list_d (free once the search is over) carries the neighbours' coordinates.
__device__ __forceinline__ void krige_fill_local(SgsSearchLds& L, const LocalCov& cov, double (&r)[50], int n, int i0, int j0, bool lagr,
                                                 int lane, int my_i, int my_j) {
  const double R00 = cov.p[0], R01 = cov.p[1], R10 = cov.p[2], R11 = cov.p[3], sill = cov.p[4], c0 = cov.p[4] - cov.p[5];
  const double my_x = cov.xs[my_j], my_y = cov.ys[my_i];        // lanes >= n: cell (0, 0), computed and dropped
  if (lane < n) { L.list_d[0][lane] = my_x; L.list_d[1][lane] = my_y; }
  __syncthreads();
  auto pair = [&](double ddx, double ddy) {
    const double u = ddx * R00 + ddy * R10, v = ddx * R01 + ddy * R11;
    return local_cov_of(u * u + v * v, c0, sill, cov.vtype);
  };
#pragma unroll
  for (int j = 0; j < 48; ++j) {
    double v = 0.0;
    if (j < n) {                                                 // wave-uniform
      const double c = pair(my_x - L.list_d[0][j], my_y - L.list_d[1][j]);
      v = (lane < n) ? c : ((lane == 48 && lagr) ? 1.0 : 0.0);
    }
    r[j] = v;
  }
  const double c = pair(my_x - cov.xs[j0], my_y - cov.ys[i0]);
  r[48] = (lane < n && lagr) ? 1.0 : 0.0;
  r[49] = (lane < n) ? c : ((lane == 48 && lagr) ? 1.0 : 0.0);
}

// The kriging system of cell (i0, j0) with the n > 0 neighbours that octant_ring_search left in L.nb_g, one row per lane in
// registers, and its solve: ordinary kriging [Sigma 1; 1' 0] w = [rho; 1] (_krige.py:25-37) or, with lagr false, simple kriging
// Sigma w = rho (_krige.py:66-73: no Lagrange row / column).  The covariances come from `cov`: a LagTableCov or a LocalCov.
// All 64 lanes call it.  Returns 0, kSgsFlagLagTable (a lag beyond the table; never with a LocalCov) or kSgsFlagSingular; with 0, lane < n holds its
// neighbour's weight w_l, its covariance with the cell rho_l and its (row, column) (my_i, my_j); w_l is 0 in the other lanes.
// L.nb_rc is scratch.
template <class Cov>
__device__ __forceinline__ int krige_solve(SgsSearchLds& L, int n, int i0, int j0, int H, int W, const Cov& cov, bool lagr, int lane,
                                           double& w_l, double& rho_l, int& my_i, int& my_j) {
  if (lane < n) { const int gg = L.nb_g[lane]; const int rr = gg / W; L.nb_rc[lane] = (rr << 16) | (gg - rr * W); }
  __syncthreads();
  double r[50];
  double c00;
  if constexpr (Cov::kLocal) {
    const int my_rc = (lane < n) ? L.nb_rc[lane] : 0;
    my_i = my_rc >> 16; my_j = my_rc & 0xFFFF;
    krige_fill_local(L, cov, r, n, i0, j0, lagr, lane, my_i, my_j);
    rho_l = r[49];
    c00 = cov.p[4] - cov.p[5];
  } else {
    constexpr bool kWholeGridTable = Cov::kWholeGrid;
    const double* __restrict__ lag = cov.lag;
    const int mi = cov.mi, mj = cov.mj;
    const int lag_w = 2 * mj + 1;
    const int my_rc = (lane < n) ? L.nb_rc[lane] : 0;
    my_i = my_rc >> 16; my_j = my_rc & 0xFFFF;
    bool lag_ok = true;
    if (kWholeGridTable && mi >= H - 1 && mj >= W - 1) {
      // the table spans every lag of the grid (lag_extents: grids up to 2048 x 2048 lags): no range test, and the index of the pair
      // (this lane's neighbour, neighbour j) is one subtraction -- (my_i + mi) lag_w + my_j + mj minus neighbour j's i lag_w + j
      const int my_base = (my_i + mi) * lag_w + my_j + mj;
      __syncthreads();
      if (lane < n) L.nb_rc[lane] = my_i * lag_w + my_j;           // the (row, col) pairs are in registers by now
      __syncthreads();
#pragma unroll
      for (int j = 0; j < 48; ++j) {
        double v = 0.0;
        if (j < n) {                                               // wave-uniform
          if (lane < n) v = lag[my_base - L.nb_rc[j]];
          else if (lane == 48 && lagr) v = 1.0;
        }
        r[j] = v;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 48; ++j) {
        double v = 0.0;
        if (j < n) {                                               // wave-uniform
          if (lane < n) {
            const int rc = L.nb_rc[j];
            const int di = my_i - (rc >> 16), dj = my_j - (rc & 0xFFFF);
            if (abs(di) > mi || abs(dj) > mj) lag_ok = false; else v = lag[(di + mi) * lag_w + dj + mj];
          } else if (lane == 48 && lagr) v = 1.0;
        }
        r[j] = v;
      }
    }
    {
      double v48 = 0.0, v49 = 0.0;
      if (lane < n) {
        const int di = my_i - i0, dj = my_j - j0;
        v48 = lagr ? 1.0 : 0.0;
        if (abs(di) > mi || abs(dj) > mj) lag_ok = false; else v49 = lag[(di + mi) * lag_w + dj + mj];
      } else if (lane == 48 && lagr) v49 = 1.0;
      r[48] = v48; r[49] = v49;
    }
    if (__ballot(!lag_ok)) return kSgsFlagLagTable;
    rho_l = r[49];
    c00 = lag[mi * lag_w + mj];
  }
  // relative pivot test: eps * N * max|diag| for the covariance pivots (conditional variances), eps * N / max|diag| for the
  // Lagrange pivot -1' Sigma^-1 1
  const double tol = 2.220446049250313e-16 * (double)(n + 1) * fabs(c00), tol_l = 2.220446049250313e-16 * (double)(n + 1) / fabs(c00);
  double mypiv = 1.0;
  bool singular = false;
  GjStep<0>::run(r, lane, n, lagr, tol, tol_l, mypiv, singular);
  if (singular) return kSgsFlagSingular;
  w_l = (lane < n) ? r[49] / mypiv : 0.0;
  return 0;
}
// krige_solve for cell `cell` = (i0, j0) of the call K, what every kernel calls: the covariances from K.local's row of the cell
// (kLocal) or from K's lag table, and in `sill` the sill that the cell's kriging variance is taken from
template <bool kLocal, bool kWholeGridTable>
__device__ __forceinline__ int krige_solve_at(SgsSearchLds& L, const KrigeSearch& K, int cell, int n, int i0, int j0, bool lagr, int lane,
                                              double& w_l, double& rho_l, int& my_i, int& my_j, double& sill) {
  if constexpr (kLocal) {
    const LocalCov cov{(LocalCov::row_t)(K.local + 6 * (size_t)cell), K.xs, K.ys, K.vtype};
    sill = cov.p[4];
    return krige_solve(L, n, i0, j0, K.H, K.W, cov, lagr, lane, w_l, rho_l, my_i, my_j);
  } else {
    sill = K.sill;
    return krige_solve(L, n, i0, j0, K.H, K.W, LagTableCov<kWholeGridTable>{K.lag, K.mi, K.mj}, lagr, lane, w_l, rho_l, my_i, my_j);
  }
}

}  // namespace gsm
