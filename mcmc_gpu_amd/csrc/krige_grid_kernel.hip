// interpolate.krige on gfx950: the kriging estimate and its variance at every listed cell of a grid, in normal-score space.
//
// Replaces:
//   krige                     gstatsMCMC/gstatsim_custom/interpolate.py:13-89 (cell loop :46-81, radius widening :65-71)
//   neighbors (octant search) gstatsMCMC/gstatsim_custom/neighbors.py:4-64
//   ok_solve / sk_solve       gstatsMCMC/gstatsim_custom/_krige.py:5-81
//
// Kriging is sequential Gaussian simulation without the sequence: the reference writes out_grid[i, j] = est and never sets
// cond_msk[i, j], and neighbors takes cells of cond_msk only, so every cell conditions on the measured values alone.  One
// wavefront per cell, all side by side: the ring search of sgs_grid_weights_kernel (a cell qualifies when the grid holds a
// value there), the radius widening, the kriging system and the Gauss-Jordan solve (sgs_search.h), and -- the neighbours'
// values being known -- the estimate and the variance in the same kernel.  No records, no value pass, no segments.
// Equidistant candidates in ascending (distance, row, column), as in the SGS kernels.
// Limits: num_points <= 48, H and W <= 32767 ((row << 16) | column in an int32).
#include "gsm_internal.h"
#include "device_util.h"
#include "sgs_search.h"
#include <math.h>
#include <algorithm>

namespace gsm {

// The octant search around cell (i0, j0) with the reference's radius widening: the num_points / 8 nearest cells of every 45-degree
// sector that `qualifies` (flat cell index -> bool) within the radius and the +-hw-cell window, widened by 100 km until a search
// finds something or covers the grid.  All 64 lanes call it; returns the number of neighbours, their flat indices in L.nb_g
// (sector by sector, ascending (distance, cell)).  sgs_grid_weights_kernel's search, with the predicate as the parameter.
template <class Qualifies>
__device__ __forceinline__ int octant_ring_search(SgsSearchLds& L, const Qualifies qualifies, int i0, int j0, int H, int W,
                                                  const double* __restrict__ xs, const double* __restrict__ ys, double radius, int hw,
                                                  int k8, int lane) {
  const double x0 = xs[j0], y0 = ys[i0];
  const double sx = xs[1] - xs[0], sy = ys[1] - ys[0];
  const double adx = fabs(sx), ady = fabs(sy), dmin = fmin(adx, ady);
  const double inv_cert = 1.0 / (dmin * (1.0 - 1e-6));
  const double fac_x = fmin(1.0, ady / adx), fac_y = fmin(1.0, adx / ady);
  int n = 0;
  for (;;) {                                                     // radius widening (interpolate.py:65-71): usually one trip
    const int ilo = max(0, i0 - hw), ihi = min(H - 1, i0 + hw), jlo = max(0, j0 - hw), jhi = min(W - 1, j0 + hw);
    const int e_up = i0 - ilo, e_dn = ihi - i0, e_lf = j0 - jlo, e_rt = jhi - j0;
    const int r_max = max(max(e_up, e_dn), max(e_lf, e_rt));
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
    unsigned done_mask = 0;
    int R = 0;
    bool long_list = false;
    auto probe = [&](int di, int dj, bool ok) {
      const int i = i0 + di, j = j0 + dj;
      ok = ok && i >= ilo && i <= ihi && j >= jlo && j <= jhi;
      const int ic = min(max(i, ilo), ihi), jc = min(max(j, jlo), jhi);
      const bool has = qualifies(ic * W + jc);
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
      if (__ballot(long_list)) {
        for (int s = 0; s < 8; ++s)
          if (L.len[s] > kSgsListCap - 64) sgs_prune_sector(L, s, k8, lane);
        long_list = false;
      }
    };
    while (R < r_max && done_mask != 0xFFu) {
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
        int rr = 0;
        for (int q = 0; q < my_len; ++q) {
          const double dq = L.list_d[my_s][q];
          const int gq = L.list_g[my_s][q];
          rr += (dq < d || (dq == d && gq < gg)) ? 1 : 0;
        }
        if (rr < k8) L.nb_g[my_base + rr] = gg;
      }
      n = tot;
    }
    __syncthreads();
    if (n > 0) break;
    if (ilo == 0 && jlo == 0 && ihi == H - 1 && jhi == W - 1 &&
        radius * radius > ((double)(W - 1) * adx) * ((double)(W - 1) * adx) + ((double)(H - 1) * ady) * ((double)(H - 1) * ady)) break;
    radius += 100e3;
    hw = (int)fmin(ceil(radius / adx), 1.0e6);
  }
  return n;
}

// ---------------------------------------------------------------------------------------------------------------------
// krige_grid_kernel: one 64-lane workgroup per listed cell
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void krige_grid_kernel(const KrigeGridArgs a) {
  __shared__ SgsSearchLds L;
  const int lane = threadIdx.x;
  const int k = a.cell0 + blockIdx.x;
  if (k >= a.n_cells) return;
  const int H = a.H, W = a.W, HW = H * W;
  const double* __restrict__ g = a.grid;
  // an erroring cell writes NaN / 0; the others still complete
  auto give_up = [&](int32_t flag) {
    if (lane == 0) { atomicOr(a.err, flag); a.est[k] = NAN; a.var[k] = NAN; a.n[k] = 0; }
  };
  const int cell = a.cells[k];
  if (cell < 0 || cell >= HW || !isnan(g[cell])) { give_up(2); return; }
  const int i0 = cell / W, j0 = cell - i0 * W;
  const int n = octant_ring_search(L, [g](int c) { return !isnan(g[c]); }, i0, j0, H, W, a.xs, a.ys, a.radius, a.hw,
                                   a.num_points / 8, lane);
  if (n == 0) { give_up(4); return; }                            // no value anywhere on the grid: the reference would loop for ever
  if (lane < n) { const int gg = L.nb_g[lane]; const int rr = gg / W; L.nb_rc[lane] = (rr << 16) | (gg - rr * W); }
  __syncthreads();
  // ---- kriging system, one row per lane (sgs_grid_weights_kernel's) ----
  const bool lagr = a.ktype == 0;
  const int mi = a.mi, mj = a.mj, lag_w = 2 * mj + 1;
  const double* __restrict__ lag = a.lag;
  double rw[50];
  const int my_rc = (lane < n) ? L.nb_rc[lane] : 0;
  const int my_i = my_rc >> 16, my_j = my_rc & 0xFFFF;
  bool lag_ok = true;
#pragma unroll
  for (int j = 0; j < 48; ++j) {
    double v = 0.0;
    if (j < n) {
      if (lane < n) {
        const int rc = L.nb_rc[j];
        const int di = my_i - (rc >> 16), dj = my_j - (rc & 0xFFFF);
        if (abs(di) > mi || abs(dj) > mj) lag_ok = false; else v = lag[(di + mi) * lag_w + dj + mj];
      } else if (lane == 48 && lagr) v = 1.0;
    }
    rw[j] = v;
  }
  {
    double v48 = 0.0, v49 = 0.0;
    if (lane < n) {
      const int di = my_i - i0, dj = my_j - j0;
      v48 = lagr ? 1.0 : 0.0;
      if (abs(di) > mi || abs(dj) > mj) lag_ok = false; else v49 = lag[(di + mi) * lag_w + dj + mj];
    } else if (lane == 48 && lagr) v49 = 1.0;
    rw[48] = v48; rw[49] = v49;
  }
  if (__ballot(!lag_ok)) { give_up(64); return; }
  const double rho_l = rw[49];
  const double c00 = lag[mi * lag_w + mj];
  const double tol = 2.220446049250313e-16 * (double)(n + 1) * fabs(c00), tol_l = 2.220446049250313e-16 * (double)(n + 1) / fabs(c00);
  double mypiv = 1.0;
  bool singular = false;
  GjStep<0>::run(rw, lane, n, lagr, tol, tol_l, mypiv, singular);
  if (singular) { give_up(8); return; }
  // ---- estimate and variance (_krige.py:38-43, :76-80) ----
  const double w_l = (lane < n) ? rw[49] / mypiv : 0.0;
  const double v_l = (lane < n) ? g[L.nb_g[lane]] : 0.0;
  const double var = a.sill - dev::wave64_sum(w_l * rho_l);     // signed: interpolate.py:83 clips at zero afterwards
  const double sw = dev::wave64_sum(w_l);
  const double swv = dev::wave64_sum(w_l * v_l);
  // ordinary: around the local mean of the neighbours; simple: around the global mean of the data
  const double mean = lagr ? dev::wave64_sum(v_l) / (double)n : a.gmean[0];
  if (lane == 0) { a.est[k] = swv + (1.0 - sw) * mean; a.var[k] = var; a.n[k] = n; }
}

hipError_t launch_krige_grid(const KrigeGridArgs& a, hipStream_t st) {
  if (a.hw < 1 || a.num_points < 8 || a.num_points > kSgsMaxPts || a.H < 2 || a.W < 2 || a.H > 32767 || a.W > 32767 || a.n_cells < 0)
    return hipErrorInvalidValue;
  constexpr int kCellsPerLaunch = 1 << 24;                       // 2^30 threads per launch
  KrigeGridArgs b = a;
  for (b.cell0 = 0; b.cell0 < a.n_cells; b.cell0 += kCellsPerLaunch)
    hipLaunchKernelGGL(krige_grid_kernel, dim3(std::min(kCellsPerLaunch, a.n_cells - b.cell0)), dim3(64), 0, st, b);
  return hipGetLastError();
}

}  // namespace gsm
