// interpolate.sgs on gfx950: sequential Gaussian simulation of whole grids, many realisations per call.
//
// Replaces, for a batch of realisations:
//   sgs                       gstatsMCMC/gstatsim_custom/interpolate.py:92-191 (cell loop :132-189, radius widening :150-157,
//                             truncated-normal draw :173-187)
//   neighbors (octant search) gstatsMCMC/gstatsim_custom/neighbors.py:4-64
//   ok_solve / sk_solve       gstatsMCMC/gstatsim_custom/_krige.py:5-81
//
// The random numbers are the caller's (NumPy on the host, in the reference's order): each realisation's visiting order
// (rng.shuffle) and one number per path cell -- a standard normal (rng.normal(est, sd) = est + sd * z) or, with bounds, a
// uniform (truncnorm.rvs = truncnorm.ppf(u, a, b) * scale + est, truncnorm.h).
//
// The block kernels' split (sgs_kernel.hip) carries over: a cell's neighbour set and kriging weights depend only on WHICH
// cells hold a value when it is visited, never on the values.
//   sgs_grid_rank_kernel / sgs_grid_slot_kernel  per realisation the visiting rank of every cell, int32 [R][H*W]: -1 for a
//                        conditioning value, the slot for a path cell, INT32_MAX for a NaN cell that is never filled (outside
//                        sim_mask);
//   sgs_grid_weights_kernel  one wavefront per (realisation, path slot) of a segment, all side by side: the block kernel's ring
//                        search (a cell qualifies when its rank is below the slot), radius widening, kriging system and
//                        Gauss-Jordan solve (sgs_search.h) -> a record per cell.  A neighbour is either a value (conditioning
//                        data, or a path cell whose bounds coincide) or an earlier path cell, NaN-boxed (slot << 25 | cell);
//                        no simulated value is read, so a segment's records do not wait for the values before it;
//   sgs_grid_values_kernel   one workgroup of four waves per realisation walks the segment's slots in 64-cell chunks, as
//                        sgs_sequence_kernel does: the four waves gather each cell's known part (values of earlier chunks come
//                        from the realisation's grid in global memory, written by wave 0 of the same workgroup before the
//                        chunk's barrier); coefficients of cells of the same chunk go to a 64 x 64 LDS tile; wave 0 then
//                        finishes the cells one by one -- cell k's estimate is complete once cells < k are, its draw is
//                        applied (est + sd z, or the truncated-normal ppf evaluated by every lane on lane k's numbers) and
//                        broadcast to the lanes that list it.
// Segments bound the records in memory: the caller picks the slots per segment (a multiple of 64, so that the chunks and
// therefore every rounding are the same whatever the segment size).
// Limits: num_points <= 48, H * W <= 2^25 cells (25-bit slot and cell fields in a record).
#include "gsm_internal.h"
#include "device_util.h"
#include "sgs_search.h"
#include "truncnorm.h"
#include <math.h>

namespace gsm {

constexpr int32_t kGridNever = 0x7fffffff;
constexpr uint64_t kGridPendingTag = 0xFFFC000000000000ull;     // bits 50..63 set: a negative quiet NaN no arithmetic produces
constexpr int kGridFieldBits = 25;
constexpr uint32_t kGridFieldMask = (1u << kGridFieldBits) - 1u;

__device__ __forceinline__ double grid_readlane_f64(double v, int l) {
  const dev::v2i32 b = __builtin_bit_cast(dev::v2i32, v);
  dev::v2i32 o;
  o.x = __builtin_amdgcn_readlane(b.x, l); o.y = __builtin_amdgcn_readlane(b.y, l);
  return __builtin_bit_cast(double, o);
}
// a value written by another wave of this workgroup: read from L2, past this CU's L1
__device__ __forceinline__ double load_l2(const double* p) {
  return __builtin_bit_cast(double, __hip_atomic_load((unsigned long long*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// ---------------------------------------------------------------------------------------------------------------------
// ranks: every cell of every realisation, then the path slots (a path cell must be NaN and listed once)
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sgs_grid_rank_kernel(const SgsGridArgs a) {
  const int r = blockIdx.y;
  const int HW = a.H * a.W;
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= HW) return;
  a.rank[(size_t)r * HW + c] = isnan(a.grid[(size_t)r * HW + c]) ? kGridNever : -1;
}
__global__ __launch_bounds__(256) void sgs_grid_slot_kernel(const SgsGridArgs a) {
  const int r = blockIdx.y;
  const int HW = a.H * a.W;
  const int64_t p0 = a.path_off[r];
  const int cnt = (int)(a.path_off[r + 1] - p0);
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= cnt) return;
  const int cell = a.path[p0 + k];
  if (cell < 0 || cell >= HW) { atomicOr(a.err, 2); return; }
  if (atomicCAS(&a.rank[(size_t)r * HW + cell], kGridNever, k) != kGridNever) atomicOr(a.err, 2);   // not NaN, or listed twice
}

// ---------------------------------------------------------------------------------------------------------------------
// sgs_grid_weights_kernel: one 64-lane workgroup per (slot of the segment, realisation)
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void sgs_grid_weights_kernel(const SgsGridArgs a) {
  __shared__ SgsSearchLds L;
  const int r = blockIdx.y, lane = threadIdx.x;
  const int slot = a.seg0 + blockIdx.x;
  const int64_t p0 = a.path_off[r];
  const int cnt = (int)(a.path_off[r + 1] - p0);
  if (slot >= cnt) return;
  const int H = a.H, W = a.W, HW = H * W;
  const size_t rec = (size_t)r * a.seg_cap + blockIdx.x;
  const int cell = a.path[p0 + slot];
  const int32_t* rank = a.rank + (size_t)r * HW;
  if (cell < 0 || cell >= HW || rank[cell] != slot) {            // flagged by sgs_grid_slot_kernel
    if (lane == 0) { a.rec_hdr[rec].n = -2; a.rec_hdr[rec].cell = 0; }
    return;
  }
  if (a.lo && a.lo[cell] == a.hi[cell]) {                        // interpolate.py:181-182: the lower bound, nothing drawn
    if (lane == 0) { a.rec_hdr[rec].n = -3; a.rec_hdr[rec].cell = cell; }
    return;
  }
  const double* __restrict__ g = a.grid + (size_t)r * HW;
  const int i0 = cell / W, j0 = cell - i0 * W;
  const int k8 = a.num_points / 8;
  const double x0 = a.xs[j0], y0 = a.ys[i0];
  const double sx = a.xs[1] - a.xs[0], sy = a.ys[1] - a.ys[0];
  const double adx = fabs(sx), ady = fabs(sy), dmin = fmin(adx, ady);
  const double inv_cert = 1.0 / (dmin * (1.0 - 1e-6));
  const double fac_x = fmin(1.0, ady / adx), fac_y = fmin(1.0, adx / ady);
  double radius = a.radius;
  int hw = a.hw;
  int n = 0;
  for (;;) {                                                     // radius widening (interpolate.py:150-157): usually one trip
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
      const int rk = rank[ic * W + jc];
      const double ddx = x0 - a.xs[jc], ddy = y0 - a.ys[ic];
      const double d = sqrt(ddx * ddx + ddy * ddy);
      const int s = octant(ddy, ddx);
      // rk: -1 = conditioning data, < slot = filled before this cell
      const bool ins = ok && rk < slot && d < radius && !((done_mask >> s) & 1u);
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
  if (n == 0) {                                                  // no value anywhere on the grid: the reference would loop forever
    if (lane == 0) { atomicOr(a.err, 4); a.rec_hdr[rec].n = 0; a.rec_hdr[rec].cell = cell; }
    return;
  }
  if (lane < n) { const int gg = L.nb_g[lane]; const int rr = gg / W; L.nb_rc[lane] = (rr << 16) | (gg - rr * W); }
  __syncthreads();
  // ---- kriging system, one row per lane (sgs_weights_kernel's) ----
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
  if (__ballot(!lag_ok)) { if (lane == 0) { atomicOr(a.err, 64); a.rec_hdr[rec].n = 0; a.rec_hdr[rec].cell = cell; } return; }
  const double rho_l = rw[49];
  const double c00 = lag[mi * lag_w + mj];
  const double tol = 2.220446049250313e-16 * (double)(n + 1) * fabs(c00), tol_l = 2.220446049250313e-16 * (double)(n + 1) / fabs(c00);
  double mypiv = 1.0;
  bool singular = false;
  GjStep<0>::run(rw, lane, n, lagr, tol, tol_l, mypiv, singular);
  if (singular) {
    if (lane == 0) { atomicOr(a.err, 8); a.rec_hdr[rec].n = 0; a.rec_hdr[rec].cell = cell; }
    return;
  }
  const double w_l = (lane < n) ? rw[49] / mypiv : 0.0;
  double var = a.sill - dev::wave64_sum(w_l * rho_l);
  var = fabs(var);                                               // interpolate.py:168
  const double sw = dev::wave64_sum(w_l);
  if (lane < kSgsMaxPts) {
    double2 vw = make_double2(0.0, 0.0);
    if (lane < n) {
      const int gg = L.nb_g[lane];
      vw.y = w_l;
      const int rk = rank[gg];
      if (rk < 0) vw.x = g[gg];                                   // conditioning value
      else if (a.lo && a.lo[gg] == a.hi[gg]) vw.x = a.lo[gg];     // a path cell whose value is its bound
      else vw.x = __builtin_bit_cast(double, kGridPendingTag | ((uint64_t)(uint32_t)rk << kGridFieldBits) | (uint64_t)(uint32_t)gg);
    }
    a.rec_vw[((rec >> 6) * kSgsMaxPts + lane) * 64 + (rec & 63)] = vw;
  }
  if (lane == 0) {
    SgsGridHdr hd;
    hd.n = n; hd.cell = cell; hd.sd = sqrt(var); hd.var = var;
    hd.c1 = lagr ? (1.0 - sw) / (double)n : a.gmean[r] * (1.0 - sw);
    a.rec_hdr[rec] = hd;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// sgs_grid_values_kernel: one workgroup of four waves per realisation, the segment's slots 64 at a time
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kGridSeqWaves = 4;
// the bounded draw of interpolate.py:183-187 for one cell: truncnorm.rvs(a, b, loc=est, scale=sd) = ppf(u, a, b) * sd + est;
// scale == 0 (scipy returns est without drawing) and a >= b (scipy raises) are domain errors
__device__ __noinline__ double grid_truncnorm_draw(double est, double sd, double lo, double hi, double u, int32_t* err) {
  if (!(sd > 0.0)) { atomicOr(err, 128); return NAN; }
  const double ta = (lo - est) / sd, tb = (hi - est) / sd;
  if (!(ta < tb)) { atomicOr(err, 128); return NAN; }
  return tn::ppf(u, ta, tb) * sd + est;
}

__global__ __launch_bounds__(64 * kGridSeqWaves) void sgs_grid_values_kernel(const SgsGridArgs a) {
  __shared__ double tile[64 * 64];                               // [chunk cell the value comes from][lane = cell that uses it]
  __shared__ double2 part[kGridSeqWaves][64];                    // per wave and cell: (sum v, sum w v) over the wave's entries
  __shared__ uint64_t mpart[kGridSeqWaves][64];
  const int r = blockIdx.x, lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int HW = a.H * a.W;
  double* __restrict__ g = a.grid + (size_t)r * HW;
  const int64_t p0 = a.path_off[r];
  const int k_end = min((int)(a.path_off[r + 1] - p0), a.seg0 + a.seg_len);
  const bool ok_k = a.ktype == 0, bounded = a.draw_kind == 1;
  for (int kc = a.seg0; kc < k_end; kc += 64) {
    __syncthreads();                                             // wave 0's values of the chunks before have been stored
    const int j = kc + lane;
    const size_t rec = (size_t)r * a.seg_cap + (size_t)(kc - a.seg0) + lane;
    SgsGridHdr hd;
    hd.n = -4; hd.cell = 0; hd.sd = 0.0; hd.var = 0.0; hd.c1 = 0.0;
    if (j < k_end) hd = a.rec_hdr[rec];
    const int n = hd.n;
    const double2* __restrict__ vw = a.rec_vw + (((size_t)r * a.seg_cap + (size_t)(kc - a.seg0)) >> 6) * kSgsMaxPts * 64;
    // ---- gather: entries wave, wave + 4, ... of every cell's list ----
    double sv = 0.0, swv = 0.0;
    uint64_t mask = 0;
    for (int e = wave; e < kSgsMaxPts; e += kGridSeqWaves) {
      if (e < n) {
        const double2 rr = vw[e * 64 + lane];
        const uint64_t bits = __builtin_bit_cast(uint64_t, rr.x);
        if ((bits >> 50) == (kGridPendingTag >> 50)) {
          const int s = (int)((bits >> kGridFieldBits) & kGridFieldMask), c = (int)(bits & kGridFieldMask);
          if (s < kc) {                                          // an earlier chunk: final, in the grid
            const double v = load_l2(g + (c < HW ? c : 0));
            sv += v; swv += rr.y * v;
          } else if (s - kc < 64) {                              // this chunk (s < j): through the tile
            tile[(s - kc) * 64 + lane] = ok_k ? rr.y + hd.c1 : rr.y;
            mask |= 1ull << (s - kc);
          }
        } else {
          sv += rr.x; swv += rr.y * rr.x;
        }
      }
    }
    part[wave][lane] = make_double2(sv, swv);
    mpart[wave][lane] = mask;
    __syncthreads();
    if (wave != 0) continue;
    // ---- sequence (wave 0) ----
    sv = 0.0; swv = 0.0; mask = 0;
#pragma unroll
    for (int w = 0; w < kGridSeqWaves; ++w) { const double2 q = part[w][lane]; sv += q.x; swv += q.y; mask |= mpart[w][lane]; }
    // est = sum w v + sum v (1 - sum w) / n (ordinary, _krige.py:42) or sum w v + global mean (1 - sum w) (simple, :79)
    double est = (n > 0) ? swv + (ok_k ? sv * hd.c1 : hd.c1) : 0.0;
    const double dr = (n > 0) ? a.draw[p0 + j] : 0.0;
    double lo_c = 0.0, hi_c = 0.0;
    if (bounded && (n > 0 || n == -3)) { lo_c = a.lo[hd.cell]; hi_c = a.hi[hd.cell]; }
    double fin = 0.0;
    const int kend = min(64, k_end - kc);
    double t_next = tile[lane];
    for (int k = 0; k < kend; ++k) {
      const double t = t_next;
      if (k + 1 < kend) t_next = tile[(k + 1) * 64 + lane];
      const int nk = __builtin_amdgcn_readlane(n, k);
      double vk = 0.0;
      if (nk > 0) {                                              // cell k's estimate is complete: every cell it lists came before
        const double ek = grid_readlane_f64(est, k), sk = grid_readlane_f64(hd.sd, k), dk = grid_readlane_f64(dr, k);
        if (bounded) vk = grid_truncnorm_draw(ek, sk, grid_readlane_f64(lo_c, k), grid_readlane_f64(hi_c, k), dk, a.err);
        else vk = ek + sk * dk;                                  // rng.normal(est, sqrt(var), 1), interpolate.py:174
      } else if (nk == -3) {
        vk = grid_readlane_f64(lo_c, k);
      } else if (nk == 0) {
        vk = NAN;                                                // error flagged by the weights pass
      }
      if (lane == k) fin = vk;
      if ((mask >> k) & 1ull) est = __fma_rn(t, vk, est);
    }
    if (j < k_end && (n > 0 || n == -3 || n == 0)) g[hd.cell] = fin;
    if (a.trace && j < k_end) {
      double* tr = a.trace + 3 * (p0 + j);
      tr[0] = (n > 0) ? (double)n : -1.0; tr[1] = (n > 0) ? est : fin; tr[2] = (n > 0) ? hd.var : 0.0;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // the stores have reached L2 before the next chunk's barrier
  }
}

static bool grid_args_ok(const SgsGridArgs& a) {
  return !(a.hw < 1 || a.num_points < 8 || a.num_points > kSgsMaxPts || a.H < 2 || a.W < 2 || a.H > 32767 || a.W > 32767 ||
           (int64_t)a.H * a.W > (int64_t)kGridFieldMask + 1 || a.n_real < 1 || a.n_real > 65535 || a.seg_cap % 64 != 0 ||
           a.seg_len < 1 || a.seg_len > a.seg_cap);
}
hipError_t launch_sgs_grid_ranks(const SgsGridArgs& a, int max_path, hipStream_t st) {
  if (!grid_args_ok(a)) return hipErrorInvalidValue;
  const int HW = a.H * a.W;
  hipLaunchKernelGGL(sgs_grid_rank_kernel, dim3((HW + 255) / 256, a.n_real), dim3(256), 0, st, a);
  if (max_path > 0) hipLaunchKernelGGL(sgs_grid_slot_kernel, dim3((max_path + 255) / 256, a.n_real), dim3(256), 0, st, a);
  return hipGetLastError();
}
hipError_t launch_sgs_grid_segment(const SgsGridArgs& a, hipStream_t st) {
  if (!grid_args_ok(a)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sgs_grid_weights_kernel, dim3(a.seg_len, a.n_real), dim3(64), 0, st, a);
  hipLaunchKernelGGL(sgs_grid_values_kernel, dim3(a.n_real), dim3(64 * kGridSeqWaves), 0, st, a);
  return hipGetLastError();
}

}  // namespace gsm
