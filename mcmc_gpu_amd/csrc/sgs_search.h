// Octant search and kriging-system helpers shared by the block SGS kernels (sgs_kernel.hip) and the whole-grid SGS kernels
// (sgs_grid_kernel.hip): the search structure in LDS, the per-sector pruning, the ring walk and the Gauss-Jordan step.
// sgs_kernel.hip's header comment describes the search and the solve.
#pragma once
#include "device_util.h"
#include <math.h>
#ifndef GSM_SGS_LISTCAP
#define GSM_SGS_LISTCAP 80
#endif

namespace gsm {

constexpr int kSgsMaxPts = 48;
// candidates kept per sector between prunings (a scan pass appends at most 64; a list is pruned to its k8 nearest when it holds more than
// kSgsListCap - 64 = 16).  The search structure's LDS bounds the kernel's occupancy: 128 -> 80 entries, 64 rings of 16-bit certification
// counters instead of 128 of 32 bits took it from 17 KiB to 9.7 KiB per workgroup = 9 -> 16 wavefronts per CU (the register budget's
// four per SIMD): +14 % per iteration at 256 chains, the extra prunings included (same-box A/B of 128 / 112 / 96 / 88 / 80 entries)
constexpr int kSgsListCap = GSM_SGS_LISTCAP;
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

template <int K>
struct GjStep {
  // one Gauss-Jordan step on pivot K: r[] is this lane's row of [A | b] (columns 0..47 neighbours, 48 the Lagrange column,
  // 49 the right-hand side)
  static __device__ __forceinline__ void run(double (&r)[50], int lane, int n, bool lagr, double tol, double tol_l, double& mypiv, bool& singular) {
    if (K < n || (K == 48 && lagr)) {                            // wave-uniform: rows n..47 do not exist; no Lagrange row in simple kriging
      const dev::v2i32 pb = __builtin_bit_cast(dev::v2i32, r[K]);
      dev::v2i32 ps;
      ps.x = __builtin_amdgcn_readlane(pb.x, K);
      ps.y = __builtin_amdgcn_readlane(pb.y, K);
      const double pv = __builtin_bit_cast(double, ps);
      if (!(fabs(pv) > (K == 48 ? tol_l : tol))) singular = true;
      // 1 / pivot: hardware estimate + two Newton steps (every lane computes the same value), then the fma-corrected quotient
      double rp = __builtin_amdgcn_rcp(pv);
      rp = __fma_rn(__fma_rn(-pv, rp, 1.0), rp, rp);
      rp = __fma_rn(__fma_rn(-pv, rp, 1.0), rp, rp);
      double f = dev::exact_div(r[K], pv, rp);
      if (lane == K) { f = 0.0; mypiv = pv; }
#pragma unroll
      for (int j = K + 1; j < 50; ++j) {
        const dev::v2i32 b = __builtin_bit_cast(dev::v2i32, r[j]);
        dev::v2i32 o;
        o.x = __builtin_amdgcn_readlane(b.x, K);
        o.y = __builtin_amdgcn_readlane(b.y, K);
        r[j] = __fma_rn(-f, __builtin_bit_cast(double, o), r[j]);
      }
    }
    GjStep<K + 1>::run(r, lane, n, lagr, tol, tol_l, mypiv, singular);
  }
};
template <>
struct GjStep<49> {
  static __device__ __forceinline__ void run(double (&)[50], int, int, bool, double, double, double&, bool&) {}
};

}  // namespace gsm
