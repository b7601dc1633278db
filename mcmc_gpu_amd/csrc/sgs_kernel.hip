// Small-scale chain on gfx950: sequential Gaussian simulation of one block per chain.  The rest of an iteration -- loss, decision,
// commit, transforms, Philox draws -- is sgs_iter_kernel.hip.
//
// Replaces, for a batch of chains:
//   sgs                      gstatsMCMC/MCMC.py:91-173   (cell loop :135-168, radius widening :150-156)
//   neighbors (octant search) gstatsMCMC/gstatsim_custom/neighbors.py:4-64
//   ok_solve                 gstatsMCMC/gstatsim_custom/_krige.py:5-44
//
// The random numbers are the caller's (replay: NumPy's PCG64 on the host, in the reference's order; Philox mode:
// sgs_iter_kernel.hip's sgs_draw_kernel): the order in which the block's cells are visited (rng.shuffle, MCMC.py:128) and one standard normal per
// simulated cell (rng.normal(est, sqrt(var)) = est + sqrt(var) * z, MCMC.py:165).
//
// What depends on what.  A cell's NEIGHBOUR SET and KRIGING WEIGHTS depend only on where values exist when the cell is
// visited -- everything outside the block, the block's conditioning data, and the block cells visited before it -- not on the
// values themselves.  So the simulation of a block is split in two:
//   sgs_weights_kernel   one wavefront per (chain, cell), all cells of all chains side by side: octant search, ordinary-kriging
//                        system, weights and kriging variance -> a record per cell (neighbour list with the values that are
//                        known already, weights, standard deviation).  The search and the solve described below are
//                        sgs_search.h's octant_ring_search and krige_solve, which sgs_grid_kernel.hip and krige_grid_kernel.hip
//                        call too; this kernel says which cells qualify and writes the record;
//   sgs_sequence_kernel  one wavefront per chain walks the cells in visiting order: est = mean + sum w (v - mean),
//                        value = est + sd * z, the only sequential part (a 48-term dot product per cell).
//
// Octant search (exact for any search radius; the reference's driver uses 48 neighbours within 30 km at 500 m = 60 cells):
// every cell within +-hw of the cell that holds a value and lies closer than `radius` belongs to one of eight 45-degree
// sectors, (b pi/4, (b+1) pi/4], b = -4..3, of atan2(y0 - y, x0 - x), decided from the signs and magnitudes of the two
// coordinate differences -- exactly what numpy.arctan2 gives on the sector boundaries (multiples of pi/4 are hit only by
// cells on the axes and diagonals, where arctan2 returns the boundary value bit for bit; checked on the host).  Per sector
// the num_points / 8 nearest are kept, equidistant ones in ascending (row, column) -- numpy.argsort(kind='stable') of the
// reference's masked C-order array; the reference's default argsort is not stable, so its choice among equidistant
// candidates is implementation-defined.  The window is scanned in square rings of growing Chebyshev
// radius R.  After ring R every unscanned cell is at least (R + 1) min(|dx|, |dy|) away, so a sector is complete as soon as it
// holds num_points / 8 candidates closer than that; a sector whose remaining cells all lie outside the grid / window is
// exhausted.  The scan stops when every sector is complete or exhausted: with values on most cells that is after 4-6 rings,
// whatever the radius.  A cell without any value inside `radius` widens the search as the reference does (radius += 100 km,
// window = ceil(radius / |dx|) cells, MCMC.py:150-156) until the window covers the grid.
//
// Ordinary kriging: (n+1) x (n+1) system [Sigma 1; 1^T 0] w = [rho; 1], covariances from a table indexed by the integer lag
// between two cells (the host evaluates the reference's covariance model -- scipy's Bessel K for Matern -- once per lag),
// solved by Gauss-Jordan elimination on the diagonal (the covariance block is positive definite, the last pivot is
// -1' Sigma^-1 1) in fp64 with one row of the augmented matrix per lane, held in registers; the pivot row of a step reaches
// the other lanes through v_readlane.  The reference calls numpy.linalg.lstsq (SVD): same solution, other rounding -- the
// stated tolerance of this path.  A pivot below eps * N * max|diag| raises the "singular" flag (lstsq would truncate there).
// Limits: num_points <= 48, block <= 1024 cells.
#include "gsm_internal.h"
#include "device_util.h"
#include "proposal_device.h"
#include "sgs_search.h"
#include <math.h>

namespace gsm {

constexpr uint64_t kSgsPendingTag = 0x7FF8C0DE00000000ull;   // neighbour record: NaN-boxed (visiting slot << 16 | block-local index) of a cell visited earlier
// with SgsArgs::defer the values of the other neighbours are not in the record either (the weights do not depend on them: the
// records of an iteration can then be made while the iteration before is still running):
constexpr uint64_t kSgsWindowTag = 0x7FF8C0DF00000000ull;    // | block-local index: conditioning data inside the block (sgs_sequence_kernel's overlay holds it)
constexpr uint64_t kSgsGridTag = 0x7FF8C0E000000000ull;      // | flat grid index: a cell outside the block, read from the grid by sgs_sequence_kernel

// two sums over the 64 lanes at once, results wave-uniform.  The halves are folded first -- v_permlane32_swap (gfx950) exchanges the
// upper 32 lanes of `a` with the lower 32 of `b`, so a' + b' carries a[l] + a[l + 32] in lanes 0..31 and b[l] + b[l + 32] in lanes
// 32..63 -- and ONE chain of row reductions then sums both: 25 instructions instead of the 52 of two full wave reductions (the
// sequence kernel is one wavefront per chain: every instruction of the cell loop is 5-8 cycles of its critical path).
__device__ __forceinline__ void wave_sum2_f64(double& a, double& b) {
  typedef unsigned v2u32 __attribute__((ext_vector_type(2)));
  const dev::v2i32 ba = __builtin_bit_cast(dev::v2i32, a), bb = __builtin_bit_cast(dev::v2i32, b);
  const v2u32 lo = __builtin_amdgcn_permlane32_swap((unsigned)ba.x, (unsigned)bb.x, false, false);
  const v2u32 hi = __builtin_amdgcn_permlane32_swap((unsigned)ba.y, (unsigned)bb.y, false, false);
  dev::v2i32 na, nb;
  na.x = (int)lo.x; na.y = (int)hi.x; nb.x = (int)lo.y; nb.y = (int)hi.y;
  double z = __builtin_bit_cast(double, na) + __builtin_bit_cast(double, nb);
  z = dev::row16_sum(z);
  z += dev::dpp_f64<0x142, 0xA>(z);                             // row_bcast:15: rows 1 and 3 now hold the totals of their halves
  const dev::v2i32 bz = __builtin_bit_cast(dev::v2i32, z);
  dev::v2i32 oa, ob;
  oa.x = __builtin_amdgcn_readlane(bz.x, 31); oa.y = __builtin_amdgcn_readlane(bz.y, 31);
  ob.x = __builtin_amdgcn_readlane(bz.x, 63); ob.y = __builtin_amdgcn_readlane(bz.y, 63);
  a = __builtin_bit_cast(double, oa); b = __builtin_bit_cast(double, ob);
}

// ---------------------------------------------------------------------------------------------------------------------
// sgs_rank_kernel: per chain, the visiting rank of every block cell (-1: the cell holds conditioning data and is never
// simulated), so that the search of cell k knows which block cells hold a value when k is visited.  One workgroup per chain.
// ---------------------------------------------------------------------------------------------------------------------
// G (all three kernels of this file): the handle has chain groups (gsm_sgs_set_groups) and zcond is [n_groups][H*W], read at the plane of
// the chain's group; without groups (G = false) the kernels are the ones they were.
template <bool G>
__device__ __forceinline__ const double* sgs_zcond_of(const SgsArgs& a, int chain) {
  return (G && a.zcond) ? a.zcond + (size_t)a.group[chain] * a.K.H * a.K.W : a.zcond;
}
template <bool G>
__global__ __launch_bounds__(256) void sgs_rank_kernel(const SgsArgs a) {
  const int chain = blockIdx.x, tid = threadIdx.x;
  const int H = a.K.H, W = a.K.W;
  const double* zcond = sgs_zcond_of<G>(a, chain);
  const int r0 = a.win[4 * chain], r1 = a.win[4 * chain + 1], c0 = a.win[4 * chain + 2], c1 = a.win[4 * chain + 3];
  const int wh = r1 - r0, ww = c1 - c0;
  int32_t* rank = a.rank + (size_t)chain * kSgsMaxWin;
  const int k_lo = a.cell_off[chain], cnt = a.cell_cnt ? a.cell_cnt[chain] : a.cell_off[chain + 1] - k_lo;
  if (r0 < 0 || c0 < 0 || r1 > H || c1 > W || wh < 0 || ww < 0 || wh * ww > kSgsMaxWin || cnt > a.max_cells || cnt < 0) {
    if (tid == 0) { atomicOr(a.K.err, kSgsFlagWindow); a.rank_ok[chain] = 0; }
    return;
  }
  if (tid == 0) a.rank_ok[chain] = 1;
  for (int p = tid; p < wh * ww; p += 256) rank[p] = 0x7fffffff;          // a window cell that is not listed never holds a value
  __syncthreads();
  const double* g = a.grid + (size_t)chain * H * W;
  for (int k = tid; k < cnt; k += 256) {
    const int i = a.cells[2 * (k_lo + k)], j = a.cells[2 * (k_lo + k) + 1];
    if (i < r0 || i >= r1 || j < c0 || j >= c1) { atomicOr(a.K.err, kSgsFlagCell); continue; }
    const double v = zcond ? zcond[i * W + j] : g[i * W + j];
    rank[(i - r0) * ww + (j - c0)] = isnan(v) ? k : -1;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// sgs_weights_kernel: one 64-lane workgroup (one wavefront) per (cell slot, chain)
// ---------------------------------------------------------------------------------------------------------------------
template <bool G>
__global__ __launch_bounds__(64) void sgs_weights_kernel(const SgsArgs a) {
  __shared__ SgsSearchLds L;
  const int slot = blockIdx.x, chain = blockIdx.y, lane = threadIdx.x;
  const double* zcond = sgs_zcond_of<G>(a, chain);
  if (!a.rank_ok[chain]) return;
  const int k_lo = a.cell_off[chain], cnt = a.cell_cnt ? a.cell_cnt[chain] : a.cell_off[chain + 1] - k_lo;
  if (slot >= cnt) return;
  const int H = a.K.H, W = a.K.W;
  const size_t rec = (size_t)chain * a.max_cells + slot;
  const int i0 = a.cells[2 * (k_lo + slot)], j0 = a.cells[2 * (k_lo + slot) + 1];
  const int r0 = a.win[4 * chain], r1 = a.win[4 * chain + 1], c0 = a.win[4 * chain + 2], c1 = a.win[4 * chain + 3];
  const int ww = c1 - c0;
  if (i0 < r0 || i0 >= r1 || j0 < c0 || j0 >= c1) { if (lane == 0) a.rec_hdr[rec].n = -2; return; }     // flagged by sgs_rank_kernel
  const int32_t* rank = a.rank + (size_t)chain * kSgsMaxWin;
  if (rank[(i0 - r0) * ww + (j0 - c0)] != slot) { if (lane == 0) { a.rec_hdr[rec].n = -1; a.rec_hdr[rec].op = (i0 - r0) * ww + (j0 - c0); } return; }       // conditioned already (MCMC.py:141)
  const double* __restrict__ g = a.grid + (size_t)chain * H * W;
  // rk: -1 = conditioning data, < slot = simulated before this cell
  auto qualifies = [&](int ic, int jc) {
    const bool inwin = ic >= r0 && ic < r1 && jc >= c0 && jc < c1;
    const int rk = rank[inwin ? (ic - r0) * ww + (jc - c0) : 0];
    const double gv = a.defer ? 0.0 : g[ic * W + jc];            // defer: every cell outside the block holds a value (the caller's promise)
    return inwin ? rk < slot : !isnan(gv);
  };
  const int n = octant_ring_search(L, qualifies, i0, j0, H, W, a.K.xs, a.K.ys, a.K.radius, a.K.hw, a.K.num_points / 8, lane);
  // a cell that fails gets no values: n = 0 in its record
  auto give_up = [&](int32_t flag) {
    if (lane == 0) { atomicOr(a.K.err, flag); a.rec_hdr[rec].n = 0; a.rec_hdr[rec].op = (i0 - r0) * ww + (j0 - c0); }
  };
  if (n == 0) { give_up(kSgsFlagNoValue); return; }                            // no value anywhere on the grid: the reference would loop forever
  const bool lagr = a.K.ktype == 0;
  double w_l, rho_l, sill;
  int my_i, my_j;
  if (const int e = krige_solve_at<false, true>(L, a.K, i0 * W + j0, n, i0, j0, lagr, lane, w_l, rho_l, my_i, my_j, sill)) { give_up(e); return; }
  double var = sill - dev::wave64_sum(w_l * rho_l);
  var = fabs(var);
  const double sw = dev::wave64_sum(w_l);
  // ---- the cell's record ---------------------------------------------------------------------------------------------
  if (lane < kSgsMaxPts) {
    double2 vw = make_double2(0.0, 0.0);
    int gg = -1;
    if (lane < n) {
      gg = L.nb_g[lane];
      vw.y = w_l;
      const bool inblk = my_i >= r0 && my_i < r1 && my_j >= c0 && my_j < c1;
      const int nb_pos = (my_i - r0) * ww + (my_j - c0);
      const int nb_slot = inblk ? rank[nb_pos] : -1;
      if (nb_slot >= 0)          // simulated earlier in this block: its visiting slot and its block-local index (both < 1024)
        vw.x = __builtin_bit_cast(double, kSgsPendingTag | ((uint64_t)nb_slot << 16) | (uint64_t)nb_pos);
      else if (a.defer)
        vw.x = __builtin_bit_cast(double, inblk ? (kSgsWindowTag | (uint64_t)nb_pos) : (kSgsGridTag | (uint64_t)(uint32_t)gg));
      else
        vw.x = (inblk && zcond) ? zcond[gg] : g[gg];
    }
    // entry `lane` of 64 consecutive cell slots lies side by side: sgs_sequence_kernel reads one cell per lane
    a.rec_vw[((rec >> 6) * kSgsMaxPts + lane) * 64 + (rec & 63)] = vw;
    if (a.nbr_trace) a.nbr_trace[(size_t)(k_lo + slot) * kSgsMaxPts + lane] = gg;
  }
  if (lane == 0) {
    SgsCellHdr hd;
    hd.n = n; hd.op = (i0 - r0) * ww + (j0 - c0); hd.sdz = sqrt(var) * a.z[k_lo + slot]; hd.var = var;
    // ordinary: est = local mean + sum w (v - local mean) (_krige.py:42) -> c1 = (1 - sum w) / n multiplies sum v;
    // simple:   est = global mean + sum w (v - global mean) (_krige.py:79) -> c1 = global mean * (1 - sum w) is added as it is
    hd.c1 = lagr ? (1.0 - sw) / (double)n : a.K.gmean[chain] * (1.0 - sw);
    a.rec_hdr[rec] = hd;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// sgs_sequence_kernel: one workgroup of four wavefronts per chain; the block's cells in visiting order, 64 at a time, one
// cell per lane.  The value pass is a sparse unit-lower-triangular solve (I - A) v = c with A[j][k] the coefficient of the
// earlier block cell k in the estimate of cell j (w_jk + (1 - sum w_j) / n_j in ordinary kriging, w_jk in simple kriging)
// and c the part of the estimate that is known already plus sd * z.  Per chunk of 64 cells:
//   gather      (all four waves, every fourth group of four list entries each) every lane walks its own cell's neighbour list:
//               values known before the block and values of cells of EARLIER chunks (final by now, in `overlay`) are summed;
//               the coefficient of a neighbour in the SAME chunk goes to column `lane` of a 64 x 64 tile in LDS, and one bit
//               of a 64-bit mask per lane says which of the tile's entries exist;
//   sequence    (wave 0) cell kk of the chunk is final once the cells before it are: its value is broadcast (v_readlane) and
//               every lane that lists it adds coefficient * value -- two v_readlane and one fma on the chain's critical path
//               per cell, where a wave reduction over the neighbour list per cell cost 650-800 cycles.
// The records of the next chunk are requested (LDS-DMA) before the sequence part of the current one and land meanwhile.
// A cell whose kriging system failed (n == 0, error flag raised by sgs_weights_kernel) gets NaN, and so does every later
// cell of its chunk and every cell that lists one of those.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kSeqWaves = 4;
template <bool G>
__global__ __launch_bounds__(64 * kSeqWaves) void sgs_sequence_kernel(const SgsArgs a) {
  __shared__ double overlay[kSgsMaxWin];
  __shared__ double tile[65 * 64];                              // [cell of the chunk the value comes from][lane = cell that uses it]; row 64 takes the writes of absent entries
  __shared__ __attribute__((aligned(16))) double2 stage[kSgsMaxPts * 64];      // a chunk's neighbour records, [entry][cell]
  __shared__ double2 part[kSeqWaves][64];                       // per wave and cell: (sum v, sum w v) over the wave's share of the list
  __shared__ uint64_t mpart[kSeqWaves][64];
  const int chain = blockIdx.x, lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (!a.rank_ok[chain]) return;
  const int H = a.K.H, W = a.K.W;
  const double* zcond = sgs_zcond_of<G>(a, chain);
  double* __restrict__ g = a.grid + (size_t)chain * H * W;
  const int r0 = a.win[4 * chain], r1 = a.win[4 * chain + 1], c0 = a.win[4 * chain + 2], c1 = a.win[4 * chain + 3];
  const int wh = r1 - r0, ww = c1 - c0;
  const int k_lo = a.cell_off[chain], cnt = a.cell_cnt ? a.cell_cnt[chain] : a.cell_off[chain + 1] - k_lo;
  const int np8 = (a.K.num_points + 7) & ~7;
  const size_t rec0 = (size_t)chain * a.max_cells;              // a multiple of 64 (sgs_fill)
  const double* __restrict__ vw_src = (const double*)(a.rec_vw + rec0 * kSgsMaxPts);
  const double4* __restrict__ hdr_src = (const double4*)(a.rec_hdr + rec0);
  static_assert(sizeof(SgsCellHdr) == 32, "a header is one double4");
  double4 hd = make_double4(0.0, 0.0, 0.0, 0.0);
  // The records of a chunk travel global -> LDS by LDS-DMA (no registers; whole 1 KiB pieces = one entry of 64 cells, piece c by
  // wave c mod 4); the headers (one per lane, the same in every wave) come through registers.
  auto request = [&](int kc) {
    hd = hdr_src[kc + lane];
    dma_to_lds<kSeqWaves, 0>(vw_src + (size_t)(kc >> 6) * kSgsMaxPts * 128, (double*)stage, np8 * 128, wave, lane);
  };
  if (cnt > 0) request(0);
  for (int p = threadIdx.x; p < wh * ww; p += 64 * kSeqWaves) {
    const int gi = (r0 + p / ww) * W + c0 + p % ww;
    overlay[p] = zcond ? zcond[gi] : g[gi];
  }
  for (int kc = 0; kc < cnt; kc += 64) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // this wave's pieces of the chunk's records and its headers have landed
    __syncthreads();                                            // ... and everybody's; the overlay holds every cell of the chunks before
    const int j = kc + lane;
    const uint64_t nop = __builtin_bit_cast(uint64_t, hd.x);
    const int n = (j < cnt) ? (int)(uint32_t)nop : -2, op = (int)(nop >> 32);
    const double sdz = hd.y, var = hd.z, c1 = hd.w;
    // ---- gather ----  (no branches; this wave's entries 4 wave + 16 k + u: all their reads first -- records from LDS, deferred values
    // from the grid, earlier cells from the overlay --, then the sums and the tile's entries)
    double sv = 0.0, swv = 0.0;
    uint64_t mask = 0;
    {
      double2 r[12];
      double gvv[12], ov[12];
#pragma unroll
      for (int q = 0; q < 12; ++q) r[q] = stage[(4 * wave + 16 * (q >> 2) + (q & 3)) * 64 + lane];
#pragma unroll
      for (int q = 0; q < 12; ++q) {
        const int e = 4 * wave + 16 * (q >> 2) + (q & 3);
        const uint64_t bits = __builtin_bit_cast(uint64_t, r[q].x);
        const uint32_t hi = (uint32_t)(bits >> 32), lo = (uint32_t)bits;
        gvv[q] = g[(e < n && hi == (uint32_t)(kSgsGridTag >> 32)) ? lo : 0u];
      }
#pragma unroll
      for (int q = 0; q < 12; ++q) {
        const int e = 4 * wave + 16 * (q >> 2) + (q & 3);
        const uint64_t bits = __builtin_bit_cast(uint64_t, r[q].x);
        const uint32_t hi = (uint32_t)(bits >> 32), lo = (uint32_t)bits;
        const bool early = (e < n) && ((hi == (uint32_t)(kSgsPendingTag >> 32) && (int)(lo >> 16) < kc) || hi == (uint32_t)(kSgsWindowTag >> 32));
        ov[q] = overlay[early ? (lo & 0xFFFFu) : 0u];
      }
#pragma unroll
      for (int q = 0; q < 12; ++q) {
        const int e = 4 * wave + 16 * (q >> 2) + (q & 3);
        const uint64_t bits = __builtin_bit_cast(uint64_t, r[q].x);
        const uint32_t hi = (uint32_t)(bits >> 32), lo = (uint32_t)bits;
        const double w = r[q].y;
        const bool pend = hi == (uint32_t)(kSgsPendingTag >> 32), inwin = hi == (uint32_t)(kSgsWindowTag >> 32), ingrid = hi == (uint32_t)(kSgsGridTag >> 32);
        const int ks = (int)(lo >> 16) - kc;                     // >= 0: a cell of this chunk (visited before this one: ks < lane)
        const bool here = (e < n) && pend && ks >= 0, known = (e < n) && !(pend && ks >= 0);
        const double v = ingrid ? gvv[q] : ((pend || inwin) ? ov[q] : r[q].x);
        const double wv = w * v;
        sv += known ? v : 0.0;
        swv += known ? wv : 0.0;
        tile[here ? ks * 64 + lane : 64 * 64 + lane] = (a.K.ktype == 0) ? w + c1 : w;       // row 64: nobody reads it
        mask |= here ? (1ull << ks) : 0ull;
      }
    }
    part[wave][lane] = make_double2(sv, swv);
    mpart[wave][lane] = mask;
    __syncthreads();                                            // the records have been read: the next chunk's may overwrite them
    if (kc + 64 < cnt) request(kc + 64);
    if (wave != 0) continue;
    // ---- sequence (wave 0) ----
    sv = 0.0; swv = 0.0; mask = 0;
#pragma unroll
    for (int w = 0; w < kSeqWaves; ++w) { const double2 q = part[w][lane]; sv += q.x; swv += q.y; mask |= mpart[w][lane]; }
    // est = mean + sum w (v - mean) (_krige.py:42) as sum w v + sum v * (1 - sum w) / n with c1 = (1 - sum w) / n from the record;
    // simple kriging (_krige.py:79): sum w v + global mean * (1 - sum w) = c1
    // val = est + sd z is what travels: value of the cell = (known part of the estimate + sd z) + the chunk's own cells' part
    // n == 0: error flagged by sgs_weights_kernel -> NaN; a lane without a cell to simulate must hold a finite number (0 * NaN)
    double val = (n > 0) ? (swv + (a.K.ktype == 0 ? sv * c1 : c1)) + sdz : (n == 0 ? NAN : 0.0);
    const int kend = min(64, cnt - kc);
    for (int k8 = 0; k8 < kend; k8 += 8) {
      double t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) { const double tt = tile[(k8 + u) * 64 + lane]; t[u] = ((mask >> (k8 + u)) & 1ull) ? tt : 0.0; }
#pragma unroll
      for (int u = 0; u < 8; ++u) val = __fma_rn(t[u], dev::readlane_f64(val, k8 + u), val);     // lane k8 + u is final: every cell it lists came before
    }
    if (n == -1) {                                              // conditioned already: nothing drawn for it (MCMC.py:141)
      if (a.trace) { a.trace[3 * (k_lo + j)] = -1.0; a.trace[3 * (k_lo + j) + 1] = overlay[op]; a.trace[3 * (k_lo + j) + 2] = 0.0; }
    } else if (n >= 0) {
      overlay[op] = val;
      if (a.trace && n > 0) { a.trace[3 * (k_lo + j)] = (double)n; a.trace[3 * (k_lo + j) + 1] = val - sdz; a.trace[3 * (k_lo + j) + 2] = var; }
    }
  }
  __syncthreads();
  for (int p = threadIdx.x; p < wh * ww; p += 64 * kSeqWaves) g[(size_t)(r0 + p / ww) * W + c0 + p % ww] = overlay[p];
}

// the two halves of launch_sgs_blocks: the records of every cell (visiting ranks, then search + kriging weights), and the value pass
hipError_t launch_sgs_weights(const SgsArgs& a, int launch_cells, hipStream_t st) {
  if (!krige_search_ok(a.K)) return hipErrorInvalidValue;
  if (a.group) {
    hipLaunchKernelGGL(sgs_rank_kernel<true>, dim3(a.n_chains), dim3(256), 0, st, a);
    if (launch_cells > 0) hipLaunchKernelGGL(sgs_weights_kernel<true>, dim3(launch_cells, a.n_chains), dim3(64), 0, st, a);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(sgs_rank_kernel<false>, dim3(a.n_chains), dim3(256), 0, st, a);
  if (launch_cells > 0) hipLaunchKernelGGL(sgs_weights_kernel<false>, dim3(launch_cells, a.n_chains), dim3(64), 0, st, a);
  return hipGetLastError();
}
hipError_t launch_sgs_sequence(const SgsArgs& a, hipStream_t st) {
  if (!krige_search_ok(a.K)) return hipErrorInvalidValue;
  if (a.group) hipLaunchKernelGGL(sgs_sequence_kernel<true>, dim3(a.n_chains), dim3(64 * kSeqWaves), 0, st, a);
  else hipLaunchKernelGGL(sgs_sequence_kernel<false>, dim3(a.n_chains), dim3(64 * kSeqWaves), 0, st, a);
  return hipGetLastError();
}
hipError_t launch_sgs_blocks(const SgsArgs& a, int launch_cells, hipStream_t st) {
  hipError_t e = launch_sgs_weights(a, launch_cells, st);
  return e != hipSuccess ? e : launch_sgs_sequence(a, st);
}

}  // namespace gsm
