// gsm_sgs_grid_draw_pcg64: the random path and the draws of whole-grid interpolate.sgs made ON THE DEVICE from the callers' own
// NumPy generators -- what mcmc_gpu_amd/interpolate.py's _Plan.draws takes from numpy.random.Generator(PCG64) per realisation:
//   rng.shuffle(inds)                 interpolate.py:127.  Generator.shuffle of a 2-D array swaps rows, Fisher-Yates from the back:
//                                     for i = n - 1 .. 1: j = random_interval(i); swap(x[i], x[j]) -- masked rejection on 32-bit
//                                     words, the second half of a 64-bit draw cached in the generator (has_uint32, uinteger)
//   rng.standard_normal(path.size)    interpolate.py:174 (rng.normal(est, sd, 1) = est + sd * z): the ziggurat on next_uint64
//   rng.random(live.sum())            interpolate.py:185 (truncnorm.rvs draws one uniform): (next_uint64 >> 11) * 2^-53
// One wavefront per realisation, realisations side by side (pcg64_device.h: a wavefront holds one stream).  The permutation lives
// in global memory (`work`, 4 bytes per cell and realisation): up to 2^25 cells, far beyond the 1024 that sgs_draw_pcg64_kernel
// keeps in LDS.  The shuffle is a sequential chain of dependent loads -- the index of a swap comes from the generator, its two
// entries from memory -- so the index of swap i - 1 is drawn while the entries of swap i are in flight; the waves of the other
// realisations hide the rest of the latency.  Compaction (entries whose cell holds no value, in order) and the draws are all-lane
// passes: normals by Stream::normals, uniforms 64 path cells at a time, lane l decoding the draw its rank among the live cells
// of the window puts it at.
#include "gsm_internal.h"
#include "pcg64_device.h"
#include "ziggurat_tables.h"

namespace gsm {
static_assert(kPcgJumpWords >= 4 * pcg::kJumpWave, "jump table size");

__global__ __launch_bounds__(64) void sgs_grid_draw_pcg64_kernel(const SgsGridDrawArgs a) {
  __shared__ uint64_t jump[4 * pcg::kJumpWave];
  __shared__ uint64_t zig[kZigTabWords];
  const int lane = threadIdx.x, real = blockIdx.x;
  for (int i = lane; i < 4 * pcg::kJumpWave; i += 64) jump[i] = a.jump[i];
  for (int i = lane; i < kZigTabWords; i += 64) zig[i] = a.zig[i];
  __syncthreads();
  pcg::Stream G;
  uint64_t* gs = a.states + 6 * (size_t)real;
  G.s = pcg::u128{gs[0], gs[1]}; G.inc = pcg::u128{gs[2], gs[3]}; G.has32 = (uint32_t)gs[4]; G.cached = (uint32_t)gs[5];
  G.jump = jump; G.zig = zig;
  const int n = a.n_cells, n_grid = a.H * a.W;
  int32_t* work = a.work + (size_t)real * (size_t)n;
  int32_t* path = a.path + (size_t)real * (size_t)a.path_len;
  double* draws = a.draws + (size_t)real * (size_t)a.path_len;
  for (int k = lane; k < n; k += 64) work[k] = a.cells[k];
  __syncthreads();
  // rng.shuffle(inds): every lane draws the same indices (uniform code), lane 0 alone loads and stores the entries -- one thread's
  // loads and stores, ordered as the program orders them.  i == j: NumPy skips the swap, here both entries are written back as they were
  if (n > 1) {
    uint32_t j = G.interval((uint32_t)(n - 1));
    for (int i = n - 1; i >= 1; --i) {
      int32_t wi, wj;                                                              // lane 0's alone: no other lane reads them
      if (lane == 0) { wi = work[i]; wj = work[j]; }
      const uint32_t j_next = (i > 1) ? G.interval((uint32_t)(i - 1)) : 0u;       // while the two loads are in flight
      if (lane == 0) { work[i] = wj; work[j] = wi; }
      j = j_next;
    }
  }
  __syncthreads();
  // the path: entries of the shuffled list whose cell holds no value, in order
  const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  int count = 0;
  bool bad_cell = false;
  for (int k0 = 0; k0 < n; k0 += 64) {
    const int k = k0 + lane;
    bool free_cell = false;
    int32_t cell = 0;
    if (k < n) {
      cell = work[k];
      if (cell < 0 || cell >= n_grid) bad_cell = true;
      else free_cell = a.has_value[cell] == 0;
    }
    const unsigned long long m = __ballot(free_cell);
    const int pos = count + __popcll(m & below);
    if (free_cell && pos < a.path_len) path[pos] = cell;
    count += __popcll(m);
  }
  if (__ballot(bad_cell) != 0ull && lane == 0) atomicOr(a.err, kSgsFlagDrawBadCell);
  if (count != a.path_len) {
    // the caller's path_len is not the number of valueless cells: no draw is made, the generator stays behind the shuffle
    if (lane == 0) {
      atomicOr(a.err, kSgsFlagDrawPathLen);
      gs[0] = G.s.lo; gs[1] = G.s.hi; gs[4] = G.has32; gs[5] = G.cached;
    }
    return;
  }
  __syncthreads();
  if (a.draw_kind == GSM_DRAW_NORMAL) {
    const pcg::u128 A_l{jump[4 * lane], jump[4 * lane + 1]};
    const pcg::u128 C_l = pcg::mul128(pcg::u128{jump[4 * lane + 2], jump[4 * lane + 3]}, G.inc);
    G.normals(count, 0.0, 1.0, draws, lane, A_l, C_l);
  } else {
    // one uniform per path cell whose bounds differ (IEEE !=: a NaN bound is live), 0.0 at the others: a live cell consumes exactly
    // one 64-bit draw, so the cell of rank q among the live ones of a window takes the draw q + 1 ahead
    for (int p0 = 0; p0 < count; p0 += 64) {
      const int p = p0 + lane;
      bool live = false;
      if (p < count) { const int32_t cell = path[p]; live = a.lo[cell] != a.hi[cell]; }
      const unsigned long long m = __ballot(live);
      const int q = __popcll(m & below);
      double d = 0.0;
      if (live) d = pcg::to_double(pcg::output_xsl_rr(G.ahead(q + 1)));
      if (p < count) draws[p] = d;
      const int used = __popcll(m);
      if (used > 0) G.advance(used);
    }
  }
  // next_uint64 leaves the cached 32-bit word in place: has32 / cached are those the shuffle left
  if (lane == 0) { gs[0] = G.s.lo; gs[1] = G.s.hi; gs[4] = G.has32; gs[5] = G.cached; }
}

hipError_t launch_sgs_grid_draw_pcg64(const SgsGridDrawArgs& a, hipStream_t st) {
  if (a.n_real < 1) return hipSuccess;
  hipLaunchKernelGGL(sgs_grid_draw_pcg64_kernel, dim3(a.n_real), dim3(64), 0, st, a);
  return hipGetLastError();
}

}  // namespace gsm
