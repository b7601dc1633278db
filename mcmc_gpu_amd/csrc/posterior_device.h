// What the posterior kernels share (posterior_kernel.hip, posterior_hist_kernel.hip, posterior_lag_kernel.hip, posterior_cov_kernel.hip,
// posterior_residual_kernel.hip, posterior_local_kernel.hip, posterior_regions_kernel.hip) and what
// gsm_api_posterior.hip sizes the slab by: the workgroup size, the 16-byte pack, the cut of the chain axis into parts, the cells
// per lane and the choice of a kernel's instantiation by state type and cells per lane.
#pragma once
#include "gsm_internal.h"
#include <algorithm>

namespace gsm {

constexpr int kPostBlock = 256;

template <typename T, int V>
struct alignas(sizeof(T) * V) Pack { T v[V]; };

// cells per lane: 16 bytes where the plane allows it, so that every chain's row of a lane starts on its own vector boundary
inline int posterior_vec(int64_t plane, int f32_state) {
  if (f32_state) return plane % 4 == 0 ? 4 : plane % 2 == 0 ? 2 : 1;
  return plane % 2 == 0 ? 2 : 1;
}

// workgroups along the cell axis of a pass with vec cells per lane
inline int64_t posterior_cell_blocks(int64_t plane, int vec) { return (plane / vec + kPostBlock - 1) / kPostBlock; }

// how many parts the chain axis is cut into so that cell_blocks * parts workgroups fill the CUs about four times over
inline int posterior_parts(int64_t cell_blocks, int n_chains, int n_cu) {
  const int64_t want = ((int64_t)n_cu * 4 + cell_blocks - 1) / cell_blocks;
  return (int)std::max<int64_t>(1, std::min<int64_t>(want, n_chains));
}

inline int chains_per_part(int n_chains, int parts) { return (n_chains + parts - 1) / parts; }

// the chains [c0, c1) of part blockIdx.y, cpp = chains_per_part chains to a part; the last parts may be short or empty
struct ChainRange { int c0, c1; };
__device__ __forceinline__ ChainRange chain_range(int cpp, int n_chains) {
  const int c0 = blockIdx.y * cpp;
  return {c0, min(n_chains, c0 + cpp)};
}

// Workgroup id -> work item so that the ids that share an L2 (id % 8: the workgroups are dealt over the 8 L2s round-robin by id) take
// a contiguous run of the n work items (bijective for any n: the first n % 8 runs are one longer).  For the tiled passes, whose
// neighbouring tiles read each other's halo.
constexpr int kXcds = 8;
__device__ __forceinline__ int xcd_contiguous(int id, int n) {
  const int q = n / kXcds, r = n % kXcds, x = id % kXcds;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + id / kXcds;
}

// workgroups of a grid-stride pass: one per per_block work items, at most eight to a CU
inline int grid_for(int64_t work_items, int per_block, int n_cu) {
  const int64_t want = (work_items + per_block - 1) / per_block;
  return (int)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)n_cu * 8));
}

// f(StateVec<T, V>{}): T the state type, V cells per lane.  dispatch_state gives the 16-byte width of the type (<float, 4>,
// <double, 2>), for the passes that are built for that width alone or that use T only; dispatch_state_vec also the narrower
// widths of posterior_vec.  Two functions so that a pass of the first kind is not instantiated for widths it never runs at.
template <typename T_, int V_>
struct StateVec { using T = T_; static constexpr int V = V_; };

template <typename F>
void dispatch_state(int f32_state, F&& f) {
  if (f32_state) f(StateVec<float, 4>{});
  else f(StateVec<double, 2>{});
}

template <typename F>
void dispatch_state_vec(int f32_state, int vec, F&& f) {
  if (vec == (f32_state ? 4 : 2)) dispatch_state(f32_state, f);
  else if (f32_state && vec == 2) f(StateVec<float, 2>{});
  else if (f32_state) f(StateVec<float, 1>{});
  else f(StateVec<double, 1>{});
}

// posterior_kernel.hip.  Every argument is validated by the C entry (gsm_api_posterior.hip); the launchers take them as they come.
constexpr int kLagMaxLags = 15;        // posterior_lag_kernel.hip: K x V fp64 accumulators and K loads per lane stay in registers
// out.f[i][cell] (+)= sum over parts, in part order, of slab[(p * n_fields + i) * plane + cell], i < n_fields <= kLagMaxLags
struct PostOut { double* f[kLagMaxLags]; };
hipError_t launch_posterior_combine(const double* slab, int parts, int n_fields, int64_t plane, const PostOut& out, int add, int n_cu,
                                    hipStream_t st);
hipError_t launch_posterior_accumulate(const void* beds, void* ref, double* s1, double* s2, int64_t n, int f32_state, int first, int n_cu,
                                       hipStream_t st);
hipError_t launch_posterior_pooled(const void* beds, const double* g, double* s1, double* s2, double* slab, int64_t plane, int n_chains,
                                   int parts, int f32_state, int n_cu, hipStream_t st);
hipError_t launch_posterior_partials(const void* ref, const double* g, const double* s1, const double* s2, double* slab, double* partials,
                                     int64_t plane, int n_chains, int n_seq, int64_t seq_stride, int n_closed, int n_per_seq, int parts, int f32_state,
                                     int n_cu, hipStream_t st);
hipError_t launch_posterior_close(const void* ref, const double* g, double* s1, double* s2, int64_t plane, int n_chains, int n_per_seq,
                                  int f32_state, hipStream_t st);
hipError_t launch_posterior_sample(const void* beds, const int32_t* cells, int n_samples, int n_chains, int64_t plane, int f32_state,
                                   double* out, hipStream_t st);
// posterior_hist_kernel.hip
constexpr int kHistMaxBins = 128;      // (bins + 4) / 2 KiB of LDS per workgroup
constexpr int kHistMaxLevels = 8;
hipError_t launch_posterior_histogram(const void* beds, const double* g, double inv_w, int n_bins, const double* levels, int n_levels,
                                      int32_t* counts, int64_t plane, int n_chains, int f32_state, int n_cu, hipStream_t st);
// posterior_lag_kernel.hip
hipError_t launch_posterior_lagged(const void* beds, void* ring, double* slab, double* lag_sqdiff, int64_t plane, int n_chains, int parts,
                                   int n_lags, int head, int n_valid, int f32_state, int n_cu, hipStream_t st);
// posterior_cov_kernel.hip.  n_probes <= kLagMaxLags: the fields one PostOut / combine launch carries
// cells per lane of the project kernel: 16 bytes of g and of every probe where the plane allows it, with either state type
inline int posterior_project_vec(int64_t plane) { return plane % 2 == 0 ? 2 : 1; }
// the most parts the project kernel cuts the plane into, so that parts * n_chains workgroups fill the CUs about eight times over;
// its slab holds n_chains * parts * n_probes partial projections
int posterior_project_parts(int64_t plane, int n_chains, int n_cu);
hipError_t launch_posterior_project(const void* beds, const double* g, const double* probes, double* slab, double* proj, int64_t plane,
                                    int n_chains, int n_probes, int f32_state, int n_cu, hipStream_t st);
hipError_t launch_posterior_cross(const void* beds, const double* g, const double* proj, double* slab, double* cross, int64_t plane,
                                  int n_chains, int parts, int n_probes, int f32_state, int n_cu, hipStream_t st);
// posterior_residual_kernel.hip.  3 + n_levels <= 7 fields: cnt, S1, S2, then one count per level
constexpr int kResMaxLevels = 4;
constexpr int kResMaxLanesXLog2 = 5;   // a tile is at most 32 lanes wide: 512 bytes of a row at 16 bytes per lane
constexpr int kResMinChains = 8;       // a part's workgroups load about 13 doubles per cell before their first chain: not for fewer chains than this
// the tile of the residual pass: vec cells of a row per lane (16 bytes where W allows it), 1 << lx_log2 lanes across and
// 256 >> lx_log2 rows, tiles_x * tiles_y tiles on the grid
struct ResTile { int vec, lx_log2, tiles_x, tiles_y; };
ResTile posterior_residual_tile(int H, int W, int f32_state);
// parts of the chain axis: posterior_parts over the tiles, but at least kResMinChains chains to a part; the slab holds parts x (3 +
// n_levels) planes
int posterior_residual_parts(const ResTile& t, int n_chains, int n_cu);
// levels [host, n_levels]
hipError_t launch_posterior_residual(const StaticFields& S, const void* beds, const double* rg, const double* levels, int n_levels,
                                     double* slab, double* sums, int n_chains, int parts, int f32_state, int n_cu, hipStream_t st);
// posterior_local_kernel.hip.  reach in [1, 4], K = 2 reach^2 + 2 reach offsets; the slab holds parts x K planes
constexpr int kLocalMaxReach = 4;
constexpr int kLocalSlabPlanes = 160;                        // parts x K stays at or below this: 4 parts at reach 4, 6 at 3, 13 at 2, 40 at 1
constexpr int64_t kLocalMaxSlabDoubles = (int64_t)1 << 27;   // and the slab at or below 1 GiB, by fewer parts
// tiles of 8 rows x 64 columns on the grid
int64_t posterior_local_tiles(int H, int W);
// parts of the chain axis: posterior_parts over the tiles, at most kLocalSlabPlanes / K and at most what keeps parts x K x H x W
// doubles within kLocalMaxSlabDoubles; 0 where one part's K planes alone exceed that (the call is refused)
int posterior_local_parts(int H, int W, int reach, int n_chains, int n_cu);
hipError_t launch_posterior_local(const void* beds, const double* g, double* slab, double* cross, int H, int W, int n_chains, int parts,
                                  int reach, int f32_state, int n_cu, hipStream_t st);
// posterior_regions_kernel.hip.  n_regions in [1, 8], n_bins 0 or even in [2, 64]
constexpr int kRegMaxRegions = 8;
constexpr int kRegMaxBins = 64;
// the most parts the regions kernel cuts the plane into, so that parts * n_chains workgroups fill the CUs about eight times over;
// its slab holds n_chains * parts * n_regions * 8 partial slots
int posterior_regions_parts(int64_t plane, int n_chains, int f32_state, int n_cu);
hipError_t launch_posterior_regions(const void* beds, const double* surf, const uint8_t* bits, int n_regions, double sea_level,
                                    double density_ratio, double* slab, double* func, double hyps_lo, double hyps_inv_w, int n_bins,
                                    int32_t* hyps, int64_t plane, int n_chains, int f32_state, int n_cu, hipStream_t st);

}  // namespace gsm
