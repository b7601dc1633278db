// Internal declarations shared by the translation units of libgsm_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>
#include "../../include/gsm.h"

namespace gsm {

// hipFuncSetAttribute is per device: one flag per (call site, device) -- `flags` is the call site's static array
constexpr int kMaxDevices = 64;
inline bool attr_needed_on_this_device(bool (&flags)[kMaxDevices], int& dev) {
  dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) { dev = -1; return true; }
  return !flags[dev];
}
// A pair of kernels with more dynamic LDS than the default limit: raise the limit of both to lds_cap once per device (the flags
// are this instantiation's, i.e. one set per kernel pair), then launch K0 if `first`, else K1.
template <auto K0, auto K1, class... Args>
inline hipError_t launch_pair(bool first, int lds_cap, dim3 grid, dim3 block, size_t lds, hipStream_t st, const Args&... args) {
  static bool attr_set[kMaxDevices] = {};
  int attr_dev;
  if (attr_needed_on_this_device(attr_set, attr_dev)) {
    hipError_t e = hipFuncSetAttribute((const void*)K0, hipFuncAttributeMaxDynamicSharedMemorySize, lds_cap);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)K1, hipFuncAttributeMaxDynamicSharedMemorySize, lds_cap);
    if (e != hipSuccess) return e;
    if (attr_dev >= 0) attr_set[attr_dev] = true;
  }
  if (first) hipLaunchKernelGGL(K0, grid, block, lds, st, args...);
  else hipLaunchKernelGGL(K1, grid, block, lds, st, args...);
  return hipGetLastError();
}

// Static fields shared by every chain of a handle (device pointers, H*W each, row-major).
struct StaticFields {
  const double* surf;
  const double* velx;
  const double* vely;
  const double* dhdt;
  const double* smb;
  const double* weight;   // nullptr => block_type 'RF'
  const uint8_t* upd;     // update / guard / resampled mask
  const uint8_t* mc;      // loss mask
  // packed copies for the step kernel's stencil: one 16-byte load per neighbour
  const double2* svx;     // (surf, velx)
  const double2* svy;     // (surf, vely)
  const double2* ds;      // (dhdt, smb)
  // folded operands of the flux step kernel (step_flux_kernel.hip): masks encoded as NaNs
  const double2* sA;      // (crf weight where update_mask else tagged NaN, surf)
  const double2* sB;      // (velx, vely)
  const double2* sC;      // (dhdt where mc_mask == 1 else NaN, smb)
  int H, W;
  // Rows [tr0, tr1) x columns [tc0, tc1): the bounding box of the set cells of `upd`, grown by one cell (the reach of the 5-point
  // stencil) and clipped to the grid; tr0 == tr1 and tc0 == tc1 when no cell is set.  No cell outside it changes its bed or its
  // energy in any step: the strip kernels cut every window down to it (strip_step.h: make_window).  Host-computed with the mask.
  int32_t tr0, tr1, tc0, tc1;
  double res;             // grid spacing h
  double two_res;         // 2.0 * h  (np.gradient interior denominator)
  double rcp_res;         // RN(1/h), RN(1/(2h)): used when fast_div
  double rcp_two_res;
  int fast_div;           // 1: x/h and x/(2 sigma^2) as fma-corrected reciprocal multiplies (bit-identical to IEEE division)
  double two_sigma2;      // 2 * sigma_mc**2
  double rcp_two_sigma2;  // RN(1/(2 sigma^2))
};

struct BlockTable {
  const int32_t* bh;      // device, n_sizes
  const int32_t* bw;      // device, n_sizes
  const double* masks;    // device, packed edge masks
  const int64_t* mask_off;  // device, n_sizes
  const double* mask1d;   // device [n_sizes][64] or nullptr: the edge masks as a function of the distance to the block's border,
                          // mask[y][x] = mask1d[size][min(y, bh - 1 - y, x, bw - 1 - x)] -- set when every mask has that form
                          // (get_edge_masks, MCMC.py:583-621: a logistic function of the distance to the nearest border cell)
  int n_sizes;
  int max_bh, max_bw;
};

struct StepArgs {
  StaticFields S;
  BlockTable B;
  int n_chains, n_steps;
  int tile_cap;           // doubles available for the LDS tile
  void* beds;             // [n_chains][H][W] double, or float when f32_state
  void* energy;           // [n_chains][H][W] masked squared residual of the current bed (0 where not counted)
  int f32_state;
  uint32_t* resampled;
  double* loss_sum;       // [n_chains][2]
  const int32_t* size_idx;
  const int32_t* centre;
  const double* u;
  const double* fields;
  int64_t field_stride;
  double* loss;
  uint8_t* accept;
  int32_t* blocks;        // optional [n_chains*n_steps*4] (row, col, bh, bw) or nullptr
  int64_t rec_stride;     // records per chain in the per-step arrays (== n_steps of the whole call)
  int64_t rec_offset;     // first record of this launch within a chain's row
  int64_t in_stride;      // records per chain in the proposal arrays (size_idx, centre, u, fields)
  int32_t* err_flag;      // device int, set non-zero on bad device data
  int strip;              // 1: the strip kernels (chain_strip_kernel.hip) take this block table; decided once per table by
                          // strip_table_ok so that the fused kernel and the replay kernel of a handle always pair up
};

// per-proposal scalars written by propose_scalars_kernel and read (uniformly) by propose_kernel
struct PropScalars {
  double scale, nug, range_x, range_y, u;
  double aa, m_const, m_kappa;   // spectral-amplitude parameters (MCMC.py:209-239); m_const = log(Matern constant) / 2
  int32_t si, row, col, bh;
  int32_t bw, fy_off, g_off, pad;   // block shape and DFT-table offsets: no dependent table look-ups in propose_kernel;
                                    // pad = offset of this shape's k^2 table in ProposeArgs::k2tab
  int64_t mask_off;
  // magic reciprocals (0xFFFFFFFF / d + 1) of the three divisors of a step -- half-plane columns bw/2 + 1, operand
  // columns M1, width of the window's halo tile -- so that no workgroup derives them with a uniform division
  uint32_t m_nc, m_m1, m_tw, reserved;
  // strip kernel (chain_strip_kernel.hip): the DFT operand tables are 1-D twiddle tables in LDS, indexed by (k * j) mod n:
  // magic reciprocals of the block height / width and the offsets of their [cos | sin](2 pi m / n) tables in ProposeArgs::tab1d
  uint32_t m_bh, m_bw;
  int32_t t1h_off, t1w_off;
};

struct ProposeArgs {
  BlockTable B;
  gsm_rf_params rf;
  int H, W;
  int n_chains, n_steps;
  int64_t step0;
  const uint64_t* seeds;
  const int32_t* centres;  // flat cell ids
  int n_centres;
  int32_t* size_idx;
  int32_t* centre;
  double* u;
  double* fields;
  int64_t field_stride;
  double* rf_scalars;      // optional
  // DFT operand tables (device), built by gsm_set_blocks; see proposal_kernel.hip for the shapes
  const double* tables;
  int tables_len;          // doubles in `tables`
  int tab_max;             // largest single table pair (2*KR*NR or 2*Kc*M1 doubles) over the block table
  const int32_t* fy_off;   // indexed by block height n: offset of [cos | sin](2 pi ky y / n), each [K1][N1]
  const int32_t* g_off;    // indexed by block width n: offset of the folded c2r table G, [K2][N2]
  int lds_sx, lds_st;      // LDS row strides of X and T^T (== 16 mod 32 doubles: conflict-free fragment reads)
  int lds_x_half;          // doubles per X plane (re or im)
  int lds_tt;              // doubles of T^T
  const double* mathtab;   // device copy of the table of math_tables.h (kMathTabDoubles doubles)
  int lds_main;            // max(4 * lds_x_half, lds_tt): T^T overlays X
  int tiles1_max, tiles2_max;  // largest stage-1 / stage-2 output-tile counts over the block table
  const double* tab1d;     // per distinct block length n: cos(2 pi m / n), m < n, then sin(2 pi m / n)  (the values of `tables`)
  const int32_t* t1_off;   // indexed by the length n: offset of its pair in tab1d
  const double* k2tab;     // (sqrt(kx^2 + ky^2) + 1e-10)^2 on ky <= bh/2, kx <= bw/2, one [nrow][ncol] table per block size
  const int32_t* k2_off;   // [n_sizes] offsets into k2tab
  PropScalars* scalars;    // device scratch, n_chains * n_steps records
  int parseval;            // the field's variance from the spectrum (Parseval) instead of from the field: same handles as split2 (the sum's order is that of
                           // 512-thread workgroups; proposal_device.h: coef_items, standardise)
  int split2;              // stage 2 of even block widths split by the parity of kx where the shape allows it (handles on the strip kernels: every kernel of
                           // such a handle holds two tile slots per wave; the flux-tile fused kernel holds one) -- proposal_device.h: prop_geom
};

// fused chain kernel (chain_fused_kernel.hip): step arguments + proposal arguments of the same call
struct FusedArgs {
  StepArgs T;
  ProposeArgs P;
  int work_len, fld_len;   // LDS region sizes in doubles, set by launch_chain_fused
  // gsm_run_noise (chain_strip_kernel<NOISE>): caller-supplied white noise instead of Philox draws -- record r's planes at
  // r * noise_stride (row-major (bh, bw)); noise_nug NULL: no nugget term
  const double* noise_re; const double* noise_im; const double* noise_nug;
  int64_t noise_stride;
};

// scratch + factor table of the Cholesky proposal generator (cholesky_kernel.hip)
struct CholArgs {
  int n_classes, n_groups;         // n_groups = n_sizes * n_classes
  const double* const* factors;    // device array [n_groups] of U matrices
  int* counts;                     // [n_groups]
  int* rec_off;                    // [n_groups + 1]
  int* tile_off;                   // [n_groups + 1]
  int* work_off;                   // [n_groups + 1] prefix of 64 x 128 output tiles (p-tiles x n-tiles) per group
  int64_t* z_off;                  // [n_groups]
  int* group_of;                   // [n_rec]
  int* order;                      // [n_rec]
  double* scale;                   // [n_rec]
  double* zbuf;                    // sum over groups of Npad * ppad doubles
};

// gsm_draw_pcg64 (pcg64_kernel.hip): NumPy's PCG64 generator streams of the reference's chains, on the device
struct PcgDrawArgs {
  int H, W, n_chains, n_steps, n_sizes;
  gsm_rf_params rf;
  const int32_t* bh; const int32_t* bw;          // block table
  uint64_t* rf_state;                            // [n_chains*6] state lo, hi, inc lo, hi, has_uint32, uinteger (in/out)
  uint64_t* ch_state;                            // same for the chain's generator
  const uint8_t* region_mask;                    // [H*W] or nullptr (update_in_region False)
  const uint64_t* jump; const uint64_t* zig;     // device copies of the constant tables
  int32_t* size_idx; int32_t* centre; double* u; double* rf_scalars;
  double* noise_re; double* noise_im; double* nugget;   // nugget may be nullptr (draws consumed, nothing stored)
  int64_t field_stride;
  int32_t* err;
};
hipError_t launch_pcg64_draw(const PcgDrawArgs& a, hipStream_t st);
constexpr int kPcgJumpWords = 4 * 512;          // = 4 * pcg::kJump (pcg64_device.h; checked there where both are visible)
void pcg64_host_tables(uint64_t* jump_out, const uint64_t** zig_out);
struct SgsDrawArgs;
hipError_t launch_sgs_draw_pcg64(const SgsDrawArgs& a, uint64_t* states, const uint64_t* jump, const uint64_t* zig, hipStream_t st);

// Device flags of the SGS and kriging kernels, OR-ed into the handle's error word (KrigeSearch::err, SgsDrawArgs::err,
// SgsGridDrawArgs::err) and decoded per entry point by gsm_api_sgs.hip's tables.  gsm_draw_pcg64's flags are another set.
enum SgsFlag : int32_t {
  kSgsFlagWindow = 1,        // a block window outside the grid or larger than 1024 cells, or more cells than max_cells
  kSgsFlagCell = 2,          // a listed cell outside its window / the grid, holding a value, or listed twice
  kSgsFlagNoValue = 4,       // no value anywhere on the grid for a cell's search
  kSgsFlagSingular = 8,      // a pivot of the kriging system below its tolerance
  kSgsFlagNoCentre = 16,     // no block centre inside the region mask
  kSgsFlagLagTable = 64,     // a lag between two chosen neighbours beyond the lag table
  kSgsFlagTruncnorm = 128,   // a truncated-normal draw outside scipy's domain
  kSgsFlagDrawPathLen = 256, // gsm_sgs_grid_draw_pcg64: the valueless cells of `cells` are not path_len many
  kSgsFlagDrawBadCell = 512, // gsm_sgs_grid_draw_pcg64: an entry of `cells` outside the grid
};
constexpr int kSgsMaxPts = 48;      // neighbours of a kriging system
constexpr int kSgsMaxWin = 1024;    // cells of a block window of the small-scale chain
// The grid, the variogram and the search of one SGS / kriging call: what sgs_search.h's octant_ring_search and krige_solve_at take
// (first member of SgsArgs, SgsGridArgs, KrigeGridArgs and KrigeCvArgs; filled by gsm_api_sgs.hip's krige_search_fill).
struct KrigeSearch {
  int H, W;
  const double* xs;        // [W] x coordinate of every column
  const double* ys;        // [H] y coordinate of every row
  const double* lag;       // [(2 mi + 1) * (2 mj + 1)] covariance at integer lag (di, dj), |di| <= mi, |dj| <= mj; or nullptr with `local`
  int mi, mj;
  const double* local;     // a variogram per cell, [H*W][6] = R00 R01 R10 R11 sill nugget, of model `vtype` (GSM_VTYPE_*); nullptr and 0 with `lag`
  int vtype;
  int hw, num_points;
  int ktype;               // 0 ordinary kriging (ok_solve), 1 simple kriging (sk_solve) with gmean
  const double* gmean;     // [n_chains] global mean of each chain's / realisation's conditioning values (simple kriging only)
  double radius, sill;
  int32_t* err;
};
// what every launcher of a kernel that searches checks again (the entry points have refused these with their own texts)
inline bool krige_search_ok(const KrigeSearch& K) {
  return K.hw >= 1 && K.num_points >= 8 && K.num_points <= kSgsMaxPts && K.H >= 2 && K.W >= 2 && K.H <= 32767 && K.W <= 32767 &&
         (K.lag == nullptr) != (K.local == nullptr);
}

// small-scale chain: sequential Gaussian simulation of one block per chain (sgs_kernel.hip)
struct SgsCellHdr {          // one per (chain, cell slot), written by sgs_weights_kernel
  int32_t n;                 // neighbours; -1: the cell holds conditioning data; -2: cell outside its window; 0: error
  int32_t op;                // block-local index of the cell
  double sdz;                // sqrt(|kriging variance|) * the cell's standard normal
  double var;                // |kriging variance|
  double c1;                 // (1 - sum of the kriging weights) / n
};
struct SgsArgs {
  KrigeSearch K;
  int n_chains;
  double* grid;            // [n_chains][H*W] in/out: the conditioning grid; the window's cells are rewritten
  const double* zcond;     // [H*W] or nullptr: initial content of the window cells (conditioning data, NaN elsewhere)
  const int32_t* win;      // [n_chains*4] r0, r1, c0, c1 of the simulated block
  int defer;               // 1: every cell outside the blocks holds a value (the caller's promise); sgs_weights_kernel then reads no grid value
                           //    -- the records name the cells -- and can run while the grid of the iteration before is still being written
  const int32_t* cell_off; // [n_chains+1] (or [n_chains] with cell_cnt)
  const int32_t* cell_cnt; // optional [n_chains]: number of cells of each chain
  const int32_t* cells;    // [total*2] (i, j) in simulation order
  const double* z;         // [total] standard normals
  double* trace;           // optional [total*3]: (neighbours, estimate, variance)
  int32_t* nbr_trace;      // optional [total*48]: the chosen neighbours (flat cell index, -1 padded) of every simulated cell
  // scratch of the handle: visiting ranks of the block cells and one record per (chain, cell slot)
  int max_cells;           // record stride per chain (>= the largest cell count of the call)
  int32_t* rank;           // [n_chains][1024]
  int32_t* rank_ok;        // [n_chains]
  SgsCellHdr* rec_hdr;     // [n_chains*max_cells]
  double2* rec_vw;         // [n_chains*max_cells/64][48][64]: entry e of 64 consecutive cell slots side by side -- (the neighbour's value,
                           //  or NaN-boxed (visiting slot << 16 | block-local index) where the neighbour is a cell simulated earlier in
                           //  the block; its kriging weight)
  const int32_t* group;    // [n_chains] or nullptr: the chain's group (gsm_sgs_set_groups); zcond is then [n_groups][H*W]
};
// interpolate.sgs on whole grids, many realisations at once (sgs_grid_kernel.hip)
struct SgsGridHdr {          // one per (realisation, path slot of the segment), written by sgs_grid_weights_kernel
  int32_t n;                 // neighbours; -3: the cell's bounds coincide (value = lower bound, no system); -2: invalid path entry; 0: error
  int32_t cell;              // flat grid index of the cell
  double sd;                 // sqrt(|kriging variance|)
  double var;                // |kriging variance|
  double c1;                 // ordinary: (1 - sum of the kriging weights) / n; simple: global mean * (1 - sum of the weights)
};
struct SgsGridArgs {
  KrigeSearch K;           // gmean [n_real]
  int n_real;
  double* grid;            // [n_real][H*W] normal scores, NaN where a value is to be simulated; the path cells are rewritten
  const int32_t* path;     // flat cell indices in visiting order, realisation r's at [path_off[r], path_off[r + 1])
  const int64_t* path_off; // [n_real + 1]
  const double* draw;      // [total] standard normal (draw_kind 0) or uniform (draw_kind 1) per path cell
  const double* lo;        // [H*W] transformed lower / upper bounds, or nullptr (draw_kind 0)
  const double* hi;
  int draw_kind;
  double* trace;           // optional [total*3]: (neighbours, estimate, variance) per path cell
  int32_t* rank;           // [n_real][H*W]: -1 conditioning value, slot of a path cell, INT32_MAX never filled
  int seg0, seg_len, seg_cap;   // this segment: slots [seg0, seg0 + seg_len); records per realisation (a multiple of 64)
  SgsGridHdr* rec_hdr;     // [n_real*seg_cap]
  double2* rec_vw;         // [n_real*seg_cap/64][48][64]: (value, or NaN-boxed (slot << 25 | cell) of a path cell; kriging weight)
};
// gsm_sgs_grid_draw_pcg64 (sgs_grid_draw_kernel.hip): path and draws of whole-grid SGS from NumPy's PCG64 streams, one wavefront per realisation
struct SgsGridDrawArgs {
  int H, W, n_real;
  uint64_t* states;          // [n_real*6] state lo, hi, inc lo, hi, has_uint32, uinteger (in/out)
  const int32_t* cells;      // [n_cells] flat indices of the cells of sim_mask in C order
  int n_cells;
  const uint8_t* has_value;  // [H*W] != 0 where the grid holds a conditioning value
  const double* lo;          // [H*W] transformed bounds (draw_kind GSM_DRAW_TRUNCATED), else nullptr
  const double* hi;
  int draw_kind;
  int32_t* work;             // [n_real][n_cells] the permutation of each realisation
  int32_t* path;             // [n_real][path_len]
  double* draws;             // [n_real][path_len]
  int path_len;
  const uint64_t* jump; const uint64_t* zig;     // device copies of the constant tables
  int32_t* err;
};
hipError_t launch_sgs_grid_draw_pcg64(const SgsGridDrawArgs& a, hipStream_t st);
// interpolate.krige: estimate and variance at listed cells of one grid (krige_grid_kernel.hip)
struct KrigeGridArgs {
  KrigeSearch K;           // gmean [1]
  int n_cells;
  int cell0;               // first entry of `cells` of this launch (set by launch_krige_grid)
  // The outputs stand before the inputs on purpose.  krige_grid_kernel uses every SGPR, and how the argument loads group decides
  // which spill slots the compiler can drop: with grid and cells first it keeps 36 bytes of (unused) private segment per lane.
  double* est;             // [n_cells] kriging estimate, in the order of `cells`; NaN where the cell raised an error
  double* var;             // [n_cells] sill - sum w rho, signed
  int32_t* n;              // [n_cells] neighbours; 0 where the cell raised an error
  const double* grid;      // [H*W] normal scores, NaN where there is no datum
  const int32_t* cells;    // [n_cells] flat indices of the cells to estimate (each NaN in grid)
};
hipError_t launch_krige_grid(const KrigeGridArgs& a, hipStream_t st);
// interpolate.cross_validate: every listed DATA cell kriged from the other data, under a hold-out, with up to kKrigeCvMaxModels
// candidate variograms per neighbour search (krige_cv_kernel.hip)
constexpr int kKrigeCvMaxModels = 8;
struct KrigeCvArgs {
  KrigeSearch K;           // gmean [1]; lag / local: model 0's table, model m's `model_stride` doubles further; sill and vtype unused
  int n_cells;
  int cell0;               // first entry of `cells` of this launch (set by launch_krige_cv)
  double* est;             // [n_models][n_cells] kriging estimate, in the order of `cells`; NaN where (model, cell) raised an error
  double* var;             // [n_models][n_cells] sill - sum w rho, signed
  int32_t* n;              // [n_cells] size of the solved systems (one neighbour set for all models); 0 where no search succeeded
  const double* grid;      // [H*W] normal scores, NaN where there is no datum
  const int32_t* cells;    // [n_cells] flat indices of the cells to validate (each holding a value)
  const int32_t* fold;     // [H*W] fold label of every cell (negative: in no fold), or nullptr
  double exclude_radius;   // > 0: cells within this distance of the target condition nothing
  int n_models;
  int64_t model_stride;    // doubles between two models' lag tables / per-cell tables
  double sill[kKrigeCvMaxModels];
  int vtype[kKrigeCvMaxModels];
};
hipError_t launch_krige_cv(const KrigeCvArgs& a, hipStream_t st);
hipError_t launch_sgs_grid_ranks(const SgsGridArgs& a, int max_path, hipStream_t st);
hipError_t launch_sgs_grid_segment(const SgsGridArgs& a, hipStream_t st);   // weights, then values of one segment
// gsm_debug_special: hipErrorInvalidValue for an unknown `which`, a NULL pointer it reads or n outside [1, 2^31 - 256)
hipError_t launch_debug_special(int which, int vtype, int64_t n, const double* x0, const double* x1, const double* x2, const double* x3,
                                const double* x4, double* out, int32_t* err, hipStream_t st);
hipError_t launch_sgs_blocks(const SgsArgs& a, int launch_cells, hipStream_t st);
hipError_t launch_sgs_weights(const SgsArgs& a, int launch_cells, hipStream_t st);     // ranks + records
hipError_t launch_sgs_sequence(const SgsArgs& a, hipStream_t st);                      // value pass
struct SgsDrawArgs {
  int H, W, n_chains, n_iters;
  int64_t iter0;
  const uint64_t* seeds;
  const uint8_t* region_mask;   // nullable
  const uint8_t* is_data;
  int min_x, max_x, min_y, max_y, max_cells;
  const double* mathtab;
  int32_t* win; int32_t* blk; int32_t* cell_off; int32_t* cell_cnt; int32_t* cells; double* z; double* u;
  int32_t* err;
};
hipError_t launch_sgs_draw(const SgsDrawArgs& a, hipStream_t st);
int sgs_loss_parts(const StaticFields& S);      // workgroups per chain of the loss kernel; scratch = n_chains * parts doubles + ints
// `group` of the launchers below: [n_chains] on the device or nullptr (gsm_sgs_set_groups).  With it trend is [n_groups][H*W] and the
// transformer's tables are [n_groups][nq], each read at the chain's group; without it the kernels are the ones they were.
hipError_t launch_sgs_loss(const StaticFields& S, int n_chains, const double* beds, const double* trend, double* loss, int32_t* bad,
                           double* part_sum, int32_t* part_bad, const int32_t* group, hipStream_t st);
// the operands of sgs_loss_tail_kernel (sgs_iter_kernel.hip), filled by gsm_sgs_iterate; `parts` is the launcher's
struct SgsTailArgs {
  const double* trend; int parts; double* part_sum; int32_t* part_bad; int32_t* ticket;
  double* loss; int32_t* bad; const double* u; double* loss_prev; uint8_t* accept; double* loss_rec; uint8_t* acc_rec; int64_t rec_stride;
  int mode; double* cur; double* beds; uint32_t* resampled; const int32_t* win;
  // QT (qt_q non-null): the two normal-score transforms of an iteration in this launch as well (see the kernel)
  const double* qt_q; const double* qt_ref; int qt_n; double clip_min, clip_max; double* next; double* next_acc;
  const int32_t* group;    // [n_chains] or nullptr (gsm_sgs_set_groups): trend, qt_q and qt_ref then hold one plane / table per group
};
hipError_t launch_sgs_loss_tail(const StaticFields& S, int n_chains, const SgsTailArgs& args, hipStream_t st);
bool sgs_tail_takes_qt(const StaticFields& S, int nq);
hipError_t launch_sgs_state_init(const StaticFields& S, int n_chains, const double* beds, const double* trend, double* energy, double* state,
                                 const int32_t* group, hipStream_t st);
hipError_t launch_sgs_finish(const StaticFields& S, int n_chains, double* cur, double* next, const double* trend, double* energy, double* state,
                             const int32_t* win, const double* u, uint32_t* resampled, uint8_t* accept, double* loss_rec, uint8_t* acc_rec,
                             int64_t rec_stride, int32_t* err, const int32_t* group, hipStream_t st);
hipError_t launch_sgs_decide(int n_chains, const double* loss_next, const int32_t* bad, const double* u, double* loss_prev,
                             uint8_t* accept, double* loss_rec, uint8_t* acc_rec, int64_t rec_stride, hipStream_t st);
hipError_t launch_qt(const double* quantiles, const double* references, int nq, double clip_min, double clip_max, const double* x,
                     double* out, int64_t n, int inverse, hipStream_t st);
// the same per chain with the tables of its group: x, out [n_chains][plane]
hipError_t launch_qt_groups(const double* quantiles, const double* references, int nq, double clip_min, double clip_max, const double* x,
                            double* out, int n_chains, int plane, const int32_t* group, int inverse, hipStream_t st);
hipError_t launch_sgs_commit_map(int H, int W, int n_chains, double* cur, const double* proposed, uint32_t* resampled, const int32_t* win,
                                 const uint8_t* accept, hipStream_t st);
hipError_t launch_sgs_commit(int H, int W, int n_chains, double* cur, double* next, uint32_t* resampled, const int32_t* win,
                             const uint8_t* accept, hipStream_t st);

// launchers (defined next to their kernels)
hipError_t launch_propose_cholesky(const ProposeArgs& a, const CholArgs& c, hipStream_t st);
hipError_t launch_cholesky_upper(double* A, int n, int ld, double jitter, int* d_info, hipStream_t st);
hipError_t launch_cov_assemble(int bh, int bw, double res, const gsm_vario& v, const double* lag_table, double* sigma,
                               int ld, hipStream_t st);
hipError_t launch_step(const StepArgs& a, hipStream_t st);
hipError_t launch_step_flux(const StepArgs& a, hipStream_t st);
bool step_flux_supported(const StepArgs& a);
hipError_t launch_pack_flux_static(const StaticFields& S, double2* sA, double2* sB, double2* sC, hipStream_t st);
hipError_t launch_init_loss(const StaticFields& S, int n_chains, const void* beds, void* energy, int f32_state,
                            double* loss_sum, double* loss0, hipStream_t st);
hipError_t launch_pack_static(const StaticFields& S, double2* svx, double2* svy, double2* ds, hipStream_t st);
hipError_t launch_residual(const StaticFields& S, int n_chains, const double* beds, double* out, hipStream_t st);
hipError_t launch_propose(const ProposeArgs& a, hipStream_t st);
hipError_t launch_propose_scalars(const ProposeArgs& a, hipStream_t st);
hipError_t launch_debug_normals(uint64_t seed, int64_t step, uint32_t stream_id, uint32_t idx0, int n, const double* mathtab, double* out,
                                hipStream_t st);
// gsm_debug_proposal_math: hipErrorInvalidValue for an unknown `which`, a NULL pointer it reads, n outside [1, 2^31 - 256) or an
// unknown model with GSM_PMATH_SPECTRAL_AMP; nothing is launched then
hipError_t launch_debug_proposal_math(int which, int model, double smoothness, int64_t n, const void* x0, const double* x1, const double* x2,
                                      const double* x3, const double* mathtab, void* out, hipStream_t st);
hipError_t launch_k2_tables(const BlockTable& B, const int32_t* k2_off, double resolution, double* k2tab, hipStream_t st);
hipError_t launch_spectral_from_noise(const ProposeArgs& a, const int32_t* size_idx, const double* rf_scalars, const double* noise_re,
                                      const double* noise_im, const double* nugget_field, hipStream_t st);
hipError_t launch_chain_fused(const FusedArgs& a, hipStream_t st);
hipError_t launch_chain_strip(const FusedArgs& a, hipStream_t st);
hipError_t launch_chain_strip_noise(const FusedArgs& a, hipStream_t st);
hipError_t launch_noise_chain_scalars(const ProposeArgs& a, const int32_t* size_idx, const int32_t* centre, const double* u,
                                      const double* rf_scalars, int32_t* err_flag, hipStream_t st);
hipError_t launch_step_strip(const StepArgs& a, hipStream_t st);
hipError_t launch_resampled_from_records(const FusedArgs& a, hipStream_t st);
bool strip_table_ok(const StaticFields& S, const BlockTable& B, int lds_main, int tiles1_max, int tiles2_max);
constexpr int kMask1D = 64;    // entries per block size of BlockTable::mask1d
bool fused_supported(const FusedArgs& a);
int propose_max_tiles_per_wave();
int propose_max_tiles1_per_wave();
int propose_waves();
size_t step_lds_bytes(int tile_cap);
hipError_t launch_min_dist(const double* xx, const double* yy, const uint8_t* mask, int n, double2* pts, int* count,
                           double* dist, hipStream_t st);
hipError_t launch_stream_copy(const double* src, double* dst, int64_t n, hipStream_t st);
// trend_kernel.hip: the weights of one axis of gsm_gaussian_filter, passed to its kernels by value
constexpr int kTrendMaxLw = 128;
struct TrendTaps { double w[2 * kTrendMaxLw + 1]; int lw; };
hipError_t launch_gaussian_filter(const TrendTaps& t0, const TrendTaps& t1, const double* x, double* tmp, double* out, int n, int H, int W,
                                  hipStream_t st);
// qt_fit_kernel.hip: the quantile tables of n fields of `cells` doubles; q [dev, nq]; keys0, keys1: n * cells keys each (sort_device.h).
// hipErrorInvalidValue: more workgroups than one launch takes
constexpr int64_t kQtFitMaxCells = int64_t(1) << 24;
constexpr int kQtFitMaxQuantiles = 1 << 20;
hipError_t launch_qt_fit(const double* x, int n, int64_t cells, const double* q, int nq, uint64_t* keys0, uint64_t* keys1, double* quantiles,
                         int64_t* n_valid, int64_t* n_inf, double* sorted, hipStream_t st);
// variogram_kernel.hip
constexpr int kVariogramMaxLag = 1 << 20;
int64_t variogram_workgroups(int mi, int mj);                           // workgroups per field and part
int variogram_default_rows_per_part(int H, int W, int mi, int mj);     // a function of the shape alone: results do not depend on the batch or the device
int variogram_parts(int H, int rows_per_part);
hipError_t launch_variogram_map(const double* fields, int n_fields, const uint8_t* mask, int H, int W, int mi, int mj, int rows_per_part,
                                double* psum, int64_t* pcount, double* sum, int64_t* count, hipStream_t st);
// variogram_local_kernel.hip: per-tile tables (k == 0: written to sum / count, tsum / tcount unused), then per-window sums of them
int64_t variogram_local_workgroups(int mi, int mj, int Tx);             // workgroups per field and tile row
hipError_t launch_variogram_local(const double* fields, int n_fields, const uint8_t* mask, int H, int W, int mi, int mj, int T, int k,
                                  double* tsum, int64_t* tcount, double* sum, int64_t* count, hipStream_t st);

}  // namespace gsm
