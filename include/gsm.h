/*
 * gsm.h -- C ABI of the MI355X-native many-chain geostatistical MCMC sampler (libgsm_hip.so).
 *
 * This is the drop-in boundary for ONE hot path of tylerrleee/mcmc-gpu: the large-scale-chain
 * Metropolis step.  Every entry point names the reference interface it replaces (paths relative to
 * the reference repository root).  The reference is pure Python, so its "FFI" for this path is a
 * ctypes binding; INTEGRATION.md shows the stub a maintainer adds to gstatsMCMC/MCMC_gpu.py.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no torch / C++ types cross the boundary.
 *   - Every pointer marked [dev] is a DEVICE pointer (e.g. torch.Tensor.data_ptr() of a cuda tensor),
 *     row-major, borrowed for the duration of the call (asynchronous calls: until the stream has been
 *     synchronised).  The caller owns all state; the library owns only its handle and scratch.
 *   - Return value 0 = ok, negative = error (GSM_E_*); gsm_last_error() gives the text.  No C++
 *     exception crosses the ABI.  A handle is not thread-safe; distinct handles are independent.
 *   - "stream" is a hipStream_t passed as void* (0 = the null stream).  Kernels are enqueued on it and
 *     the call returns without synchronising unless stated.
 *   - Grids are H rows x W columns.  Static fields are fp64; the per-chain state (beds, energy) is fp64, or
 *     fp32 for a handle created with dtype 1 (then `void* beds` / `void* energy` point to float arrays).
 *     Chain c's bed starts at element c*H*W.
 *
 * Layout of per-step records, for chain c and step s of a call with n_steps steps: index c*n_steps+s.
 */
#ifndef GSM_H
#define GSM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gsm_context* gsm_handle;

enum {
  GSM_OK = 0,
  GSM_E_ARG = -1,       /* bad argument (null pointer, non-positive size, block larger than grid ...) */
  GSM_E_STATE = -2,     /* call order violated (e.g. run before set_static) */
  GSM_E_HIP = -3,       /* a HIP runtime call failed */
  GSM_E_UNSUPPORTED = -4, /* valid request this build cannot serve (dtype, block larger than the LDS tile) */
  GSM_E_DEVICE_DATA = -5  /* a kernel found an out-of-range size index / block centre in device data */
};

enum { GSM_MODEL_GAUSSIAN = 0, GSM_MODEL_EXPONENTIAL = 1, GSM_MODEL_MATERN = 2 };

/* Random-field parameters: mirrors RandField.__init__ (gstatsMCMC/MCMC.py:462-510) plus the grid
 * resolution handed to spectral_synthesis_field (MCMC.py:176, :767). */
typedef struct {
  double range_min_x, range_max_x, range_min_y, range_max_y;
  double scale_min, scale_max;
  double nugget_max;
  double smoothness;  /* Matern nu; ignored otherwise */
  double resolution;
  int32_t model;      /* GSM_MODEL_* */
  int32_t isotropic;  /* 1: one range draw shared by x and y (MCMC.py:207) */
  int32_t generator;  /* GSM_GEN_SPECTRAL (reference's generator) or GSM_GEN_CHOLESKY (precomputed factors) */
  int32_t reserved;
} gsm_rf_params;

enum { GSM_GEN_SPECTRAL = 0, GSM_GEN_CHOLESKY = 1 };
enum { GSM_VTYPE_EXPONENTIAL = 0, GSM_VTYPE_GAUSSIAN = 1, GSM_VTYPE_SPHERICAL = 2, GSM_VTYPE_MATERN = 3 };

/* Variogram of gstatsim_custom (the `vario` dict of _krige.py:83-122 / covariance.py:4-28). */
typedef struct {
  double azimuth, major_range, minor_range, sill, nugget, s;
  int32_t vtype;      /* GSM_VTYPE_* */
  int32_t reserved;
} gsm_vario;

/* Library / build identification: "gsm-hip <version> gfx950 src:<hash>", hash = first 16 hex digits of the SHA-256 of the
 * library sources at build time (the Python loader checks it against the sources it sees). */
const char* gsm_version(void);

/* Text of the last error on this handle (or of the last failed gsm_create when h is NULL). */
const char* gsm_last_error(gsm_handle h);

/* Create a sampler for n_chains chains on an H x W grid on HIP device `device`.
 * dtype: 0 = fp64 state; 1 = fp32 state with fp64 arithmetic (beds and energy are float arrays; every value is
 * rounded to float before it is used, so the carried loss sum always equals the sum of what is stored --
 * BASELINE configs[4]; the reference's torch class is all-fp32, MCMC_gpu.py:261).
 * H, W >= 1; a handle whose grid has a side below 3 cells serves gsm_gaussian_filter alone (axes of one or two cells are cases of
 * its reflection) and every other entry point returns GSM_E_ARG on it: their stencils and searches need 3 x 3 cells.
 * Replaces: the per-process chain construction of lsc_run_wrapper
 * (largeScaleChain_multiprocessing_GPU.py:126-127) -- one handle holds all chains of one GPU. */
int gsm_create(gsm_handle* out, int32_t H, int32_t W, int32_t n_chains, int32_t dtype, int32_t device);
int gsm_destroy(gsm_handle h);

/* Static fields shared by all chains [dev, H*W each].  crf_weight may be NULL => block_type 'RF'
 * (MCMC.py:1279-1282).  update_mask: 1 where a proposal may change the bed AND where the thickness
 * guard and resampled_times apply (region_mask when update_in_region else grounded_ice_mask,
 * MCMC.py:1287-1290, :1323-1328, :1349-1352).  mc_mask: 1 where the residual enters the loss
 * (mc_region_mask, MCMC.py:1041).  The arrays are copied; the caller may free them afterwards.
 * Replaces: chain.__init__ / set_update_region / set_loss_type / set_crf_data_weight state
 * (MCMC.py:808-848, :849-872, :950-1018, :1124-1134). */
int gsm_set_static(gsm_handle h, const double* surf, const double* velx, const double* vely,
                   const double* dhdt, const double* smb, const double* crf_weight,
                   const uint8_t* update_mask, const uint8_t* mc_mask,
                   double resolution, double sigma_mc, void* stream);

/* Proposal block table: n_sizes (bh, bw) pairs [host] and their edge masks packed back to back [dev],
 * mask i starting at mask_offsets[i] doubles [host, n_sizes entries].  Masks are needed only by the
 * Philox proposal generator; replay mode receives fields that already carry the mask.
 * Every bh and bw must be even and >= 2 (RandField.get_block_sizes makes them so, MCMC.py:576-579) and at most the grid's
 * size, else GSM_E_ARG: the proposal kernels' DFT stages exist for even lengths only.
 * A new table drops the factors registered with gsm_set_factors (they belong to the old one): call it again.
 * Replaces: RandField.set_block_sizes / set_weight_param (MCMC.py:524-566, :568-623). */
int gsm_set_blocks(gsm_handle h, int32_t n_sizes, const int32_t* bh, const int32_t* bw,
                   const double* edge_masks_packed, const int64_t* mask_offsets, void* stream);

/* Cells (flat index row*W+col) [dev] from which Philox mode draws block centres uniformly --
 * the cells with region_mask==1; same distribution as the rejection loop of MCMC.py:1253-1261. */
int gsm_set_centres(gsm_handle h, const int32_t* cells, int32_t n_cells, void* stream);

/* Full-grid residual and loss of every chain's current bed: initialises the carried state.
 * energy   [dev, n_chains*H*W]: r^2 where the cell enters the loss (mc_mask == 1 and r not NaN: nansum
 *           semantics of MCMC.py:1041), else 0 -- the build's counterpart of the carried residual array
 *           mc_res (MCMC.py:1189, :1308-1315, :1340);
 * loss_sum [dev, n_chains*2]: compensated (hi, lo) pair with hi + lo = sum(energy);
 * loss0    [dev, n_chains] (may be NULL): sum / (2 sigma^2) = loss_cache[0].
 * Replaces: MCMC.py:1189-1195 (Topography.get_mass_conservation_residual, Topography.py:592-600,
 * and chain.loss, MCMC.py:1021-1044). */
int gsm_init_loss(gsm_handle h, const void* beds, void* energy, double* loss_sum, double* loss0, void* stream);

/* Full-grid residual of chain beds [dev, n_chains*H*W] -> residual [dev, same shape].
 * Replaces: Topography.get_mass_conservation_residual (Topography.py:592-600). */
int gsm_residual(gsm_handle h, const double* beds, double* residual, void* stream);

/* n_steps Metropolis steps per chain with caller-supplied draws ("replay" / parity mode).
 *   size_idx [dev, n_chains*n_steps]      index into the block table
 *   centre   [dev, n_chains*n_steps*2]    (row, col) block centre
 *   u        [dev, n_chains*n_steps]      uniform draw of the accept test
 *   fields   [dev]                        masked proposal fields f (bh x bw, row-major) at
 *                                         fields + (c*n_steps+s)*field_stride doubles
 * In/out state: beds, energy, resampled (uint32 counts), loss_sum.  Outputs: loss [n_chains*n_steps]
 * (loss_cache entries), accept [n_chains*n_steps] (0/1).
 * Synchronises the stream before returning (it reports out-of-range device data as GSM_E_DEVICE_DATA).
 * Replaces: the loop body of chain_crf.run, MCMC.py:1263-1360 (torch twin MCMC_gpu.py:385-494). */
int gsm_run_replay(gsm_handle h, int32_t n_steps, void* beds, void* energy, uint32_t* resampled, double* loss_sum,
                   const int32_t* size_idx, const int32_t* centre, const double* u,
                   const double* fields, int64_t field_stride,
                   double* loss, uint8_t* accept, void* stream);

/* Philox4x32-10 proposal generator: for every chain and steps step0 .. step0+n_steps-1 draws the block
 * size, the block centre, the accept uniform and one spectral-synthesis field (already multiplied by
 * its edge mask), into the same layout gsm_run_replay consumes.  rf_scalars (optional, may be NULL)
 * [dev, n_chains*n_steps*4] receives (scale, nugget, range_x, range_y).
 * Key = seeds[c] [dev, n_chains]; counters are functions of (absolute step, draw index) only, so a run
 * split into segments reproduces the unsplit run.  Block tables up to about 110 x 110 (the four coefficient planes must fit
 * 160 KiB of LDS, at most 32 output tiles of 16 x 16 per DFT stage); larger tables return GSM_E_UNSUPPORTED.  Tables beyond
 * ~80 x 80 use a wider instantiation of the proposal kernel and, in gsm_run_philox, the two-kernel pipeline.
 * Replaces: RandField.get_rfblock + spectral_synthesis_field (MCMC.py:742-778, :176-254), the centre
 * rejection loop (MCMC.py:1253-1261) and rng.random() (MCMC.py:1336). */
int gsm_propose_philox(gsm_handle h, int32_t n_steps, int64_t step0, const uint64_t* seeds,
                       const gsm_rf_params* rf, int32_t* size_idx, int32_t* centre, double* u,
                       double* fields, int64_t field_stride, double* rf_scalars, void* stream);

/* The reference's OWN random numbers on the device ('pcg64' draw mode): every chain's two numpy.random.Generator(PCG64) streams --
 * RandField.rng and the chain's generator, SURVEY.md section 8 a13 -- advanced by n_steps Metropolis steps' worth of draws in the
 * reference's call order, bit for bit what NumPy returns on the host (PCG64 XSL-RR, the 32-bit half cache of integers(), Lemire's
 * bounded integers, uniform, the 256-layer ziggurat normal incl. libm's log1p in its tail: mcmc_gpu_amd/csrc/pcg64_device.h,
 * restated in oracle/pcg64_oracle.py and pinned there against NumPy itself).
 *   rf_state, chain_state [dev, n_chains*6] in/out   per generator: state lo, state hi, inc lo, inc hi, has_uint32, uinteger -- the
 *                                                   integers of numpy's bit_generator.state dict
 *   region_mask [dev, H*W] or NULL                   centre rejection of MCMC.py:1253-1258 (NULL: update_in_region False)
 * Outputs, record r = c * n_steps + s: size_idx[r] (RandField.rng.integers(0, n_sizes), MCMC.py:755), rf_scalars[4 r] = (scale / 3,
 * nugget, range_x, range_y) (MCMC.py:199-207), noise_re / noise_im / nugget_field at r * field_stride: the rng.normal planes of
 * MCMC.py:242 and :251, row-major (bh, bw) (nugget_field may be NULL when rf->nugget_max == 0: the draws are consumed, nothing is
 * stored), centre[2 r] (row, col) and u[r] (MCMC.py:1336).  Feed them to gsm_spectral_from_noise and gsm_run_replay: the chain
 * then follows the CPU reference on the same seeds -- accept masks identical, beds / losses to the 1e-12 x scale of the device's
 * inverse DFT against pocketfft -- without any host draw.  Asynchronous on `stream`.
 * Replaces: the numpy.random calls of RandField.get_rfblock / spectral_synthesis_field / chain_crf.run listed above. */
int gsm_draw_pcg64(gsm_handle h, int32_t n_steps, const gsm_rf_params* rf, uint64_t* rf_state, uint64_t* chain_state,
                   const uint8_t* region_mask, int32_t* size_idx, int32_t* centre, double* u, double* rf_scalars,
                   double* noise_re, double* noise_im, double* nugget_field, int64_t field_stride, void* stream);

/* The 'pcg64' draw mode with synthesis and step in ONE launch: per (chain, step) record r = c * n_steps + s of gsm_draw_pcg64's
 * outputs, the proposal field is formed from the white-noise planes exactly as gsm_spectral_from_noise forms it (the same stage
 * functions, bit-identical fields) and consumed by the Metropolis step exactly as gsm_run_replay consumes it, inside the
 * workgroup that owns the chain -- the field never goes to HBM (chain_strip_kernel.hip, two chains per CU).  Results equal
 * gsm_spectral_from_noise + gsm_run_replay on the same handle bit for bit (tests/test_gpu_pcg64.py).  Needs a block table that
 * goes to the strip kernels (gsm_strip_active), else GSM_E_UNSUPPORTED.  nugget_field may be NULL (no nugget term).  Checks the
 * size indices and centres on the device (GSM_E_DEVICE_DATA).  Synchronises `stream` before returning (error flag).
 * Replaces: RandField.get_rfblock + spectral_synthesis_field + the loop body of chain_crf.run (MCMC.py:742-778, :176-254,
 * :1247-1360) for draws that are the reference's own. */
int gsm_run_noise(gsm_handle h, int32_t n_steps, void* beds, void* energy, uint32_t* resampled, double* loss_sum,
                  const int32_t* size_idx, const int32_t* centre, const double* u, const double* rf_scalars,
                  const gsm_rf_params* rf, const double* noise_re, const double* noise_im, const double* nugget_field,
                  int64_t field_stride, double* loss, uint8_t* accept, void* stream);

/* The spectral synthesis alone, fed with CALLER-SUPPLIED white noise instead of Philox draws: the value pin of the device
 * arithmetic against the reference's.  For field r of n_fields:
 *   size_idx   [dev, n_fields]                 block-table index -> shape (bh, bw)
 *   rf_scalars [dev, n_fields*4]               (scale, nugget, range_x, range_y): `scale` is the value multiplied in at
 *                                              MCMC.py:251 (already / 3), ranges as drawn at MCMC.py:204-207
 *   noise_re, noise_im [dev]                   the two rng.normal(size=(bh, bw)) planes of MCMC.py:242, row-major at
 *                                              r*field_stride doubles
 *   nugget_field [dev] (may be NULL)           rng.normal(0, sqrt(nug), size=(bh, bw)) of MCMC.py:251, same layout
 * The library forms the Hermitian half Zh[k] = sqrt(S(k)) ((N1[k] + N1[-k])/2 + i (N2[k] - N2[-k])/2) -- Re(ifft2(Z)) is
 * the inverse DFT of the Hermitian part of Z -- and then runs EXACTLY the code of gsm_propose_philox / the fused kernel
 * on it: spectral amplitude, folded matrix-core inverse DFT, standardisation, scale, nugget, edge mask (MCMC.py:221-251,
 * :778).  fields [dev] receives f * edge_mask at r*field_stride.
 * Replaces: spectral_synthesis_field (MCMC.py:176-254) for given draws. */
int gsm_spectral_from_noise(gsm_handle h, int32_t n_fields, const int32_t* size_idx, const double* rf_scalars,
                            const gsm_rf_params* rf, const double* noise_re, const double* noise_im,
                            const double* nugget_field, double* fields, int64_t field_stride, void* stream);

/* Philox mode end to end.  Spectral generator: the fused chain kernel (per chain-step the proposal is generated and
 * consumed inside one workgroup; nothing but chain state touches HBM), launched once per segment of at most 4096 steps
 * (scratch: one 140-byte scalar record per chain and step of a SEGMENT; `batch` is not used).  Cholesky generator, block
 * tables beyond the fused kernel's LDS budget, or gsm_set_option(h, GSM_OPT_FUSED, 0): batches of `batch` steps, proposals of
 * batch k+1 generated on a second stream while batch k is stepped, scratch owned by the handle.
 * Both forms give bit-identical results, whatever the segment / batch size.  Outputs as gsm_run_replay plus blocks
 * [dev, n_chains*n_steps*4] = (row, col, bh, bw) (blocks_cache, MCMC.py:1264).  Synchronises the stream before returning.
 * Replaces: chain_crf.run for a whole shard of chains (MCMC.py:1137-1443) as called from
 * lsc_run_wrapper (largeScaleChain_multiprocessing_GPU.py:194-201). */
int gsm_run_philox(gsm_handle h, int32_t n_steps, int64_t step0, int32_t batch, const uint64_t* seeds,
                   const gsm_rf_params* rf, void* beds, void* energy, uint32_t* resampled, double* loss_sum,
                   double* loss, uint8_t* accept, int32_t* blocks, void* stream);

/* Which kernels the calls that follow on this handle run.  Every setting computes the same chain (bit for bit, or to the bound
 * its test states); the options exist for A/B measurements and because a test uses each selected path as the reference of another.
 *   GSM_OPT_FUSED          0 / 1, default 1   gsm_run_philox, spectral generator: 1 = fused chain kernel, 0 = two-kernel pipeline
 *   GSM_OPT_STRIP          0 / 1, default 1   0 = never the strip kernels on this handle (gsm_strip_active)
 *   GSM_OPT_SPLIT2         0 / 1, default 1   0 = direct sums in stage 2 of the proposal DFT instead of the sums split by the parity
 *                                             of kx; has an effect on handles that run the strip kernels only
 *   GSM_OPT_FUSED_SEGMENT  >= 1, default 4096 steps per launch of the fused chain kernel
 * May be set at any time between calls and takes effect at the next call.  GSM_E_ARG for a NULL handle, an unknown option or
 * a value outside its range (nothing changes then). */
enum { GSM_OPT_FUSED = 0, GSM_OPT_STRIP = 1, GSM_OPT_SPLIT2 = 2, GSM_OPT_FUSED_SEGMENT = 3 };
int gsm_set_option(gsm_handle h, int32_t which, int32_t value);
/* Which form the last gsm_run_philox call on this handle ran: 1 = fused chain kernel, 0 = the two-kernel pipeline. */
int gsm_last_run_fused(gsm_handle h);
/* Which step kernels this handle's static fields, block table and GSM_OPT_STRIP select (one decision for gsm_run_replay and
 * gsm_run_philox alike, so that fused == propose + replay holds bit for bit): 1 = the strip kernels (chain_strip_kernel.hip:
 * 512-thread workgroups, two chains per CU, candidate bed in a (bh + 2) x (bw + 2) LDS tile), 0 = the flux-tile kernels
 * (1024-thread workgroups, one chain per CU: grids whose packed static operands, 48 bytes per cell, exceed an XCD's 4 MiB L2
 * -- more than 87 381 cells --, block tables whose strips would exceed 16 rows or whose proposal work area exceeds 80 KiB,
 * GSM_OPT_STRIP = 0).  Needs gsm_set_static and gsm_set_blocks.  Same arithmetic per cell (MCMC.py:1279-1360,
 * Topography.py:592-600); the window sums of a step are taken in another order (loss within 1e-15 relative). */
int gsm_strip_active(gsm_handle h);

/* Average duration in milliseconds of the step kernel / the proposal kernel over the launches made
 * by the last gsm_run_philox call, measured with HIP events on the streams the kernels ran on
 * (0 when timing was not enabled with gsm_enable_timing(h, 1)). */
int gsm_enable_timing(gsm_handle h, int32_t on);
int gsm_last_timing(gsm_handle h, double* step_kernel_ms, int32_t* step_launches,
                    double* proposal_kernel_ms, int32_t* proposal_launches);

/* Dense covariance of the bh*bw cells of a block (cell a = i*bw + j at (x, y) = (j*res, i*res)):
 * sigma[a*ld + b] = cov(|| (coord_a - coord_b) @ R ||) with R the anisotropy rotation/scaling matrix.
 * lag_table [dev, (2bh-1)*(2bw-1)] is required for GSM_VTYPE_MATERN (values from scipy.special.kv, which is what
 * covariance.py:17-22 evaluates) and optional otherwise.  sigma [dev, N*ld], ld >= N = bh*bw.
 * Replaces: gstatsim_custom._krige.make_rotation_matrix / make_sigma (_krige.py:83-122) with the covariance
 * models of gstatsim_custom/covariance.py:4-28 (incl. the spherical model's `sill - 1` beyond the range). */
int gsm_cov_assemble(gsm_handle h, int32_t bh, int32_t bw, double resolution, const gsm_vario* vario,
                     const double* lag_table, double* sigma, int64_t ld, void* stream);

/* In-place Cholesky factorisation, upper form: on entry a [dev, n*ld] holds a symmetric positive-definite matrix
 * (only its upper triangle is read), on exit its upper triangle holds U with U^T U = A + jitter*I and the strict lower
 * triangle is zero.  n must be a multiple of 64 (pad with an identity block).  Setup-time helper of the Cholesky
 * proposal generator (blocked right-looking, panel updates on the fp64 matrix cores); synchronises the stream.
 * GSM_E_ARG with the failing pivot in gsm_last_error when the matrix is not positive definite. */
int gsm_cholesky_upper(gsm_handle h, double* a, int32_t n, int64_t ld, double jitter, void* stream);

/* Precomputed factors of the Cholesky proposal generator: for block size i and range class r,
 * factors[i*n_classes + r] [host array of dev pointers] is U = chol(Sigma + jitter I)^T, upper triangular,
 * row-major [Npad][Npad] with Npad = N rounded up to 64 and zero padding.  The matrices stay caller-owned.
 * Call after gsm_set_blocks, and again after every later gsm_set_blocks (GSM_E_STATE from the generator otherwise).
 * n_sizes * n_classes <= 4096, else GSM_E_UNSUPPORTED.
 * With rf->generator == GSM_GEN_CHOLESKY, gsm_propose_philox / gsm_run_philox draw f = scale * (L z) * edge_mask
 * (z ~ N(0, I) from Philox, size and range class uniform) instead of the spectral field.
 * The reference has no such generator (README.md:21-23 lists it as future work); this is north_star's. */
int gsm_set_factors(gsm_handle h, int32_t n_classes, const double* const* factors, void* stream);

/* ---- small-scale chain (chain_sgs, gstatsMCMC/MCMC.py:1445-1911) ------------------------------------------------------
 * Sequential Gaussian simulation of one block per chain with ordinary kriging on octant-searched neighbours.
 *   grids    [dev, n_chains*H*W] in/out  the conditioning grid of each chain (`bed_tosim`, MCMC.py:1766-1771): values
 *                                       everywhere except NaN at the cells to simulate; on return the block's cells hold
 *                                       the simulated values (`newsim`, MCMC.py:1774)
 *   zcond    [dev, H*W] or NULL         if given, the block's cells are first set from it (the conditioning data of the
 *                                       block, NaN where there is none: z_cond_bed, MCMC.py:1771)
 *   windows  [dev, n_chains*4]          (row0, row1, col0, col1) of each chain's block; at most 1024 cells
 *   x_axis [dev, W], y_axis [dev, H]    coordinates of the columns / rows (the grid must be axis-aligned: xx[i][j] = x_axis[j])
 *   lag_cov  [dev, (2 lag_mi + 1) * (2 lag_mj + 1)]  covariance at the integer lag (di, dj), |di| <= lag_mi, |dj| <= lag_mj,
 *                                       row-major: the caller evaluates the variogram model (covariance.py:4-28 through
 *                                       make_sigma / make_rho, _krige.py:105-143) once per lag.  Two chosen neighbours are at
 *                                       most 2 hw apart: lag_mi >= min(2 hw, H - 1), lag_mj >= min(2 hw, W - 1); the whole grid
 *                                       (H - 1, W - 1) if the radius-widening fallback is to work
 *   hw                                  search half-width in cells: ceil(radius / |x_axis[1] - x_axis[0]|), the half-width of the
 *                                       reference's circle stencil (neighbors.py:66-83) -- any value >= 1 (the reference's driver:
 *                                       30 km at 500 m = 60).  The ring-by-ring search certifies a sector as complete from
 *                                       per-ring counters kept for the first 64 rings; beyond ring 64 (hw > 64 with sparse data) a
 *                                       sector completes only when its candidates are exhausted -- same result, more passes
 *   cell_off [dev, n_chains+1], cells [dev, total*2]   the (row, col) of each chain's cells in simulation order -- the
 *                                       caller's rng.shuffle (MCMC.py:128); every cell must lie inside the chain's window
 *   z        [dev, total]               one standard normal per listed cell (used only if the cell is simulated):
 *                                       rng.normal(est, sqrt(var)) = est + sqrt(var) * z (MCMC.py:165)
 *   max_cells                           upper bound of a chain's cell count (<= 1024): stride of the library's scratch records
 *   trace    [dev, total*3] or NULL     (number of neighbours, kriging estimate, kriging variance) per cell; -1 neighbours =
 *                                       cell was conditioned already
 *   nbr_trace [dev, total*48] or NULL   the chosen neighbours of every simulated cell (flat index row * W + col, sector by
 *                                       sector, ascending distance; -1 padded)
 * num_points in [8, 48] (num_points / 8 per octant; equidistant candidates in ascending (row, col): numpy.argsort(kind='stable')
 * of the reference's masked array -- the reference's default argsort is unstable, its choice there is implementation-defined).
 * A cell with no value within `radius` widens the search by 100 km steps like the reference (MCMC.py:150-156).
 * The kriging systems are solved by Gauss-Jordan elimination on the diagonal (the covariance block is symmetric positive
 * definite) where the reference calls numpy.linalg.lstsq (_krige.py:37), so not bit for bit.  Measured against the solution of
 * the same fp64 system in extended precision (tests/test_gpu_krige_exact.py; n = 1 .. 48 neighbours, condition numbers 1 .. 1e12,
 * ordinary and simple kriging): estimate and variance are within 0.36 of (n + 3) * 2^-53 * cond * ||w||_1 * max|value| and
 * (n + 3) * 2^-53 * cond * sill * (1 + ||w||_1) in every kernel, as is a NumPy fp64 elimination in the same order; lstsq itself is
 * up to 3 x such a bound away from that solution.  lstsq(rcond=None) truncates singular values below eps * N * s_max; here a pivot below eps * N * max|diag|
 * ends the call with GSM_E_DEVICE_DATA ("singular kriging system") instead -- tested range: tests/test_gpu_sgs.py.
 * Ordinary kriging unless gsm_sgs_set_kriging selected simple kriging (sk_solve; chain_sgs.run itself never passes ktype,
 * MCMC.py:1599, :160-161).
 * Synchronises the stream.
 * Replaces: sgs (MCMC.py:91-173), neighbors (gstatsim_custom/neighbors.py:4-64), ok_solve (gstatsim_custom/_krige.py:5-44). */
int gsm_sgs_blocks(gsm_handle h, double* grids, const double* zcond, const int32_t* windows, const double* x_axis,
                   const double* y_axis, const double* lag_cov, int32_t lag_mi, int32_t lag_mj, int32_t hw, double radius,
                   int32_t num_points, double sill, const int32_t* cell_off, const int32_t* cells, const double* z,
                   int32_t max_cells, double* trace, int32_t* nbr_trace, void* stream);

/* gsm_sgs_blocks for batches of iterations: no trace, the chain's cells are cells[cell_off[c] .. cell_off[c] + cell_cnt[c])
 * when cell_cnt is given (else .. cell_off[c + 1]), and NO synchronisation: device-side errors accumulate in the handle and
 * are reported by gsm_sgs_check. */
int gsm_sgs_blocks_batch(gsm_handle h, double* grids, const double* zcond, const int32_t* windows, const double* x_axis,
                         const double* y_axis, const double* lag_cov, int32_t lag_mi, int32_t lag_mj, int32_t hw, double radius,
                         int32_t num_points, double sill, const int32_t* cell_off, const int32_t* cell_cnt, const int32_t* cells,
                         const double* z, int32_t max_cells, void* stream);
/* Synchronises the stream and reports what gsm_sgs_blocks_batch calls since the last check have flagged (GSM_OK if nothing). */
int gsm_sgs_check(gsm_handle h, void* stream);

/* Philox mode of the small-scale chain: the draws of n_iters iterations of every chain on the device -- what chain_sgs.run takes
 * from chain.rng per iteration (MCMC.py:1750-1765 block centre with rejection on region_mask and block sizes, :128 the visiting
 * order, :165 one normal per simulated cell, :1797 the accept uniform), from Philox4x32-10 counters (draw index, stream 4,
 * iteration), key = seeds[c]:
 *   draws 0..63: centre attempts (row = mulhi(x, H), col = mulhi(y, W)), the first with region_mask == 1 (any if NULL) is taken;
 *   draw 64: block sizes bs_x = min_x + mulhi(x, max_x - min_x), bs_y likewise (numpy's integers(low, high): high excluded), accept
 *   uniform from (z, w); draws 128 + p: visiting key of window cell p (row-major) -- cells are visited in ascending (key, p);
 *   draws 2048 + p / 2: the standard normal of cell p (first / second Box-Muller value for even / odd p).
 * Outputs, [dev], record r = j * n_chains + c for iteration iter0 + j: windows[4 r] (r0, r1, c0, c1 as MCMC.py:1758-1761),
 * blocks[4 r] (row, col, bs_x, bs_y), cell_cnt[r], cell_off[r] = r * max_cells, cells[2 (r max_cells + k)] the k-th visited cell,
 * z[r max_cells + k] its normal (0 for a conditioning cell: is_data != 0), u[r].  max_cells >= (max_x - 1) * (max_y - 1) windows fit.
 * oracle/sgs_philox_oracle.py restates it. */
int gsm_sgs_draw_philox(gsm_handle h, const uint64_t* seeds, int64_t iter0, int32_t n_iters, const uint8_t* region_mask,
                        const uint8_t* is_data, int32_t min_x, int32_t max_x, int32_t min_y, int32_t max_y, int32_t max_cells,
                        int32_t* windows, int32_t* blocks, int32_t* cell_off, int32_t* cell_cnt, int32_t* cells, double* z, double* u,
                        void* stream);

/* gsm_sgs_draw_philox's outputs from the chains' OWN NumPy generators ('pcg64' draw mode of the small-scale chain): chain_state
 * [dev, n_chains*6] (state lo, hi, inc lo, hi, has_uint32, uinteger of numpy's PCG64 bit_generator.state; in/out) is advanced by
 * n_iters iterations' worth of draws in chain_sgs.run's order -- integers(0, H), integers(0, W) until region_mask == 1 and
 * integers(min_x, max_x), integers(min_y, max_y) (MCMC.py:1750-1757), rng.shuffle of the block's (row, col) list (:128: Fisher-Yates
 * from the back, random_interval's masked rejection on 32-bit words), one rng.normal per cell without conditioning data in
 * visiting order (:165), rng.random() (:1797) -- bit for bit what NumPy returns (mcmc_gpu_amd/csrc/pcg64_device.h).  Record
 * r = j * n_chains + c for the j-th iteration; layouts as in gsm_sgs_draw_philox.  Asynchronous; device-side errors are reported
 * by gsm_sgs_check. */
int gsm_sgs_draw_pcg64(gsm_handle h, uint64_t* chain_state, int32_t n_iters, const uint8_t* region_mask, const uint8_t* is_data,
                       int32_t min_x, int32_t max_x, int32_t min_y, int32_t max_y, int32_t max_cells, int32_t* windows,
                       int32_t* blocks, int32_t* cell_off, int32_t* cell_cnt, int32_t* cells, double* z, double* u, void* stream);

/* Loss and thickness guard of proposed beds over the whole grid: loss[c] = nansum(residual(bed_c + trend)^2 where
 * mc_mask == 1) / (2 sigma^2), bad[c] = number of cells with update_mask == 1 (set it to grounded_ice_mask) and
 * surf - (bed_c + trend) <= 0.  beds [dev, n_chains*H*W], trend [dev, H*W] or NULL, loss [dev, n_chains], bad [dev, n_chains].
 * Replaces: chain_sgs.run's per-iteration loss and guard (MCMC.py:1781-1795). */
int gsm_sgs_loss(gsm_handle h, const double* beds, const double* trend, double* loss, int32_t* bad, void* stream);

/* The Metropolis decision of one small-scale iteration on the device, so that a batch of iterations needs no host round
 * trip: loss_next[c] (set to +inf where bad[c] > 0), p = 1 if loss_prev[c] > loss_next[c] else min(1, exp(loss_prev[c] -
 * loss_next[c])) (a NaN exponential -- a NaN loss, or inf - inf -- gives p = 1 as the reference's built-in min(1, nan) does,
 * and as the large-scale step's fmin), accept[c] = u[c] <= p; an accepted chain's loss_prev[c]
 * becomes loss_next[c].  loss_rec[c * rec_stride] = loss_prev[c] after the decision and acc_rec[c * rec_stride] =
 * accept[c] (the iteration's column of the caller's [n_chains][rec_stride] record arrays; either may be NULL).  All [dev].
 * Replaces: chain_sgs.run's acceptance test (MCMC.py:1797-1812). */
int gsm_sgs_decide(gsm_handle h, const double* loss_next, const int32_t* bad, const double* u, double* loss_prev,
                   uint8_t* accept, double* loss_rec, uint8_t* acc_rec, int64_t rec_stride, void* stream);

/* Windowed end of a small-scale iteration for chains WITHOUT a normal-score transformer.  The reference recomputes residual, loss
 * and thickness guard over the whole map every iteration (MCMC.py:1781-1795); without a transformer only the block differs from the
 * current bed, so only the residuals of the block and its one-cell halo change.  Carried per chain: `energy` [dev, n_chains*H*W]
 * (squared residual where mc_mask == 1 and the residual is not NaN, else 0 -- as the large-scale step kernels carry it) and
 * state [dev, n_chains*4] = (sum of energy: hi, lo of a compensated pair; loss = sum / (2 sigma^2); number of cells with
 * update_mask == 1 -- set it to grounded_ice_mask -- and surf - (bed + trend) <= 0).
 * gsm_sgs_state_init fills both from the current beds (trend [dev, H*W] or NULL).
 * gsm_sgs_finish: loss and guard of the proposal `next` (== `cur` outside windows[c]) from the halo window, the acceptance test of
 * gsm_sgs_decide with u[c], then gsm_sgs_commit's bookkeeping (cur / next / resampled) and the update of energy / state of an
 * accepted chain.  accept [dev, n_chains]; loss_rec / acc_rec / rec_stride as in gsm_sgs_decide.  The loss equals the full-grid
 * nansum up to summation order (<= 1e-12 relative).  A window whose halo exceeds 36 x 36 cells is reported by gsm_sgs_check.
 * Replaces: chain_sgs.run's per-iteration loss, guard, acceptance test and commit (MCMC.py:1781-1812) when do_transform is False. */
int gsm_sgs_state_init(gsm_handle h, const double* beds, const double* trend, double* energy, double* state, void* stream);
int gsm_sgs_finish(gsm_handle h, double* cur, double* next, const double* trend, double* energy, double* state,
                   const int32_t* windows, const double* u, uint32_t* resampled, uint8_t* accept, double* loss_rec,
                   uint8_t* acc_rec, int64_t rec_stride, void* stream);

/* scikit-learn's QuantileTransformer(output_distribution="normal") of one feature on the device, as chain_sgs.run applies it
 * to the whole map around every SGS block (MCMC.py:1766, :1777): out[i] = transform(x[i]) (inverse == 0) or
 * inverse_transform(x[i]) (inverse != 0), i < n.  quantiles = transformer.quantiles_[:, 0], references =
 * transformer.references_, both [dev, nq] ascending; x, out [dev, n] (may alias).  NaN stays NaN.  Same arithmetic as
 * QuantileTransformer._transform_col with scipy.stats.norm.ppf / cdf (Cephes ndtri / ndtr): mcmc_gpu_amd/csrc/normal_score.h. */
int gsm_qt_transform(gsm_handle h, const double* quantiles, const double* references, int32_t nq, const double* x, double* out,
                     int64_t n, int32_t inverse, void* stream);

/* gsm_sgs_commit for a chain with a normal-score transformer: the inverse transform touches every cell of the proposed map,
 * so an accepted chain takes the WHOLE plane of `proposed` (cur[c] = proposed[c]) and the resampled counts of its window are
 * incremented (MCMC.py:1803-1812); a rejected chain keeps cur.  cur, proposed [dev, n_chains*H*W]. */
int gsm_sgs_commit_map(gsm_handle h, double* cur, const double* proposed, uint32_t* resampled, const int32_t* windows,
                       const uint8_t* accept, void* stream);

/* Accept / reject bookkeeping of one small-scale iteration: where accept[c] != 0 the block of chain c is copied from
 * `next` into `cur` and resampled counts of the block are incremented (MCMC.py:1803-1812); elsewhere the block of `next`
 * is restored from `cur`.  cur, next [dev, n_chains*H*W], resampled [dev, n_chains*H*W], windows as in gsm_sgs_blocks,
 * accept [dev, n_chains]. */
int gsm_sgs_commit(gsm_handle h, double* cur, double* next, uint32_t* resampled, const int32_t* windows,
                   const uint8_t* accept, void* stream);

/* Chain groups of the small-scale chain: chains that continue DIFFERENT large-scale beds in one handle.  The reference's driver
 * derives the trend, the normal-score transformer and the transformed conditioning data from the large-scale bed it starts from
 * (smallScaleChain_multiprocessing.py:479-496), so they belong to the bed, not to the problem.  group [HOST, n_chains]: the group of
 * every chain, each in [0, n_groups) (GSM_E_ARG otherwise; nothing changes then); the values are copied.  While groups are set, these
 * arguments hold one plane or table per GROUP and chain c reads the one of group[c]:
 *   trend                      [dev, n_groups*H*W]   gsm_sgs_loss, gsm_sgs_state_init, gsm_sgs_finish, gsm_sgs_iterate (batch->trend)
 *   zcond                      [dev, n_groups*H*W]   gsm_sgs_blocks, gsm_sgs_blocks_batch, gsm_sgs_iterate (batch->zcond)
 *   quantiles, references      [dev, n_groups*nq]    gsm_qt_transform, gsm_sgs_iterate (batch->qt_quantiles, batch->qt_references; one nq)
 * (NULL keeps its meaning).  gsm_qt_transform then takes whole maps of all chains only: n == n_chains * H * W, anything else is
 * GSM_E_ARG (and at most 65535 chains).  Every result of chain c equals, bit for bit, the result of the same call on a handle that
 * holds only the chains of group[c] and is given that group's plane and tables.  gsm_sgs_batch keeps its layout: the groups live in
 * the handle.  group == NULL or n_groups == 1 removes the groups; with none set every entry point runs the kernels it ran before
 * groups existed, on the caller's pointers.  Waits for the device (the table may be in use).  Groups of a handle whose chains do
 * not all share one variogram are out of scope: the reference asks for one consistent V1_p.
 * Replaces: one process per large-scale bed in smallScaleChain_multiprocessing.py (:479-496 run once per bed). */
int gsm_sgs_set_groups(gsm_handle h, const int32_t* group, int32_t n_groups);

/* Kriging type of the gsm_sgs_blocks* calls that follow on this handle.  GSM_KRIGING_ORDINARY (the default; what
 * chain_sgs.run uses, MCMC.py:1774 passes no ktype): ok_solve, the (n+1) x (n+1) system with the Lagrange row, estimate around
 * the LOCAL mean of the neighbours (_krige.py:5-44).  GSM_KRIGING_SIMPLE: sk_solve, Sigma w = rho, estimate
 * global_mean + sum w (v - global_mean) (_krige.py:46-81); global_mean [dev, n_chains] = the mean of each chain's conditioning
 * values BEFORE the call (MCMC.py:81, np.mean(out_grid[cond_msk])), read when the blocks are simulated.
 * Replaces: the ktype argument of MCMC.sgs (MCMC.py:91, :158-161). */
#define GSM_KRIGING_ORDINARY 0
#define GSM_KRIGING_SIMPLE 1
int gsm_sgs_set_kriging(gsm_handle h, int32_t ktype, const double* global_mean);

/* ---- interpolate.sgs on whole grids (gstatsim_custom/interpolate.py:92-191) --------------------------------------------
 * Sequential Gaussian simulation of n_chains = R whole-grid realisations on one handle, in normal-score space.
 *   grids    [dev, R*H*W] in/out        normal scores: the conditioning values, NaN at every cell without one; on return
 *                                       every path cell holds its simulated value (NaN cells off the paths stay NaN)
 *   path     [dev, total]               flat cell indices (row * W + col) in visiting order -- the caller's rng.shuffle of
 *                                       the cells of sim_mask (interpolate.py:127) without the cells that hold a value;
 *                                       realisation r's path is path[path_off[r] .. path_off[r + 1])
 *   path_off [dev, R + 1]               int64 offsets; max_path >= the longest path
 *   draws    [dev, total]               one number per path cell: draw_kind GSM_DRAW_NORMAL, a standard normal,
 *                                       rng.normal(est, sqrt(var), 1) = est + sqrt(var) * z (interpolate.py:174);
 *                                       GSM_DRAW_TRUNCATED, a uniform u (rng.random()): truncnorm.rvs(a, b, loc=est,
 *                                       scale=sqrt(var)) = truncnorm.ppf(u, a, b) * scale + est with a, b = (lower - est) /
 *                                       scale, (upper - est) / scale (interpolate.py:176-187; scipy 1.15's truncnorm has
 *                                       no _rvs of its own).  Unused at cells whose bounds coincide
 *   lower, upper [dev, H*W] or NULL     transformed bounds (GSM_DRAW_TRUNCATED only): a cell with lower == upper takes
 *                                       lower and solves no system (interpolate.py:181-182)
 *   x_axis, y_axis, lag_cov, lag_mi, lag_mj, hw, radius, num_points, sill   as in gsm_sgs_blocks.  The search widens by
 *                                       100 km steps (interpolate.py:150-157): lag_mi / lag_mj must cover 2 ceil(r / |dx|)
 *                                       for the widest radius r any visit reaches (or H - 1 / W - 1)
 *   seg_cells                           path slots whose records (800 bytes each per realisation) are resident at once,
 *                                       rounded up to a multiple of 64; the result does not depend on it
 *   trace    [dev, total*3] or NULL     (number of neighbours, kriging estimate, kriging variance) per path cell; -1
 *                                       neighbours where no system was solved (bounds coincide)
 * Kriging type and, for simple kriging, the global mean of each realisation [dev, R] from gsm_sgs_set_kriging.
 * Neighbour sets, tie order and solve as gsm_sgs_blocks; the truncated-normal ppf restates scipy's (csrc/truncnorm.h).
 * Errors: GSM_E_ARG for H * W > 2^25 (25-bit slot / cell fields) or inconsistent arguments; GSM_E_DEVICE_DATA for a path
 * cell that holds a value or is listed twice, a cell with no value anywhere, a singular system, a lag table too small, or a
 * truncated draw outside scipy's domain (scale 0 or lower >= upper after standardising).  Synchronises the stream.
 * Replaces: interpolate.sgs (gstatsim_custom/interpolate.py:92-191), neighbors (gstatsim_custom/neighbors.py:4-64),
 * ok_solve / sk_solve (gstatsim_custom/_krige.py:5-81). */
#define GSM_DRAW_NORMAL 0
#define GSM_DRAW_TRUNCATED 1
int gsm_sgs_grid(gsm_handle h, double* grids, const int32_t* path, const int64_t* path_off, int32_t max_path,
                 const double* draws, const double* lower, const double* upper, int32_t draw_kind, const double* x_axis,
                 const double* y_axis, const double* lag_cov, int32_t lag_mi, int32_t lag_mj, int32_t hw, double radius,
                 int32_t num_points, double sill, int32_t seg_cells, double* trace, void* stream);

/* ---- interpolate.krige on a whole grid (gstatsim_custom/interpolate.py:13-89) -------------------------------------------
 * The kriging estimate and its variance at n_cells cells of ONE grid, in normal-score space, on a handle created with
 * n_chains = 1.  Kriging is gsm_sgs_grid without the sequence: the reference never adds an estimated cell to its conditioning
 * mask, so every cell conditions on the measured values alone and all cells are solved side by side (one wavefront each).
 *   grid     [dev, H*W]                 normal scores: the conditioning values, NaN at every cell without one; not written
 *   cells    [dev, n_cells]             flat indices (row * W + col) of the cells to estimate -- the cells of sim_mask that
 *                                       hold no value, in any order (the reference visits them in C order); each must be NaN
 *                                       in `grid`.  n_cells = 0 is a no-op
 *   x_axis, y_axis, lag_cov, lag_mi, lag_mj, hw, radius, num_points, sill   as in gsm_sgs_grid.  A cell with no value within
 *                                       `radius` widens the search by 100 km steps (interpolate.py:65-71): lag_mi / lag_mj must
 *                                       cover 2 ceil(r / |dx|) for the widest radius r any cell reaches (or H - 1 / W - 1)
 *   est      [dev, n_cells]             kriging estimate of cells[k] at k: sum w v + (1 - sum w) * m, m the mean of the
 *                                       neighbours' values (ordinary, _krige.py:42) or the global mean (simple, _krige.py:79)
 *   var      [dev, n_cells]             sill - sum w rho, SIGNED (_krige.py:41, :78): the reference clips negative values to
 *                                       zero afterwards (interpolate.py:83), and so does the caller
 *   n_neighbours [dev, n_cells]         size of the solved system (1 .. num_points)
 * Kriging type and, for simple kriging, the global mean [dev, 1] from gsm_sgs_set_kriging.  Neighbour sets, tie order
 * (ascending (distance, row, column)) and solve as gsm_sgs_blocks.
 * Limits: 8 <= num_points <= 48, H and W in [2, 32767], hw >= 1 (GSM_E_ARG / GSM_E_UNSUPPORTED as in gsm_sgs_grid).
 * Errors found on the device, GSM_E_DEVICE_DATA with one text per cause: a listed cell outside the grid or holding a value; no
 * value anywhere on the grid; a lag table too small ("lag covariance table"); a singular system.  Such a cell gets est = var =
 * NaN and n_neighbours = 0; every other cell of the call is still completed.  Synchronises the stream.
 * Replaces: interpolate.krige (gstatsim_custom/interpolate.py:13-89), neighbors (gstatsim_custom/neighbors.py:4-64),
 * ok_solve / sk_solve (gstatsim_custom/_krige.py:5-81). */
int gsm_krige_grid(gsm_handle h, const double* grid, const int32_t* cells, int32_t n_cells,
                   const double* x_axis, const double* y_axis, const double* lag_cov, int32_t lag_mi, int32_t lag_mj,
                   int32_t hw, double radius, int32_t num_points, double sill,
                   double* est, double* var, int32_t* n_neighbours, void* stream);

/* ---- a variogram per cell: non-stationary interpolate.sgs / interpolate.krige ------------------------------------------------
 * The reference takes every variogram parameter as a number or as a map of the grid's shape and builds a local_vario for each
 * visited cell (interpolate.py:56-62, :141-147, scalars broadcast by _preprocess :226-231): the kriging system of cell (i, j) is
 * assembled from the parameters AT (i, j), whatever its neighbours' own parameters are.  gsm_sgs_grid_local / gsm_krige_grid_local
 * are gsm_sgs_grid / gsm_krige_grid with `lag_cov, lag_mi, lag_mj, sill` replaced by
 *   local    [dev, H*W*6]               per cell R00, R01, R10, R11, sill, nugget: R = make_rotation_matrix(azimuth, major_range,
 *                                       minor_range) (_krige.py:83-103), computed by the caller.  Rows of cells that are never
 *                                       visited may hold NaN
 *   vtype                               GSM_VTYPE_EXPONENTIAL, GSM_VTYPE_GAUSSIAN or GSM_VTYPE_SPHERICAL (covariance.py:4-15);
 *                                       anything else (GSM_VTYPE_MATERN: no Bessel K on the device) is GSM_E_UNSUPPORTED
 * No covariance table exists when every cell has its own model: each covariance of a system is evaluated in the kernel from
 * the two points' coordinates (x_axis, y_axis; either may descend), dx = x_a - x_b, dy = y_a - y_b, u = dx R00 + dy R10,
 * v = dx R01 + dy R11, h = sqrt(u u + v v), C(h) the model with the cell's sill and nugget.  (The reference multiplies the
 * absolute coordinates by R and subtracts afterwards, make_sigma / make_rho, _krige.py:105-144.)  The kriging variance is the
 * cell's sill - sum w rho.  Every other argument, the search, the solve, the records, errors and limits are those of the table
 * functions; the "lag covariance table" error cannot occur.
 * Replaces: the local_vario of interpolate.krige and interpolate.sgs (gstatsim_custom/interpolate.py:56-62, :141-147),
 * make_rotation_matrix's use, make_sigma, make_rho (gstatsim_custom/_krige.py:105-144), the covariance models
 * (gstatsim_custom/covariance.py:4-15). */
int gsm_sgs_grid_local(gsm_handle h, double* grids, const int32_t* path, const int64_t* path_off, int32_t max_path,
                       const double* draws, const double* lower, const double* upper, int32_t draw_kind, const double* x_axis,
                       const double* y_axis, const double* local, int32_t vtype, int32_t hw, double radius,
                       int32_t num_points, int32_t seg_cells, double* trace, void* stream);
int gsm_krige_grid_local(gsm_handle h, const double* grid, const int32_t* cells, int32_t n_cells,
                         const double* x_axis, const double* y_axis, const double* local, int32_t vtype,
                         int32_t hw, double radius, int32_t num_points,
                         double* est, double* var, int32_t* n_neighbours, void* stream);

/* ---- kriging cross-validation: leave-one-out, buffered and fold hold-outs (interpolate.cross_validate) ----------------------
 * Every listed DATA cell of one grid kriged from the other data under a hold-out, in normal-score space, for n_models candidate
 * variograms at once (gstat's krige.cv / GSLIB's jackknife; the reference has no such function -- search, widening and solve
 * are its krige's).  gsm_krige_grid with three differences.
 * The target: cells[k] must HOLD a value (gsm_krige_grid: must not).
 * The hold-out: cell c conditions target t only if grid[c] is a value, c != t, and
 *   fold     [dev, H*W] int32 or NULL   not (fold[t] >= 0 and fold[c] == fold[t]): a target in a fold is estimated without
 *                                       that fold; a negative label means "in no fold" (held out only as the target itself)
 *   exclude_radius                      not (exclude_radius > 0 and d(c, t) <= exclude_radius), d = sqrt((x_t - x_c)^2 +
 *                                       (y_t - y_c)^2) as the search computes it, no fused multiply-add.  0 with fold = NULL is
 *                                       leave-one-out.  Choose it off the lattice distances (2.5 cells on a square grid)
 * What is left is searched as in gsm_krige_grid, radius widening included: the result for target t equals, bit for bit,
 * gsm_krige_grid on a copy of the grid with the held-out cells set to NaN -- one copy per fold, but one per TARGET for the
 * buffer and for leave-one-out, which is why this is a kernel.  The global mean of simple kriging (gsm_sgs_set_kriging) is
 * taken as given: the mean of all data, the target's included, as the kriging run that follows will use it.
 * The models: the neighbour set does not depend on the covariance, so each target is searched once and then solved per model.
 *   n_models                            1 .. 8
 *   lag_cov  [dev, n_models * (2 lag_mi + 1) * (2 lag_mj + 1)]  model m's table after model m - 1's, one (lag_mi, lag_mj) for all.
 *                                       Which neighbours a hold-out leaves is not known on the host: pass whole-grid tables
 *                                       (lag_mi = H - 1, lag_mj = W - 1)
 *   sill     [HOST, n_models]           sill of each model (read before the launch)
 *   est, var [dev, n_models * n_cells]  model m's results at m * n_cells + k; var SIGNED as in gsm_krige_grid
 *   n_neighbours [dev, n_cells]         size of the solved systems, the same for every model
 * gsm_krige_cv_local: n_models per-cell tables, local [dev, n_models * H*W*6], and vtype [HOST, n_models], each as in
 * gsm_krige_grid_local (GSM_VTYPE_MATERN: GSM_E_UNSUPPORTED).
 * Refused before any launch: GSM_E_ARG for a NULL pointer (fold may be NULL), n_cells outside [0, H * W], n_models outside
 * [1, 8], exclude_radius negative or NaN; num_points, hw, radius, grid sides and the handle as in gsm_krige_grid.
 * Errors found on the device, GSM_E_DEVICE_DATA with one text per cause: a listed cell outside the grid or holding no value,
 * and no value anywhere outside a target's hold-out -- est = var = NaN for every model and n_neighbours = 0 at that cell; a lag
 * table too small ("lag covariance table") and a singular system -- est = var = NaN for that (model, cell) alone.  Everything
 * else of the call is still completed.  Synchronises the stream. */
int gsm_krige_cv(gsm_handle h, const double* grid, const int32_t* cells, int32_t n_cells, const int32_t* fold,
                 double exclude_radius, const double* x_axis, const double* y_axis, int32_t n_models,
                 const double* lag_cov, int32_t lag_mi, int32_t lag_mj, int32_t hw, double radius, int32_t num_points,
                 const double* sill, double* est, double* var, int32_t* n_neighbours, void* stream);
int gsm_krige_cv_local(gsm_handle h, const double* grid, const int32_t* cells, int32_t n_cells, const int32_t* fold,
                       double exclude_radius, const double* x_axis, const double* y_axis, int32_t n_models,
                       const double* local, const int32_t* vtype, int32_t hw, double radius, int32_t num_points,
                       double* est, double* var, int32_t* n_neighbours, void* stream);

/* ---- gsm_sgs_grid's path and draws from the callers' OWN NumPy generators ('pcg64' mode of interpolate.sgs) -----------------
 * What interpolate.sgs takes from its numpy.random.Generator(PCG64), made on the device for all R = n_chains realisations side by
 * side (one wavefront each), bit for bit what NumPy returns (mcmc_gpu_amd/csrc/pcg64_device.h):
 *   states   [dev, R*6] in/out          per realisation state lo, hi, inc lo, hi, has_uint32, uinteger of bit_generator.state
 *                                       (the layout of gsm_sgs_draw_pcg64); on return where NumPy would leave the generator
 *   cells    [dev, n_cells]             flat indices (row * W + col) of the cells of sim_mask in C order: the rows of `inds`
 *                                       before the shuffle, the same for every realisation
 *   has_value [dev, H*W]                != 0 where the grid holds a conditioning value (the reference's cond_msk)
 *   lower, upper [dev, H*W] or NULL     transformed bounds, read with GSM_DRAW_TRUNCATED only
 *   work     [dev, R*n_cells]           scratch: each realisation's shuffled copy of `cells`
 *   path     [dev, R*path_len]          out: realisation r's visiting order at r * path_len -- its shuffled cells without those that
 *                                       hold a value (the cell loop skips them).  Every realisation filters the same
 *                                       cells by the same mask, so all paths have path_len cells: gsm_sgs_grid's path_off[r] =
 *                                       r * path_len, max_path = path_len
 *   draws    [dev, R*path_len]          out: gsm_sgs_grid's `draws`, one number per path cell in path order
 * In NumPy's order per realisation: rng.shuffle(inds) (interpolate.py:127; Generator.shuffle of a 2-D array: for i = n - 1 .. 1,
 * j = random_interval(i) -- masked rejection on 32-bit words, the unused half of a 64-bit draw staying cached -- and rows i and j
 * change places); then with GSM_DRAW_NORMAL one standard normal per path cell (the z of rng.normal(est, sqrt(var), 1),
 * interpolate.py:174: the 256-layer ziggurat on 64-bit draws, wedge and tail paths included), with GSM_DRAW_TRUNCATED one
 * rng.random() per path cell whose bounds differ (the uniform of truncnorm.rvs, interpolate.py:185; lower != upper as IEEE
 * compares them, so a NaN bound draws) and 0.0 at the others (interpolate.py:181-182 draws nothing there).  The 64-bit draws
 * leave the cached 32-bit word where the shuffle left it, as NumPy's next_uint64 does.  n_cells of 0 or 1 and path_len = 0 are
 * valid and consume what NumPy consumes (nothing, or the shuffle alone).
 * Errors: GSM_E_ARG, before anything is written, for a NULL pointer that is read, n_cells outside [0, H * W], path_len outside
 * [0, n_cells], GSM_DRAW_TRUNCATED without both bounds, an unknown draw_kind.  GSM_E_DEVICE_DATA when the listed cells without a
 * value are not path_len many ("path length": such a realisation makes no draw, its generator stays behind the shuffle) or a
 * listed cell lies outside the grid.  Synchronises the stream.
 * Replaces: rng.shuffle, the cond_msk filter and the per-cell draws of interpolate.sgs (gstatsim_custom/interpolate.py:127,
 * :174, :185); numpy/random/_generator.pyx Generator.shuffle, src/distributions/distributions.c random_interval,
 * random_standard_normal, next_double. */
int gsm_sgs_grid_draw_pcg64(gsm_handle h, uint64_t* states, const int32_t* cells, int32_t n_cells, const uint8_t* has_value,
                            const double* lower, const double* upper, int32_t draw_kind, int32_t* work, int32_t* path,
                            double* draws, int32_t path_len, void* stream);

/* One batch of small-scale iterations in ONE call: for j < n_iters, in the order of chain_sgs.run's loop body
 * (MCMC.py:1741-1822) -- [gsm_qt_transform cur -> next] gsm_sgs_blocks_batch [gsm_sgs_finish | gsm_qt_transform next ->
 * proposed, gsm_sgs_loss, gsm_sgs_decide, gsm_sgs_commit(_map)] -- with iteration j's draws at windows + 4*n_chains*j,
 * cell_off + cell_off_stride*j, cell_cnt + n_chains*j (or NULL), u + n_chains*j and records at loss_rec + j / acc_rec + j
 * (rec_stride = n_iters).  cell_base (HOST, n_iters entries, or NULL = 0): iteration j's cells / z start at
 * cells + 2*cell_base[j] / z + cell_base[j] (the tightly packed lists of replay mode).  Asynchronous; gsm_sgs_check reports a
 * raised device flag.
 * grid_finite != 0: the caller's promise that no cell of `cur` is NaN (it stays so: simulation fills every cell of a block).
 * A cell's neighbour set and kriging weights depend on WHERE values are, not on the values; with the promise the search reads no
 * grid value, the records name their cells, and the records of iteration j + 1 are made on a second stream of the handle while
 * iteration j runs its value pass, transforms, loss and decision (the longest kernel of an iteration leaves the critical path;
 * the value pass then reads the neighbours' values from the grid).  Same numbers as without the promise.  With NaN cells in
 * `cur` the promise is false and the neighbour sets would be wrong: leave it 0.
 * tail_qt: with a transformer, whether both transforms of an iteration run inside the launch that ends it (where its tables
 * and the map's parts fit) or as launches of their own -- same numbers.  GSM_TAIL_QT_AUTO (0, a zeroed struct): inside from 12
 * chains on, where that is faster; GSM_TAIL_QT_ON / GSM_TAIL_QT_OFF: always / never.  Anything else is GSM_E_ARG. */
enum { GSM_TAIL_QT_AUTO = 0, GSM_TAIL_QT_ON = 1, GSM_TAIL_QT_OFF = 2 };
typedef struct gsm_sgs_batch {
  double* cur; double* next; double* proposed;            /* proposed: only with a transformer */
  const double* zcond; const double* trend;               /* trend NULL: not detrended */
  const double* qt_quantiles; const double* qt_references;
  double* energy; double* state;                          /* windowed finish only */
  const double* x_axis; const double* y_axis; const double* lag_cov;
  const int32_t* windows; const int32_t* cell_off; const int32_t* cell_cnt; const int32_t* cells; const double* z;
  const int64_t* cell_base;                               /* HOST or NULL */
  const double* u;
  uint32_t* resampled; double* loss; int32_t* bad; double* loss_prev; uint8_t* accept; double* loss_rec; uint8_t* acc_rec;
  double radius, sill;
  int64_t cell_off_stride;
  int32_t qt_n, windowed, lag_mi, lag_mj, hw, num_points, max_cells;
  int32_t grid_finite;                                    /* the caller's promise: no NaN in cur (see below) */
  int32_t tail_qt;                                        /* GSM_TAIL_QT_* */
} gsm_sgs_batch;
int gsm_sgs_iterate(gsm_handle h, const gsm_sgs_batch* batch, int32_t n_iters, void* stream);

/* Setup-time distance transform: dist[i] = Euclidean distance from cell i (coordinates xx[i], yy[i]) to the nearest
 * cell with mask[i] != 0, all [dev, H*W].  Exact (brute force over the masked cells, same dx*dx + dy*dy, sqrt
 * arithmetic as the KD-tree query).  Synchronises the stream.
 * Replaces: Utilities.min_dist_from_mask (Utilities.py:21-24), used by RandField.get_crf_weight /
 * chain_crf.set_crf_data_weight (MCMC.py:689-714, :1124-1134). */
int gsm_min_dist_from_mask(gsm_handle h, const double* xx, const double* yy, const uint8_t* mask, double* dist,
                           void* stream);

/* Gaussian trend of a stack of beds: out[r] = scipy.ndimage.gaussian_filter(x[r], sigma, mode='reflect', truncate=t) for the
 * n fields x [dev, n*H*W] at once (H, W must be the handle's; n is the call's own and need not be n_chains), fp64, out [dev, n*H*W]
 * must not alias x.  Asynchronous on `stream`.
 *   w0 [HOST, 2 lw0 + 1], w1 [HOST, 2 lw1 + 1]   the weights of axis 0 (down the rows) and axis 1 (along a row), read before the
 *                                       call returns.  The caller makes them in scipy's NumPy arithmetic (_gaussian_kernel1d):
 *                                       lw = int(truncate * sigma + 0.5), x = arange(-lw, lw + 1), phi = exp(-0.5 / sigma^2 * x^2),
 *                                       w = phi / phi.sum().  The device evaluates no exponential.  0 <= lw <= 128
 * Passes as in scipy: axis 0 first, then axis 1 on its result.  Each pass, for every cell i of its axis of n cells:
 *   acc = 0;  for k = 0, 1, .. 2 lw in this order:  acc = fma(w[k], x[refl(i + k - lw)], acc)
 * one fused multiply-add per tap into one accumulator; refl is the half-sample-symmetric reflection of period 2 n
 * (d c b a | a b c d | d c b a), folded as often as it takes (n < lw, n = 1).  scipy pairs the symmetric taps instead: the two agree
 * to within the rounding of either order ((2 lw0 + 2 lw1 + 6) * 2^-53 times the filter of |x|, tests/trend_common.py), not bit for bit.
 * The order is the same for every cell and no sum is split or shared: field r of a batch has the bits of the one-field call, and
 * the same call twice gives the same bits.  No atomics.  NaN and infinities propagate by this arithmetic alone (the cells within
 * lw of a NaN along either pass).
 * Scratch: the result of the axis-0 pass, n*H*W doubles, is owned by the handle (grow-only, released by gsm_destroy; growing it
 * frees the smaller buffer, which waits for the device).
 * Errors (GSM_E_ARG, nothing launched): a NULL pointer, out == x, n < 1, H or W not the handle's, lw0 or lw1 outside [0, 128], H * W
 * above 2^30, n * H * W beyond one launch's 2^31 workgroups.
 * Replaces: trend = sp.ndimage.gaussian_filter(initial_bed, sigma=10) (smallScaleChain_multiprocessing.py:486) for every
 * large-scale bed of an ensemble at once; scipy/ndimage/_filters.py gaussian_filter, gaussian_filter1d, correlate1d. */
int gsm_gaussian_filter(gsm_handle h, const double* x, double* out, int32_t n, int32_t H, int32_t W, const double* w0, int32_t lw0,
                        const double* w1, int32_t lw1, void* stream);

/* Fit of the normal-score transformers of a stack of fields: quantiles[r] = the table quantiles_[:, 0] that
 * QuantileTransformer(n_quantiles=nq, subsample=None).fit(x[r].reshape(-1, 1)) of scikit-learn holds, for the n fields x [dev, n*cells]
 * at once, fp64, bit for bit.  n and cells are the call's own: cells need not be the handle's H*W (a caller may fit on the cells of
 * a mask), and the handle's grid may have any size.  x is only read.  Asynchronous on `stream`.
 *   q [HOST, nq]             the probabilities, read before the call returns.  The caller makes them as scikit-learn and NumPy do:
 *                            q = (np.linspace(0, 1, nq, endpoint=True) * 100) / 100 (references_ to percent and back).
 *   quantiles [dev, n*nq]    the tables
 *   n_valid, n_inf [dev, n]  int64: the values of field r that are not NaN, and those that are +inf or -inf
 *   sorted [dev, n*cells]    or NULL: the values of field r that are not NaN in ascending order, then NaN up to `cells`
 * Arithmetic, with s the ascending values of a field that are not NaN and m = n_valid[r], for every k < nq:
 *   v = (m - 1) * q[k]                                  one fp64 multiply
 *   lo = floor(v);  g = v - lo;  hi = min(lo + 1, m - 1);  a = s[lo];  b = s[hi];  d = b - a
 *   t[k] = g >= 0.5 ? b - d * (1 - g) : a + d * g       every operation rounded on its own: nothing is fused
 *   quantiles[r][k] = max(t[0..k])                      the running maximum, np.maximum.accumulate (NaN stays)
 * which is np.nanpercentile(x[r], q * 100, method='linear') with NumPy's _lerp, then scikit-learn's np.maximum.accumulate.
 * m == 0 gives a row of NaN, as NumPy does.
 * Order: each field is sorted on its own by order-preserving 64-bit keys, -inf < .. < -0 < +0 < .. < +inf < NaN (every NaN is one
 * key); a tile sort in LDS, then ceil(log2(ceil(cells / 4096))) merge passes.  Keys carry nothing else, so the sorted sequence is
 * the one ascending arrangement of the values: field r of a batch has the bits of the one-field call, the same call twice gives the
 * same bits, and nothing depends on the tiling or the batch.  No atomics.
 * Scratch: two key buffers of n*cells 64-bit keys (the second only when cells > 4096) and q's copy are owned by the handle
 * (grow-only, released by gsm_destroy; growing one frees the smaller buffer, which waits for the device).
 * Errors (GSM_E_ARG, nothing launched): a NULL pointer other than sorted, quantiles or sorted == x, n < 1, cells outside [1, 2^24],
 * nq outside [2, 2^20], a q that does not ascend within [0, 1] (NaN included), n * ceil(cells / 4096) beyond one launch's 2^31
 * workgroups.
 * Replaces: nst_trans = QuantileTransformer(n_quantiles=1000, output_distribution="normal", subsample=None,
 * random_state=rng_seed).fit(data) (smallScaleChain_multiprocessing.py:493-494) for every large-scale bed of an ensemble at once;
 * sklearn/preprocessing/_data.py QuantileTransformer._dense_fit.  references_ = np.linspace(0, 1, nq) and n_quantiles_ = nq are
 * the caller's. */
int gsm_qt_fit(gsm_handle h, const double* x, int32_t n, int64_t cells, const double* q, int32_t nq, double* quantiles,
               int64_t* n_valid, int64_t* n_inf, double* sorted, void* stream);

/* ---- posterior accumulator: moments of the bed over all chains and a thinned set of iterations --------------------------
 * The reference looks inside a run through host caches of one chain: bed_cache[i] = bed_c (only_save_last_bed=False,
 * MCMC.py:1198, :1362-1363) and sample_values[:, i] = bed_c at the sample points (set_sample_points_locations,
 * MCMC.py:1174-1182, :1366), one whole-bed copy per iteration.  These entry points keep, on the device and for every chain of
 * the handle, what statistics of bed_cache[burn_in::thin] need -- shifted sums per cell -- and copy the sample points.  The
 * caller decides which iterations are snapshots and calls once per snapshot between two run calls; all arrays are caller-owned.
 * `beds` is the handle's state array [dev, n_chains*H*W] in its state dtype (double, or float for dtype 1).
 *
 * gsm_posterior_accumulate: one snapshot into the sums of ONE sequence of every chain (a chain, or one half of it for
 * split-R-hat).  ref [dev, n_chains*H*W], state dtype: each chain's bed at the first snapshot of the sequence being filled.  first != 0: ref = bed is
 * written and s1 = d, s2 = d*d with d = bed - bed (0; NaN where the bed is not finite); otherwise d = bed - ref, s1 += d,
 * s2 += d*d.  s1, s2 [dev, n_chains*H*W] fp64.  The shift keeps the variance (s2 - s1^2/N)/(N-1) free of cancellation against
 * the bed's magnitude, and a cell that never changes has d == 0, hence s1 == s2 == 0 and variance 0, exactly.  beds, ref, s1
 * and s2 must be 16-byte aligned (GSM_E_ARG otherwise).  sample_out [dev, n_chains*n_samples] fp64 (may be NULL) receives
 * bed_c[sample_cells[p]] at c*n_samples + p, sample_cells [dev, n_samples] flat cell indices row*W+col (NaN for an index
 * outside the grid).  48 bytes per chain-cell with fp64 state (8 bed, 8 ref, 16 read and 16 written of the sums), one pass.
 * Replaces: bed_cache / sample_values of chain_crf.run (MCMC.py:1198, :1362-1366) as the input of per-chain moments.
 *
 * gsm_posterior_accumulate_pooled: the same snapshot into sums over ALL chains, when no per-chain statistic is wanted:
 * S1[cell] += sum_c d, S2[cell] += sum_c d*d with d = bed_c - g, g [dev, H*W] fp64 one common reference field, S1, S2
 * [dev, H*W] fp64.  Reads the beds only (8 bytes per chain-cell).  Chains are summed in index order within a part of the chain
 * axis and the parts in part order (a second kernel; no atomics): bit-reproducible from run to run.
 *
 * gsm_posterior_sample: the sample points alone (a snapshot that belongs to no sequence).
 *
 * gsm_posterior_close: a finished sequence's sums become its statistics, in place: s1 = a_m = (ref_c - g) + s1 / N (the
 * sequence mean minus the common field g [dev, H*W]), s2 = v_m = (s2 - s1^2 / N) / (N - 1) (its ddof=1 variance), N = n_per_seq.
 * `ref` is then free for the next sequence of the same chains (gsm_posterior_accumulate with first != 0), so that every sequence
 * is shifted by a bed of its own: a cell that is constant within a sequence has v_m == 0 exactly, also when it changed between
 * the two halves of a chain.  GSM_E_ARG for NULL pointers or n_per_seq < 2.
 *
 * gsm_posterior_partials: reduction over this handle's sequences, per cell, to partials [dev, 3*H*W] fp64:
 *   P0 = sum_m a_m, P1 = sum_m a_m^2, P2 = sum_m v_m,  a_m = (ref_c - g) + s1_m / N,  v_m = (s2_m - s1_m^2 / N) / (N - 1)
 * with N = n_per_seq snapshots per sequence; a_m is sequence m's mean minus the common field g [dev, H*W] (which only keeps P1
 * well conditioned), v_m its ddof=1 variance.  Sequence k < n_seq_per_chain (1 or 2) of chain c has its sums at
 * s1 + k*seq_stride + c*H*W (likewise s2); the first n_closed sequences of every chain were closed (their arrays hold a_m, v_m),
 * the others are open and `ref` is theirs.  The sum runs over chains in index order, k innermost.  Partials of several handles
 * (ranks) add.  With M sequences in all: mean = g + P0/M, within-sequence variance W = P2/M, between-sequence variance over N
 * B/N = (P1 - P0^2/M)/(M-1), pooled ddof=1 variance ((N-1) P2 + N (P1 - P0^2/M)) / (M N - 1), R-hat = sqrt(((N-1)/N W + B/N) / W).
 * Errors: GSM_E_ARG for NULL pointers, n_per_seq < 2, n_seq_per_chain not 1 or 2, n_closed outside [0, n_seq_per_chain],
 * seq_stride < n_chains*H*W with two sequences.
 * Replaces: numpy statistics over bed_cache[burn_in::thin] of every chain of a pool (MCMC.py:1198, :1363).
 *
 * gsm_posterior_histogram: one snapshot into per-cell counts over ALL chains, from which quantiles of the bed (to within one
 * bin width) and probabilities of lying below fixed levels (exactly) follow; moments give neither where the posterior is skewed.
 * counts [dev, (n_bins + 3 + n_levels)*H*W] int32, slot-major (slot s of a cell at s*H*W + cell), is ADDED to: zero it once,
 * call once per snapshot; counts of several handles (ranks) add.  Per chain-cell value x = (double)bed, d = x - g[cell] with the
 * common field g [dev, H*W] fp64, and kf = floor(d * inv_width) + n_bins/2 in double (a product, a floor and a sum: nothing to
 * contract, so the slot is reproducible in any IEEE arithmetic), compared in double:
 *   NaN -> slot n_bins + 2;  kf < 0 -> slot 0 (underflow, also -inf);  kf >= n_bins -> slot n_bins + 1 (overflow, also +inf);
 *   otherwise slot (int)kf + 1: bin k = slot - 1 holds (k - n_bins/2) w <= d < (k + 1 - n_bins/2) w, w = 1 / inv_width (to the product's rounding).
 * Slots 0 .. n_bins + 2 of a cell therefore sum to the number of values seen.  Slot n_bins + 3 + l counts x < levels[l] (strict;
 * a NaN is below no level), levels [host, n_levels] absolute heights, read during the call.  n_bins even, 2 <= n_bins <= 128;
 * 0 <= n_levels <= 8.  Reads the beds only (8 bytes per chain-cell with fp64 state, 4 with fp32) and adds each part's non-zero
 * counters to `counts` (at most (n_bins + 3 + n_levels) * 4 bytes per cell and part of the chain axis).  Integer sums: the result
 * does not depend on the order and is bit-reproducible.  The caller keeps a cell's total below 2^31.
 * Errors: GSM_E_ARG for a NULL beds, g or counts, n_bins odd or outside [2, 128], n_levels outside [0, 8], NULL levels with
 * n_levels > 0, an inv_width that is not finite and > 0.
 * Replaces: np.quantile / (bed_cache < level).mean over bed_cache[burn_in::thin] of every chain of a pool (MCMC.py:1198, :1363).
 *
 * gsm_posterior_lagged: one snapshot into per-cell sums of squared differences at the lags 1 .. n_lags, over ALL chains:
 *   lag_sqdiff[(t - 1)*H*W + cell] += sum_c (x_c - y_{c,t})^2   for t = 1 .. n_valid,
 * x_c = (double)bed of chain c, y_{c,t} = (double)bed of chain c at the snapshot t calls earlier.  These are the sums S_t of the
 * variogram form of the autocorrelation rho_t = 1 - S_t / (M (N - t)) / (2 var+) (Gelman et al., BDA3 section 11.5), which needs no
 * per-chain mean; the effective sample size follows on the host.  ring [dev, n_lags*n_chains*H*W], state dtype, slot-major
 * (slot s of chain c at (s*n_chains + c)*H*W), holds the last snapshots of every chain and belongs to the caller, who also keeps
 * its two counters: the call reads slot (head - t) mod n_lags for t = 1 .. n_valid (the other slots are not read: the ring needs
 * no initialisation), then writes the beds to slot `head`; after it the caller sets head = (head + 1) mod n_lags and
 * n_valid = min(n_valid + 1, n_lags).  n_valid = 0 starts a sequence: the call only stores the beds, so no pair straddles two
 * sequences.  lag_sqdiff [dev, n_lags*H*W] fp64 is ADDED to: zero it once; sums of several handles (ranks) add.  A NaN bed makes
 * the sums of its cell NaN at the lags that pair it.  Differences, squares and sums are fp64 with either state type.  Chains are
 * summed in index order within a part of the chain axis and the parts in part order (a second kernel; no atomics):
 * bit-reproducible from run to run.  (n_valid + 2) state values per chain-cell are moved (n_valid + 1 read, 1 written): 72 bytes
 * at n_lags = 7 with fp64 state and a full ring, 36 with fp32.
 * Errors: GSM_E_ARG for a NULL beds, ring or lag_sqdiff, n_lags outside [1, 15], head outside [0, n_lags), n_valid outside
 * [0, n_lags], beds or ring not 16-byte aligned; nothing is written then.
 * Replaces: autocorrelations of bed_cache[burn_in::thin] of every chain of a pool (MCMC.py:1198, :1363).
 *
 * gsm_posterior_project and gsm_posterior_cross: the posterior covariance matrix C (H*W x H*W) applied to n_probes <= 15 weight
 * fields ("probes") of the grid's shape, probes [dev, n_probes*H*W] fp64, probe-major: an indicator gives the covariance map with
 * a point, a normalised mask that with a region mean, random fields the sketch of a low-rank factorisation.  With d_c[cell] =
 * (double)bed_c[cell] - g[cell], g [dev, H*W] fp64 the common field:
 *   project   proj[c*n_probes + k] = sum over the cells with probes[k][cell] != 0 of probes[k][cell] * d_c[cell]     (written)
 *   cross     cross[k*H*W + cell] += sum_c d_c[cell] * proj[c*n_probes + k]                                          (ADDED to)
 * proj [dev, n_chains*n_probes] fp64, chain-major; cross [dev, n_probes*H*W] fp64: zero it once, call project then cross once
 * per snapshot with the same beds; sums of several handles (ranks) add.  With n values per cell in all, S1 = sum d and q_k = sum
 * of proj over the same values, the covariance of cell and functional k is (cross_k - S1 q_k / n) / (n - 1).
 * A cell with weight zero is skipped, not multiplied: a NaN bed outside a probe's support does not touch that probe, one inside
 * it makes proj[c, k] NaN.  In cross a NaN d or a NaN proj makes the entries it enters NaN: a NaN bed its cell for every k, a NaN
 * proj[c, k] the whole field k.  Differences, products and sums are fp64 with either state type; cross uses fused multiply-adds.
 * No atomics: project sums a chain's cells in a fixed tree (lane, wave, workgroup, then the plane parts in part order); cross
 * sums the chains in index order within a part of the chain axis and the parts in part order (a second kernel):
 * bit-reproducible from run to run.  Bytes per chain-cell: project reads one state value from memory and (1 + n_probes) * 8 bytes
 * of g and the probes, which every chain re-reads and which are expected to stay in the caches (7.5 MiB of probes at 256 x 256 x 15);
 * cross reads one state value (8 bytes with fp64 state, 4 with fp32) and, per chain and wave, n_probes * 8 bytes of proj.
 * Errors: GSM_E_ARG for a NULL pointer, n_probes outside [1, 15], beds not 16-byte aligned; GSM_E_UNSUPPORTED for project with
 * more than 65535 chains; nothing is written then.
 * Replaces: np.cov of bed_cache[burn_in::thin] of every chain of a pool against functionals of it (MCMC.py:1198, :1363).
 *
 * gsm_posterior_residual: one snapshot into per-cell sums of the mass-conservation residual over ALL chains -- where the ensemble
 * fails to meet mass conservation, by how much, and how much of that the chains agree on.  For every chain c, r_c is the residual
 * of (double)bed_c from the static fields and the resolution of gsm_set_static, np.gradient differences, one-sided at the four
 * borders: the value, bit for bit, that gsm_residual writes for the same bed.  sums [dev, (3 + n_levels)*H*W] fp64, plane-major,
 * is ADDED to: zero it once, call once per snapshot; sums of several handles (ranks) add.  Per cell, over the chains whose r_c is
 * finite (a NaN or an infinity is skipped: the loss's nansum, MCMC.py:1041) and with d = r_c - rg[cell], rg [dev, H*W] fp64 any
 * finite field (a shift that keeps S2 - S1^2 / cnt free of cancellation against the residual's magnitude):
 *   plane 0   cnt += the number of those chains          plane 1   S1 += sum d          plane 2   S2 += sum d*d
 *   plane 3 + l   A_l += the number of them with |r_c| > levels[l]   (a NaN compares false)
 * levels [host, n_levels], 0 <= n_levels <= 4, finite and >= 0, in the residual's unit, read during the call.  The counts are
 * exact integers in fp64.  One pass: the stencil and the sums in one kernel, no per-chain residual is stored; each bed value is
 * read by its own lane and as the neighbour of four others, from memory about once (8 bytes per chain-cell with fp64 state, 4
 * with fp32, plus the halo of a workgroup's tile).  Differences, products and sums are fp64 with either state type, without
 * fused multiply-adds.  No atomics: chains are summed in index order within a part of the chain axis and the parts in part order
 * (a second kernel): bit-reproducible from run to run.
 * Errors: GSM_E_ARG for a NULL beds, rg or sums, n_levels outside [0, 4], NULL levels with n_levels > 0, a level that is negative
 * or not finite, beds not 16-byte aligned; GSM_E_STATE before gsm_set_static; nothing is written then.
 * Replaces: Topography.get_mass_conservation_residual (Topography.py:592-612) over bed_cache[burn_in::thin] of every chain of a
 * pool, and the statistics of that stack.
 *
 * gsm_posterior_local: one snapshot into the per-cell cross sums of the bed with its neighbours over ALL chains -- the short-range
 * structure of the uncertainty, from which the variance of anything local and linear follows (a slope, a block mean, a correlation
 * length).  reach R in [1, 4]; the K = 2 R^2 + 2 R offsets (di, dj) of the upper half plane in this order: (0, 1) .. (0, R), then for
 * di = 1 .. R: (di, -R) .. (di, R) (K = 4, 12, 24, 40; the lower half plane holds the same pairs).  With d_c[cell] = (double)bed_c[cell]
 * - g[cell], g [dev, H*W] fp64 the common field:
 *   cross[k*H*W + i*W + j] += sum_c d_c[i, j] * d_c[i + di_k, j + dj_k]     where (i + di_k, j + dj_k) lies inside the grid
 * cross [dev, K*H*W] fp64, offset-major, is ADDED to: zero it once, call once per snapshot; sums of several handles (ranks) add.
 * With n values per cell in all, m = S1 / n at the cell and m' at its partner (S1 = sum d of the pooled moments), the covariance of
 * the pair is (cross_k - n m m') / (n - 1).  An entry whose partner lies outside the grid is never touched: it stays exactly 0.  A
 * NaN bed of chain c at a cell makes NaN exactly the entries that pair that cell -- its own K entries and entry k of the cell at
 * minus offset k, where those lie inside the grid -- and nothing else.  Differences, products and sums are fp64 with either state
 * type, the products and sums fused multiply-adds.  No atomics: chains are summed in index order within a part of the chain axis
 * and the parts in part order (a second kernel, one launch per group of at most 15 offsets): bit-reproducible from run to run.
 * One pass: each bed value is read from memory about once (8 bytes per chain-cell with fp64 state, 4 with fp32, plus the halo of a
 * workgroup's 8 x 64 tile: R rows below, R columns left and right), turned into d once and shared through LDS among the up to 2 K
 * multiply-adds that use it.  The part merge writes and reads back parts x K planes of the handle's slab.  The rule that bounds it:
 * parts = the parts that fill the device (as for the other passes, over the tiles), but at most 160 / K (4 at reach 4) and at
 * most what keeps parts x K x H x W doubles within 1 GiB; the call is refused where K planes alone exceed 1 GiB.  The cut changes
 * the order of the sum, never which terms enter it.
 * Errors: GSM_E_ARG for a NULL beds, g or cross, reach outside [1, 4], beds not 16-byte aligned; GSM_E_UNSUPPORTED where K x H x W
 * doubles exceed 1 GiB; nothing is written then.
 * Replaces: np.cov between neighbouring cells of bed_cache[burn_in::thin] of every chain of a pool (MCMC.py:1198, :1363).
 *
 * gsm_posterior_regions: one snapshot into non-linear functionals of EVERY chain's bed per region -- the scalars an ensemble is
 * published as: ice volume, volume above flotation (the sea-level contribution), area below sea level, area grounded below sea
 * level, the deepest and the highest point, and the hypsometric (area-elevation) curve.  None follows from per-cell moments or from
 * a projection.  region_bits [dev, H*W] uint8: bit k of a cell says that the cell belongs to region k < n_regions, 1 <= n_regions
 * <= 8; regions may overlap (a basin, its sub-basin, the whole domain); bits at or above n_regions are ignored.  surf is the plane
 * given to gsm_set_static.  Per chain c and cell, all fp64 with either state type and without fused multiply-adds, in this order:
 *   x = (double)bed;  s = surf[cell];  valid = isfinite(x) && isfinite(s)
 *   h = s - x;  t_thick = h > 0 ? h : 0
 *   b = x - sea_level;  p = density_ratio * (b < 0 ? b : 0);  q = h + p;  t_haf = q > 0 ? q : 0
 * so that the same expressions in any IEEE arithmetic give every term bit for bit (density_ratio = rho_water / rho_ice).
 * func [dev, n_chains*n_regions*8] fp64 is WRITTEN: func[(c*n_regions + k)*8 + f] over the valid cells of region k,
 *   f = 0  their number          f = 1  sum x            f = 2  sum t_thick        f = 3  sum t_haf
 *   f = 4  the number with b < 0    f = 5  the number with b < 0 and t_haf > 0 (grounded below sea level)
 *   f = 6  min x, +inf without a valid cell            f = 7  max x, -inf without a valid cell
 * Counts are exact integers in fp64.  A cell that is not valid enters nothing: it does not make its region NaN.
 * Hypsometry: n_bins = 0 (none; hyps may be NULL) or even in [2, 64].  kf = floor((x - hyps_lo) * hyps_inv_width) in double, a
 * difference, a product and a floor; kf < 0 -> slot 0, kf >= n_bins -> slot n_bins + 1, otherwise slot (int)kf + 1 (the slot rule
 * of gsm_posterior_histogram).  hyps [dev, n_chains*n_regions*(n_bins + 2)] int32, at (c*n_regions + k)*(n_bins + 2) + slot, is
 * ADDED to: zero it once, call once per snapshot; only valid cells are counted; the caller keeps a counter below 2^31.
 * One pass: each bed value is read from memory once per call and serves every region it belongs to (8 bytes per chain-cell with
 * fp64 state, 4 with fp32); the bit plane and surf, 9 bytes per cell, are re-read by every chain and are expected to stay in the
 * caches.  No floating-point atomics: the four sums are taken in a fixed tree (lane, wave, workgroup, then the plane parts in part
 * order, a second kernel), so func is bit-reproducible from run to run; the integer hypsometry counts are combined in LDS and with
 * integer atomics, exact in any order.
 * Errors: GSM_E_ARG for a NULL beds, region_bits or func, n_regions outside [1, 8], n_bins odd or outside {0} and [2, 64], a NULL
 * hyps with n_bins > 0, a sea_level that is not finite, a density_ratio that is not finite and > 0, with n_bins > 0 an
 * hyps_inv_width that is not finite and > 0 or an hyps_lo that is not finite, beds not 16-byte aligned; GSM_E_STATE before
 * gsm_set_static; GSM_E_UNSUPPORTED with more than 65535 chains; nothing is written then.
 * Replaces: region statistics over bed_cache[burn_in::thin] of every chain of a pool (MCMC.py:1198, :1363).
 * All twelve are asynchronous on `stream`. */
int gsm_posterior_accumulate(gsm_handle h, const void* beds, void* ref, double* s1, double* s2, int32_t first,
                             const int32_t* sample_cells, int32_t n_samples, double* sample_out, void* stream);
int gsm_posterior_accumulate_pooled(gsm_handle h, const void* beds, const double* g, double* s1, double* s2,
                                    const int32_t* sample_cells, int32_t n_samples, double* sample_out, void* stream);
int gsm_posterior_sample(gsm_handle h, const void* beds, const int32_t* sample_cells, int32_t n_samples, double* sample_out,
                         void* stream);
int gsm_posterior_close(gsm_handle h, const void* ref, const double* g, double* s1, double* s2, int32_t n_per_seq, void* stream);
int gsm_posterior_partials(gsm_handle h, const void* ref, const double* g, const double* s1, const double* s2,
                           int32_t n_seq_per_chain, int64_t seq_stride, int32_t n_closed, int32_t n_per_seq, double* partials,
                           void* stream);
int gsm_posterior_histogram(gsm_handle h, const void* beds, const double* g, double inv_width, int32_t n_bins, const double* levels,
                            int32_t n_levels, int32_t* counts, void* stream);
int gsm_posterior_lagged(gsm_handle h, const void* beds, void* ring, int32_t n_lags, int32_t head, int32_t n_valid,
                         double* lag_sqdiff, void* stream);
int gsm_posterior_project(gsm_handle h, const void* beds, const double* g, const double* probes, int32_t n_probes,
                          double* proj /* [dev, n_chains*n_probes], written */, void* stream);
int gsm_posterior_cross(gsm_handle h, const void* beds, const double* g, const double* proj, int32_t n_probes,
                        double* cross /* [dev, n_probes*H*W], ADDED to */, void* stream);
int gsm_posterior_residual(gsm_handle h, const void* beds, const double* rg, const double* levels, int32_t n_levels,
                           double* sums /* [dev, (3+n_levels)*H*W], ADDED to */, void* stream);
int gsm_posterior_local(gsm_handle h, const void* beds, const double* g, int32_t reach,
                        double* cross /* [dev, K*H*W], ADDED to */, void* stream);
int gsm_posterior_regions(gsm_handle h, const void* beds, const uint8_t* region_bits, int32_t n_regions,
                          double sea_level, double density_ratio,
                          double* func /* [dev, n_chains*n_regions*8], written */,
                          double hyps_lo, double hyps_inv_width, int32_t n_bins,
                          int32_t* hyps /* [dev, n_chains*n_regions*(n_bins+2)], ADDED to; NULL with n_bins 0 */,
                          void* stream);

/* ---- variogram map of gridded fields ---------------------------------------------------------------------------------------
 * On an axis-aligned uniform grid the separation of two cells depends on their integer offset (di, dj) alone, so an
 * experimental variogram with any bins (isotropic or directional) is host arithmetic on one small table per field: for every
 * offset of the half plane di in [0, mi], dj in [-mj, mj]
 *   sum   [dev, n_fields*(mi+1)*(2*mj+1)] fp64    sum of (z[i, j] - z[i+di, j+dj])^2 over the cells (i, j) with both cells inside
 *                                                 the grid and both values present, at (r*(mi+1) + di)*(2*mj+1) + dj + mj
 *   count [dev, same extent] int64                the number of those pairs
 * The entries (0, dj <= 0) are zero: (0, -dj) holds the same pairs.  Semivariance of an offset: sum / (2 count).
 *   fields [dev, n_fields*H*W] fp64               row-major; NaN or an infinity marks a missing cell; not written
 *   mask   [dev, H*W] uint8, or NULL              shared by all fields: a 0 makes the cell count as missing
 *   mi, mj                                        mi >= H or mj >= W is legal: offsets beyond the grid hold 0 / 0
 *   rows_per_part                                 0 = the library's default, a function of (H, W, mi, mj) alone.  The rows of a
 *                                                 field are summed in parts of this many rows (so that one field fills the device)
 *                                                 and the parts are added in part order by a second kernel
 * No atomics; neither the split nor the order of any sum depends on n_fields or on the device: the same call twice gives the
 * same bits, and field r of a batched call gives the bits of the call on that field alone.  Each term is computed in fp64 with
 * three roundings (difference, square, addition).  Asynchronous on `stream`; all arrays are caller-owned (the partials of a
 * split live in the handle).
 * Errors: GSM_E_ARG for NULL fields / sum / count, n_fields < 1, mi < 0 or mj < 0, rows_per_part < 0, more than 65535 parts;
 * GSM_E_UNSUPPORTED for mi or mj above 2^20 or an offset table of more than about 2^33 entries.
 * Replaces: the pair sums inside skgstat.Variogram as the reference calls it (gstatsim_custom/utilities.py:102, variograms;
 * MCMC.py:305, fit_variogram), which take scattered points and compare every pair's distance with the bin edges. */
int gsm_variogram_map(gsm_handle h, const double* fields, int32_t n_fields, const uint8_t* mask, int32_t mi, int32_t mj,
                      int32_t rows_per_part, double* sum, int64_t* count, void* stream);

/* ---- local variogram maps: one table per tile, or per window of tiles ---------------------------------------------------------
 * The grid is cut into tiles of tile x tile cells, Ty = ceil(H / tile) by Tx = ceil(W / tile), the last row and column ragged.
 * A pair (i, j), (i + di, j + dj) of gsm_variogram_map's half plane belongs to the tile that holds its midpoint,
 *   ti = (2 i + di) / (2 tile),  tj = (2 j + dj) / (2 tile)       (integer division; both numerators are >= 0),
 * whichever end is called first: every pair belongs to exactly one tile, and the tile tables add up to gsm_variogram_map's.
 * The window of a tile is the (2 half_window + 1)^2 tiles centred on it, clipped at the lattice's edge; its table is the sum of
 * its tiles' tables in ascending (ti, tj).  half_window = 0 returns the tile tables themselves.
 *   sum, count [dev, n_fields*Ty*Tx*(mi+1)*(2*mj+1)]   per field, window and offset, at
 *                                                      (((r*Ty + ti)*Tx + tj)*(mi+1) + di)*(2*mj+1) + dj + mj; fp64 / int64
 *   fields, mask, mi, mj                               as gsm_variogram_map: (0, dj <= 0) and offsets beyond the grid hold 0 / 0
 *   tile                                               >= 2; a tile beyond the grid is one tile
 * No atomics; no sum's order depends on n_fields or on the device: the same call twice gives the same bits, and field r of a
 * batched call gives the bits of the call on that field alone.  Terms as gsm_variogram_map's (three roundings each).
 * With half_window > 0 the tile tables are a scratch of the call (fields go through in slices of at most 1 GiB of it) and the
 * call returns when `stream` has drained; with half_window == 0 it is asynchronous on `stream`.
 * Errors (a refused call writes nothing): GSM_E_ARG for NULL fields / sum / count, n_fields < 1, mi < 0 or mj < 0, tile < 2,
 * half_window < 0; GSM_E_UNSUPPORTED for mi or mj above 2^20, more than 2^31 entries per field, more than 65535 tile rows or
 * 2^30 workgroups per tile row; GSM_E_HIP (with the size) when the scratch cannot be allocated.
 * Replaces: one gsm_variogram_map call per cropped window, which counts every pair once per window that holds it.  The
 * reference takes per-cell variogram parameters (interpolate.py:56-62) and has no estimator for them. */
int gsm_variogram_local(gsm_handle h, const double* fields, int32_t n_fields, const uint8_t* mask, int32_t mi, int32_t mj,
                        int32_t tile, int32_t half_window, double* sum, int64_t* count, void* stream);

/* Diagnostics: stream-copy n doubles src -> dst [dev] with the step kernel's access shape (8 bytes per lane,
 * coalesced).  A known byte count for calibrating rocprofv3's FETCH_SIZE / WRITE_SIZE (MI355X_MICROARCH.md, HBM). */
int gsm_debug_stream_copy(const double* src, double* dst, int64_t n, void* stream);

/* Test hook: the device's standard-normal pairs (Philox4x32-10 counters (idx, stream, step), Box-Muller with the table-driven
 * log / sincos, 53 bits per uniform: normals2, as the nugget pass and the Cholesky generator draw; the coefficient phase's normals4
 * is reached through gsm_debug_proposal_math) for idx = idx0 .. idx0 + n - 1: out[2 i], out[2 i + 1] [dev].  Checked against
 * oracle/philox_oracle.normals2 (numpy log / sqrt / cos / sin). */
int gsm_debug_normals(uint64_t seed, int64_t step, uint32_t stream_id, uint32_t idx0, int32_t n, double* out, void* stream);

/* Test hook: the scalar special functions of the device, element by element -- out[i] = f(x0[i], x1[i], ...) for i < n, with the
 * device compiler's code and the device's libm (exp, log, log1p, expm1, hypot, sqrt), through the very functions the whole-grid
 * SGS and kriging kernels call.  Takes no handle.
 *   which          GSM_SPECIAL_*: the function and the arguments it reads (x0, x1, ... in the order given below)
 *   vtype          GSM_VTYPE_EXPONENTIAL / _GAUSSIAN / _SPHERICAL for GSM_SPECIAL_LOCAL_COV; ignored otherwise
 *   x0 .. x4       [dev, n] each; the ones `which` does not read may be NULL
 *   out            [dev, n]
 *   flag           [dev, 1] int32: zeroed, then the error bits the function raises are OR-ed into it (only
 *                  GSM_SPECIAL_TRUNCNORM_DRAW raises one: 128 for sd <= 0 or NaN, or lower >= upper after standardising -- that
 *                  element is NaN, the others of the launch are unaffected)
 * Returns after the stream has drained.  Errors: GSM_E_ARG for an unknown `which`, n < 1 or n >= 2^31 - 256, a NULL out / flag or
 * a NULL argument that `which` reads, a vtype that GSM_SPECIAL_LOCAL_COV does not evaluate; GSM_E_HIP for a runtime failure.
 * Checked against scipy 1.15 (scipy.special, scipy.stats.truncnorm) and mpmath by tests/test_gpu_special.py. */
enum {
  GSM_SPECIAL_NDTR = 0,           /* scipy.special.ndtr(x0) */
  GSM_SPECIAL_NDTRI = 1,          /* scipy.special.ndtri(x0) */
  GSM_SPECIAL_ERFC = 2,           /* scipy.special.erfc(x0) */
  GSM_SPECIAL_LOG_NDTR = 3,       /* scipy.special.log_ndtr(x0) */
  GSM_SPECIAL_NDTRI_EXP = 4,      /* scipy.special.ndtri_exp(x0) */
  GSM_SPECIAL_ERFCX_POS = 5,      /* scipy.special.erfcx(x0), x0 >= 0 */
  GSM_SPECIAL_LOG_GAUSS_MASS = 6, /* log of the standard normal mass in [x0, x1] */
  GSM_SPECIAL_TRUNCNORM_PPF = 7,  /* scipy.stats.truncnorm.ppf(q = x0, a = x1, b = x2) */
  GSM_SPECIAL_TRUNCNORM_DRAW = 8, /* the bounded draw of gsm_sgs_grid: (est, sd, lower, upper, u) = (x0 .. x4) */
  GSM_SPECIAL_LOCAL_COV = 9,      /* the covariance of gsm_*_grid_local: (squared normalised lag, sill - nugget, sill) = (x0, x1, x2) */
  GSM_SPECIAL_COUNT = 10
};
int gsm_debug_special(int32_t which, int32_t vtype, int64_t n, const double* x0, const double* x1, const double* x2, const double* x3,
                      const double* x4, double* out, int32_t* flag, void* stream);

/* Test hook: the scalar arithmetic of the Philox proposal path on the device, element by element, on caller-supplied arguments --
 * the very inline functions the proposal, chain and Cholesky kernels call (csrc/proposal_device.h, csrc/math_tables.h, csrc/philox.h),
 * with the math table staged in LDS as those kernels stage it.  Takes no handle.
 *   which          GSM_PMATH_*: the function, the layout of x0 and of out (below); i < n throughout
 *   model          GSM_MODEL_* and
 *   smoothness     the Matern nu (0 stands for 1, as in gsm_rf_params): GSM_PMATH_SPECTRAL_AMP only, ignored otherwise
 *   x0             [dev] fp64 [n], or uint32 words where the selector says so
 *   x1, x2, x3     [dev, n] fp64: GSM_PMATH_SPECTRAL_AMP only; may be NULL otherwise
 *   out            [dev] fp64 (uint32 for GSM_PMATH_PHILOX), n times the selector's values per element
 * Returns after the stream has drained.  Errors: GSM_E_ARG for an unknown `which`, n < 1 or n >= 2^31 - 256, a NULL x0 / out, and for
 * GSM_PMATH_SPECTRAL_AMP a NULL x1 / x2 / x3 or an unknown model -- nothing is written then; GSM_E_HIP for a runtime failure.
 * Checked against mpmath at constructed arguments by tests/test_gpu_proposal_math.py (point sets and bars: tests/proposal_math_common.py). */
enum {
  GSM_PMATH_PHILOX = 0,         /* x0 uint32 [n][6] = (seed lo, seed hi, step lo, step hi, stream, idx) -> out uint32 [n][4]: philox_draw */
  GSM_PMATH_LOG_TAB = 1,        /* x0 = x (positive, finite, normal) -> log_tab(x) */
  GSM_PMATH_SINCOS_TAB = 2,     /* x0 = u in [0, 1) -> out [n][2] = (sin, cos)(2 pi u) of sincos_tab */
  GSM_PMATH_SQRT_LEAN = 3,      /* x0 = t in [0, 2^500) -> sqrt_lean(t) */
  GSM_PMATH_EXP_LEAN = 4,       /* x0 = x -> exp_lean(x) */
  GSM_PMATH_NORMALS4_WORDS = 5, /* x0 uint32 [n][4] = one Philox block -> out [n][4] = (g1, g2, h1, h2) of normals4 (coefficient phase) */
  GSM_PMATH_NORMALS2_WORDS = 6, /* x0 uint32 [n][4] = one Philox block -> out [n][2] = (g1, g2) of normals2 / normals2_key */
  GSM_PMATH_SPECTRAL_AMP = 7,   /* (x0, x1, x2, x3) = (aa, m_kappa, m_const, k2) -> spectral_amp of `model`, `smoothness` */
  GSM_PMATH_COUNT = 8
};
int gsm_debug_proposal_math(int32_t which, int32_t model, double smoothness, int64_t n, const void* x0, const double* x1, const double* x2,
                            const double* x3, void* out, void* stream);

/* Test hook: one Philox4x32-10 block on the host (ctr[4], key[2] -> out[4]); the device generator uses
 * the same inline function.  Checked against the Random123 known-answer vectors. */
int gsm_philox_selftest(const uint32_t* ctr4, const uint32_t* key2, uint32_t* out4);

/* sizeof of a struct of this header as the library was compiled: which = 0 gsm_rf_params, 1 gsm_sgs_batch, 2 gsm_vario; -1 for any other value.
 * For bindings that restate the structs (ctypes, cgo ...): a mismatch is a layout error that would otherwise corrupt silently. */
int gsm_struct_size(int32_t which);

#ifdef __cplusplus
}
#endif
#endif /* GSM_H */
