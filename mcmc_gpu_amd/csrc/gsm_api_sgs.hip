// C ABI of libgsm_hip.so, sequential Gaussian simulation: the small-scale chain (gsm_sgs_* on blocks, gsm_sgs_iterate), whole-grid gsm_sgs_grid, gsm_krige_grid and the cross-validation gsm_krige_cv, each with its per-cell-variogram twin (gsm_*_local), and gsm_sgs_grid's draws from NumPy generators (gsm_sgs_grid_draw_pcg64).
#include "gsm_context.h"
#include <algorithm>

using namespace gsm;

// The grid, variogram and search of a call from the arguments of its entry point `w` and the handle, with the checks that
// gsm_sgs_blocks*, gsm_sgs_iterate, gsm_sgs_grid* and gsm_krige_grid* share: the search parameters, and a lag table (lag_cov; local
// NULL, vtype 0) or a variogram per cell (local; lag_cov NULL, lag_mi, lag_mj, sill unused), never both.  Each entry has checked its
// own pointers and keeps its own limits on the grid.
static int krige_search_fill(gsm_handle h, const std::string& w, KrigeSearch& K, const double* x_axis, const double* y_axis,
                             const double* lag_cov, int32_t lag_mi, int32_t lag_mj, const double* local, int32_t vtype, int32_t hw,
                             double radius, int32_t num_points, double sill) {
  if (hw < 1) return fail(h, GSM_E_ARG, w + ": search half-width (ceil(radius / grid spacing)) must be >= 1 cell");
  if (num_points < 8 || num_points > kSgsMaxPts) return fail(h, GSM_E_UNSUPPORTED, w + ": num_points must be in [8, 48]");
  if (!(radius > 0.0)) return fail(h, GSM_E_ARG, w + ": radius must be > 0");
  if (lag_mi < 0 || lag_mj < 0) return fail(h, GSM_E_ARG, w + ": lag table extents must be >= 0");
  if ((lag_cov == nullptr) == (local == nullptr)) return fail(h, GSM_E_ARG, w + ": NULL pointer");
  K.H = h->H; K.W = h->W; K.xs = x_axis; K.ys = y_axis; K.lag = lag_cov; K.mi = lag_mi; K.mj = lag_mj; K.local = local; K.vtype = vtype;
  K.hw = hw; K.num_points = num_points; K.ktype = h->sgs_ktype; K.gmean = h->sgs_gmean; K.radius = radius; K.sill = sill;
  K.err = h->d_err.get();
  return GSM_OK;
}

// One row of an entry point's table of device flags (gsm_internal.h: SgsFlag): the code and the text (after the entry's name) of the
// error that the flag means there.  sgs_report_flags reads and clears the handle's flag once `st` has drained and reports the first
// row whose bit is set; a flag of no row is `rest` (after the entry's name), or "device flag N" without one.
struct SgsFlagRow { int32_t bit; int code; const char* text; };
template <size_t N>
static int sgs_report_flags(gsm_handle h, hipStream_t st, const std::string& w, const SgsFlagRow (&rows)[N], const char* rest = nullptr) {
  int32_t flag = 0;
  if (int rc = read_and_clear_flag(h, st, &flag)) return rc;
  if (!flag) return GSM_OK;
  for (const SgsFlagRow& r : rows)
    if (flag & r.bit) return fail(h, r.code, w + r.text);
  return fail(h, GSM_E_DEVICE_DATA, w + (rest ? std::string(rest) : ": device flag " + std::to_string(flag)));
}
// kSgsFlagLagTable is GSM_E_ARG from the block and whole-grid SGS entries and GSM_E_DEVICE_DATA from gsm_krige_grid*: kept as it was
static const SgsFlagRow kBlockFlags[] = {
  {kSgsFlagNoValue, GSM_E_DEVICE_DATA, ": a cell to simulate has no conditioning value anywhere on the grid (the reference "
                                       "would widen its search radius for ever, MCMC.py:150-156)"},
  {kSgsFlagSingular, GSM_E_DEVICE_DATA, ": singular kriging system (a pivot below eps * N * max|diag|: numpy.linalg.lstsq "
                                        "would truncate singular values there, _krige.py:37)"},
  {kSgsFlagNoCentre, GSM_E_DEVICE_DATA, ": no block centre inside the region mask after 64 attempts"},
  {kSgsFlagLagTable, GSM_E_ARG, ": the lag covariance table does not reach the lag between two chosen neighbours "
                                "(lag_mi / lag_mj must cover 2 * hw, or the whole grid when the search radius is widened)"}};
static const char kBlockFlagsRest[] = ": window outside the grid / larger than 1024 cells, more cells than max_cells, or a listed cell outside its window";
static const SgsFlagRow kGridFlags[] = {
  {kSgsFlagCell, GSM_E_DEVICE_DATA, ": a path cell outside the grid, holding a value, or listed twice"},
  {kSgsFlagNoValue, GSM_E_DEVICE_DATA, ": a cell to simulate has no value anywhere on the grid (the reference would widen "
                                       "its search radius for ever, interpolate.py:150-157)"},
  {kSgsFlagSingular, GSM_E_DEVICE_DATA, ": singular kriging system (a pivot below eps * N * max|diag|)"},
  {kSgsFlagLagTable, GSM_E_ARG, ": the lag covariance table does not reach the lag between two chosen neighbours "
                                "(it must cover twice the widest search radius)"},
  {kSgsFlagTruncnorm, GSM_E_DEVICE_DATA, ": truncated-normal draw outside scipy's domain (kriging variance 0, or "
                                         "lower >= upper after standardising)"}};
static const SgsFlagRow kKrigeFlags[] = {
  {kSgsFlagCell, GSM_E_DEVICE_DATA, ": a listed cell outside the grid or holding a value"},
  {kSgsFlagNoValue, GSM_E_DEVICE_DATA, ": a cell to estimate has no value anywhere on the grid (the reference would widen "
                                       "its search radius for ever, interpolate.py:65-71)"},
  {kSgsFlagSingular, GSM_E_DEVICE_DATA, ": singular kriging system (a pivot below eps * N * max|diag|)"},
  {kSgsFlagLagTable, GSM_E_DEVICE_DATA, ": the lag covariance table does not reach the lag between two chosen neighbours "
                                        "(it must cover twice the widest search radius)"}};
static const SgsFlagRow kGridDrawFlags[] = {
  {kSgsFlagDrawBadCell, GSM_E_DEVICE_DATA, ": an entry of `cells` outside the grid"},
  {kSgsFlagDrawPathLen, GSM_E_DEVICE_DATA, ": path length: path_len is not the number of listed cells without a value"}};

static int sgs_fill(gsm_handle h, SgsArgs& a, double* grids, const double* zcond, const int32_t* windows, const double* x_axis,
                    const double* y_axis, const double* lag_cov, int32_t lag_mi, int32_t lag_mj, int32_t hw, double radius,
                    int32_t num_points, double sill, const int32_t* cell_off, const int32_t* cells, const double* z,
                    int32_t max_cells, const char* who, int parity = 0) {
  if (!grids || !windows || !x_axis || !y_axis || !lag_cov || !cell_off || !cells || !z) return fail(h, GSM_E_ARG, std::string(who) + ": NULL pointer");
  if (int rc = krige_search_fill(h, who, a.K, x_axis, y_axis, lag_cov, lag_mi, lag_mj, nullptr, 0, hw, radius, num_points, sill)) return rc;
  if (max_cells < 1 || max_cells > 1024) return fail(h, GSM_E_ARG, std::string(who) + ": max_cells must be in [1, 1024]");
  // cells travel packed as (row << 16 | col) in an int32 and are unpacked with an arithmetic shift: rows up to 32767
  if (h->H < 2 || h->W < 2 || h->H > 32767 || h->W > 32767) return fail(h, GSM_E_UNSUPPORTED, std::string(who) + ": grid sides must be in [2, 32767]");
  // scratch: per (chain, slot) 48 x (value, weight) and a header; then ranks [n][1024] i32, rank_ok [n] i32
  max_cells = (max_cells + 63) & ~63;                        // record stride: whole 64-cell chunks (sgs_sequence_kernel: one cell per lane)
  const size_t n = (size_t)h->n_chains, cells_cap = n * (size_t)max_cells;
  if (h->sgs_rec_cells[parity] < cells_cap) {
    h->sgs_rec_cells[parity] = 0;
    const size_t bytes = n * 1024 * 4 + n * 4 + 64 + cells_cap * (sizeof(SgsCellHdr) + 48 * sizeof(double2));
    hipError_t e = h->d_sgs_rec[parity].ensure(bytes);
    if (e != hipSuccess) return fail(h, GSM_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
    h->sgs_rec_cells[parity] = cells_cap;
  }
  char* p = h->d_sgs_rec[parity].get();
  const size_t cap = h->sgs_rec_cells[parity];
  a.rec_vw = (double2*)p; p += cap * 48 * sizeof(double2);
  a.rec_hdr = (SgsCellHdr*)p; p += cap * sizeof(SgsCellHdr);
  a.rank = (int32_t*)p; p += n * 1024 * 4;
  a.rank_ok = (int32_t*)p;
  a.n_chains = h->n_chains; a.grid = grids; a.zcond = zcond; a.win = windows;
  a.cell_off = cell_off; a.cells = cells; a.z = z; a.max_cells = max_cells; a.defer = 0; a.group = h->sgs_group();
  return GSM_OK;
}

extern "C" int gsm_sgs_blocks(gsm_handle h, double* grids, const double* zcond, const int32_t* windows, const double* x_axis,
                              const double* y_axis, const double* lag_cov, int32_t lag_mi, int32_t lag_mj, int32_t hw, double radius,
                              int32_t num_points, double sill, const int32_t* cell_off, const int32_t* cells, const double* z,
                              int32_t max_cells, double* trace, int32_t* nbr_trace, void* stream) {
  GSM_GRID_HANDLE(h);
  SgsArgs a{};
  HIPCHK(h, hipSetDevice(h->device));
  int rc = sgs_fill(h, a, grids, zcond, windows, x_axis, y_axis, lag_cov, lag_mi, lag_mj, hw, radius, num_points, sill, cell_off, cells, z,
                    max_cells, "gsm_sgs_blocks");
  if (rc) return rc;
  a.cell_cnt = nullptr; a.trace = trace; a.nbr_trace = nbr_trace;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(h, launch_sgs_blocks(a, a.max_cells, st));
  return sgs_report_flags(h, st, "gsm_sgs_blocks", kBlockFlags, kBlockFlagsRest);
}

extern "C" int gsm_sgs_blocks_batch(gsm_handle h, double* grids, const double* zcond, const int32_t* windows, const double* x_axis,
                                    const double* y_axis, const double* lag_cov, int32_t lag_mi, int32_t lag_mj, int32_t hw, double radius,
                                    int32_t num_points, double sill, const int32_t* cell_off, const int32_t* cell_cnt, const int32_t* cells,
                                    const double* z, int32_t max_cells, void* stream) {
  GSM_GRID_HANDLE(h);
  SgsArgs a{};
  HIPCHK(h, hipSetDevice(h->device));
  int rc = sgs_fill(h, a, grids, zcond, windows, x_axis, y_axis, lag_cov, lag_mi, lag_mj, hw, radius, num_points, sill, cell_off, cells, z,
                    max_cells, "gsm_sgs_blocks_batch");
  if (rc) return rc;
  a.cell_cnt = cell_cnt; a.trace = nullptr; a.nbr_trace = nullptr;
  HIPCHK(h, launch_sgs_blocks(a, a.max_cells, (hipStream_t)stream));
  return GSM_OK;
}

extern "C" int gsm_sgs_set_groups(gsm_handle h, const int32_t* group, int32_t n_groups) {
  GSM_GRID_HANDLE(h);
  HIPCHK(h, hipSetDevice(h->device));
  if (!group || n_groups == 1) {                              // one group is no groups: the entry points run as they always have
    HIPCHK(h, hipDeviceSynchronize());                        // nothing in flight reads the table that goes
    h->sgs_n_groups = 0;
    h->d_sgs_group.reset();
    return GSM_OK;
  }
  if (n_groups < 1) return fail(h, GSM_E_ARG, "gsm_sgs_set_groups: n_groups must be >= 1");
  for (int c = 0; c < h->n_chains; ++c)
    if (group[c] < 0 || group[c] >= n_groups)
      return fail(h, GSM_E_ARG, "gsm_sgs_set_groups: group[" + std::to_string(c) + "] = " + std::to_string(group[c]) + " is outside [0, n_groups)");
  HIPCHK(h, hipDeviceSynchronize());
  h->sgs_n_groups = 0;
  HIPCHK(h, h->d_sgs_group.ensure((size_t)h->n_chains));
  HIPCHK(h, hipMemcpy(h->d_sgs_group.get(), group, (size_t)h->n_chains * sizeof(int32_t), hipMemcpyHostToDevice));
  h->sgs_n_groups = n_groups;
  return GSM_OK;
}

extern "C" int gsm_sgs_set_kriging(gsm_handle h, int32_t ktype, const double* global_mean) {
  GSM_GRID_HANDLE(h);
  if (ktype != GSM_KRIGING_ORDINARY && ktype != GSM_KRIGING_SIMPLE) return fail(h, GSM_E_ARG, "gsm_sgs_set_kriging: ktype must be GSM_KRIGING_ORDINARY or GSM_KRIGING_SIMPLE");
  if (ktype == GSM_KRIGING_SIMPLE && !global_mean) return fail(h, GSM_E_ARG, "gsm_sgs_set_kriging: simple kriging needs the global mean of every chain");
  h->sgs_ktype = ktype; h->sgs_gmean = ktype == GSM_KRIGING_SIMPLE ? global_mean : nullptr;
  return GSM_OK;
}

// the model of a per-cell variogram table: the three the device evaluates (Matern needs Bessel K)
static int local_vtype_check(gsm_handle h, const std::string& w, int32_t vtype) {
  if (vtype != GSM_VTYPE_EXPONENTIAL && vtype != GSM_VTYPE_GAUSSIAN && vtype != GSM_VTYPE_SPHERICAL)
    return fail(h, GSM_E_UNSUPPORTED, w + ": vtype must be GSM_VTYPE_EXPONENTIAL, GSM_VTYPE_GAUSSIAN or GSM_VTYPE_SPHERICAL");
  return GSM_OK;
}

// gsm_sgs_grid (lag_cov, local NULL) and gsm_sgs_grid_local (local, lag_cov NULL; lag_mi, lag_mj, sill unused)
static int sgs_grid_run(gsm_handle h, const std::string& w, double* grids, const int32_t* path, const int64_t* path_off, int32_t max_path,
                        const double* draws, const double* lower, const double* upper, int32_t draw_kind, const double* x_axis,
                        const double* y_axis, const double* lag_cov, int32_t lag_mi, int32_t lag_mj, const double* local, int32_t vtype,
                        int32_t hw, double radius, int32_t num_points, double sill, int32_t seg_cells, double* trace, void* stream) {
  if (!grids || !path || !path_off || !draws || !x_axis || !y_axis || (!lag_cov && !local)) return fail(h, GSM_E_ARG, w + ": NULL pointer");
  if (draw_kind != GSM_DRAW_NORMAL && draw_kind != GSM_DRAW_TRUNCATED) return fail(h, GSM_E_ARG, w + ": draw_kind must be GSM_DRAW_NORMAL or GSM_DRAW_TRUNCATED");
  if ((draw_kind == GSM_DRAW_TRUNCATED) != (lower != nullptr) || (lower != nullptr) != (upper != nullptr))
    return fail(h, GSM_E_ARG, w + ": bounds (lower and upper) go with GSM_DRAW_TRUNCATED and only with it");
  SgsGridArgs a{};
  if (int rc = krige_search_fill(h, w, a.K, x_axis, y_axis, lag_cov, lag_mi, lag_mj, local, vtype, hw, radius, num_points, sill)) return rc;
  if (h->H > 32767 || h->W > 32767 || (int64_t)h->H * h->W > (1LL << 25))
    return fail(h, GSM_E_ARG, w + ": at most 2^25 cells and 32767 per side (25-bit slot and cell fields in the records)");
  if (h->n_chains > 65535) return fail(h, GSM_E_ARG, w + ": at most 65535 realisations per handle");
  if (max_path < 0 || (int64_t)max_path > (int64_t)h->H * h->W) return fail(h, GSM_E_ARG, w + ": max_path must be in [0, H * W]");
  if (seg_cells < 1) return fail(h, GSM_E_ARG, w + ": seg_cells must be >= 1");
  if (h->sgs_ktype == GSM_KRIGING_SIMPLE && !h->sgs_gmean) return fail(h, GSM_E_STATE, w + ": simple kriging without global means");
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  const size_t R = (size_t)h->n_chains, HW = (size_t)h->H * h->W;
  const int seg_cap = (int)std::min<int64_t>(((int64_t)seg_cells + 63) / 64 * 64, std::max<int64_t>(64, ((int64_t)max_path + 63) / 64 * 64));
  a.n_real = (int)R; a.grid = grids; a.path = path; a.path_off = path_off; a.draw = draws; a.lo = lower; a.hi = upper;
  a.draw_kind = draw_kind; a.trace = trace; a.seg_cap = seg_cap; a.seg_len = seg_cap;
  // scratch of the call: ranks [R][H*W], then per realisation seg_cap records (headers + 48 (value, weight) entries)
  const size_t bytes = R * HW * sizeof(int32_t) + 256 + R * (size_t)seg_cap * (sizeof(SgsGridHdr) + 48 * sizeof(double2));
  DevBuf<char> scratch;
  hipError_t e = scratch.ensure(bytes);
  if (e != hipSuccess) return fail(h, GSM_E_HIP, w + ": records of " + std::to_string(seg_cap) + " slots x " + std::to_string(R) +
                                                 " realisations: " + hipGetErrorString(e));
  char* p = scratch.get();
  a.rec_vw = (double2*)p; p += R * (size_t)seg_cap * 48 * sizeof(double2);
  a.rec_hdr = (SgsGridHdr*)p; p += R * (size_t)seg_cap * sizeof(SgsGridHdr);
  a.rank = (int32_t*)p;
  e = launch_sgs_grid_ranks(a, max_path, st);
  for (int s0 = 0; e == hipSuccess && s0 < max_path; s0 += seg_cap) {
    a.seg0 = s0; a.seg_len = std::min(seg_cap, max_path - s0);
    e = launch_sgs_grid_segment(a, st);
  }
  if (e != hipSuccess) return fail(h, GSM_E_HIP, w + ": " + hipGetErrorString(e));
  return sgs_report_flags(h, st, w, kGridFlags);                  // the scratch lives until the stream has drained
}

extern "C" int gsm_sgs_grid(gsm_handle h, double* grids, const int32_t* path, const int64_t* path_off, int32_t max_path,
                            const double* draws, const double* lower, const double* upper, int32_t draw_kind, const double* x_axis,
                            const double* y_axis, const double* lag_cov, int32_t lag_mi, int32_t lag_mj, int32_t hw, double radius,
                            int32_t num_points, double sill, int32_t seg_cells, double* trace, void* stream) {
  GSM_GRID_HANDLE(h);
  return sgs_grid_run(h, "gsm_sgs_grid", grids, path, path_off, max_path, draws, lower, upper, draw_kind, x_axis, y_axis, lag_cov, lag_mi,
                      lag_mj, nullptr, 0, hw, radius, num_points, sill, seg_cells, trace, stream);
}

extern "C" int gsm_sgs_grid_local(gsm_handle h, double* grids, const int32_t* path, const int64_t* path_off, int32_t max_path,
                                  const double* draws, const double* lower, const double* upper, int32_t draw_kind, const double* x_axis,
                                  const double* y_axis, const double* local, int32_t vtype, int32_t hw, double radius,
                                  int32_t num_points, int32_t seg_cells, double* trace, void* stream) {
  GSM_GRID_HANDLE(h);
  if (int rc = local_vtype_check(h, "gsm_sgs_grid_local", vtype)) return rc;
  return sgs_grid_run(h, "gsm_sgs_grid_local", grids, path, path_off, max_path, draws, lower, upper, draw_kind, x_axis, y_axis, nullptr, 0,
                      0, local, vtype, hw, radius, num_points, 0.0, seg_cells, trace, stream);
}

// gsm_krige_grid (lag_cov, local NULL) and gsm_krige_grid_local (local, lag_cov NULL; lag_mi, lag_mj, sill unused)
static int krige_grid_run(gsm_handle h, const std::string& w, const double* grid, const int32_t* cells, int32_t n_cells,
                          const double* x_axis, const double* y_axis, const double* lag_cov, int32_t lag_mi, int32_t lag_mj,
                          const double* local, int32_t vtype, int32_t hw, double radius, int32_t num_points, double sill, double* est,
                          double* var, int32_t* n_neighbours, void* stream) {
  if (n_cells < 0 || (int64_t)n_cells > (int64_t)h->H * h->W) return fail(h, GSM_E_ARG, w + ": n_cells must be in [0, H * W]");
  if (n_cells == 0) return GSM_OK;
  if (!grid || !cells || !x_axis || !y_axis || (!lag_cov && !local) || !est || !var || !n_neighbours) return fail(h, GSM_E_ARG, w + ": NULL pointer");
  KrigeGridArgs a{};
  if (int rc = krige_search_fill(h, w, a.K, x_axis, y_axis, lag_cov, lag_mi, lag_mj, local, vtype, hw, radius, num_points, sill)) return rc;
  if (h->H < 2 || h->W < 2 || h->H > 32767 || h->W > 32767) return fail(h, GSM_E_ARG, w + ": grid sides must be in [2, 32767]");
  if (h->n_chains != 1) return fail(h, GSM_E_ARG, w + ": one grid per handle (create it with n_chains = 1)");
  if (h->sgs_ktype == GSM_KRIGING_SIMPLE && !h->sgs_gmean) return fail(h, GSM_E_STATE, w + ": simple kriging without a global mean");
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  a.n_cells = n_cells; a.grid = grid; a.cells = cells; a.est = est; a.var = var; a.n = n_neighbours;
  HIPCHK(h, launch_krige_grid(a, st));
  return sgs_report_flags(h, st, w, kKrigeFlags);
}

extern "C" int gsm_krige_grid(gsm_handle h, const double* grid, const int32_t* cells, int32_t n_cells, const double* x_axis,
                              const double* y_axis, const double* lag_cov, int32_t lag_mi, int32_t lag_mj, int32_t hw, double radius,
                              int32_t num_points, double sill, double* est, double* var, int32_t* n_neighbours, void* stream) {
  GSM_GRID_HANDLE(h);
  return krige_grid_run(h, "gsm_krige_grid", grid, cells, n_cells, x_axis, y_axis, lag_cov, lag_mi, lag_mj, nullptr, 0, hw, radius,
                        num_points, sill, est, var, n_neighbours, stream);
}

extern "C" int gsm_krige_grid_local(gsm_handle h, const double* grid, const int32_t* cells, int32_t n_cells, const double* x_axis,
                                    const double* y_axis, const double* local, int32_t vtype, int32_t hw, double radius,
                                    int32_t num_points, double* est, double* var, int32_t* n_neighbours, void* stream) {
  GSM_GRID_HANDLE(h);
  if (int rc = local_vtype_check(h, "gsm_krige_grid_local", vtype)) return rc;
  return krige_grid_run(h, "gsm_krige_grid_local", grid, cells, n_cells, x_axis, y_axis, nullptr, 0, 0, local, vtype, hw, radius,
                        num_points, 0.0, est, var, n_neighbours, stream);
}

// gsm_krige_cv (lag_cov and sill, local and vtype NULL) and gsm_krige_cv_local (local and vtype, lag_cov and sill NULL; lag_mi, lag_mj
// unused): n_models tables one after the other, sill / vtype [n_models] on the host
static const SgsFlagRow kKrigeCvFlags[] = {
  {kSgsFlagCell, GSM_E_DEVICE_DATA, ": a listed cell outside the grid or holding no value"},
  {kSgsFlagNoValue, GSM_E_DEVICE_DATA, ": a cell to validate has no value anywhere on the grid outside its hold-out (its fold "
                                       "holds all the data, or the exclusion radius covers them)"},
  {kSgsFlagSingular, GSM_E_DEVICE_DATA, ": singular kriging system (a pivot below eps * N * max|diag|)"},
  {kSgsFlagLagTable, GSM_E_DEVICE_DATA, ": the lag covariance table does not reach the lag between two chosen neighbours "
                                        "(it must cover twice the widest search radius)"}};
static int krige_cv_run(gsm_handle h, const std::string& w, const double* grid, const int32_t* cells, int32_t n_cells, const int32_t* fold,
                        double exclude_radius, const double* x_axis, const double* y_axis, int32_t n_models, const double* lag_cov,
                        int32_t lag_mi, int32_t lag_mj, const double* sill, const double* local, const int32_t* vtype, int32_t hw,
                        double radius, int32_t num_points, double* est, double* var, int32_t* n_neighbours, void* stream) {
  if (n_cells < 0 || (int64_t)n_cells > (int64_t)h->H * h->W) return fail(h, GSM_E_ARG, w + ": n_cells must be in [0, H * W]");
  if (n_models < 1 || n_models > kKrigeCvMaxModels) return fail(h, GSM_E_ARG, w + ": n_models must be in [1, 8]");
  if (!(exclude_radius >= 0.0)) return fail(h, GSM_E_ARG, w + ": exclude_radius must be >= 0 (0: no buffer around the target)");
  if (n_cells == 0) return GSM_OK;
  if (!grid || !cells || !x_axis || !y_axis || (!lag_cov && !local) || (lag_cov && !sill) || (local && !vtype) || !est || !var || !n_neighbours)
    return fail(h, GSM_E_ARG, w + ": NULL pointer");
  KrigeCvArgs a{};
  if (int rc = krige_search_fill(h, w, a.K, x_axis, y_axis, lag_cov, lag_mi, lag_mj, local, 0, hw, radius, num_points, 0.0)) return rc;
  if (h->H < 2 || h->W < 2 || h->H > 32767 || h->W > 32767) return fail(h, GSM_E_ARG, w + ": grid sides must be in [2, 32767]");
  if (h->n_chains != 1) return fail(h, GSM_E_ARG, w + ": one grid per handle (create it with n_chains = 1)");
  if (h->sgs_ktype == GSM_KRIGING_SIMPLE && !h->sgs_gmean) return fail(h, GSM_E_STATE, w + ": simple kriging without a global mean");
  for (int m = 0; m < n_models; ++m) {
    if (local) { if (int rc = local_vtype_check(h, w, vtype[m])) return rc; a.vtype[m] = vtype[m]; }
    else a.sill[m] = sill[m];
  }
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  a.n_cells = n_cells; a.grid = grid; a.cells = cells; a.fold = fold; a.exclude_radius = exclude_radius; a.n_models = n_models;
  a.model_stride = local ? (int64_t)h->H * h->W * 6 : (int64_t)(2 * lag_mi + 1) * (2 * lag_mj + 1);
  a.est = est; a.var = var; a.n = n_neighbours;
  HIPCHK(h, launch_krige_cv(a, st));
  return sgs_report_flags(h, st, w, kKrigeCvFlags);
}

extern "C" int gsm_krige_cv(gsm_handle h, const double* grid, const int32_t* cells, int32_t n_cells, const int32_t* fold,
                            double exclude_radius, const double* x_axis, const double* y_axis, int32_t n_models, const double* lag_cov,
                            int32_t lag_mi, int32_t lag_mj, int32_t hw, double radius, int32_t num_points, const double* sill,
                            double* est, double* var, int32_t* n_neighbours, void* stream) {
  GSM_GRID_HANDLE(h);
  return krige_cv_run(h, "gsm_krige_cv", grid, cells, n_cells, fold, exclude_radius, x_axis, y_axis, n_models, lag_cov, lag_mi, lag_mj, sill,
                      nullptr, nullptr, hw, radius, num_points, est, var, n_neighbours, stream);
}

extern "C" int gsm_krige_cv_local(gsm_handle h, const double* grid, const int32_t* cells, int32_t n_cells, const int32_t* fold,
                                  double exclude_radius, const double* x_axis, const double* y_axis, int32_t n_models, const double* local,
                                  const int32_t* vtype, int32_t hw, double radius, int32_t num_points, double* est, double* var,
                                  int32_t* n_neighbours, void* stream) {
  GSM_GRID_HANDLE(h);
  return krige_cv_run(h, "gsm_krige_cv_local", grid, cells, n_cells, fold, exclude_radius, x_axis, y_axis, n_models, nullptr, 0, 0, nullptr,
                      local, vtype, hw, radius, num_points, est, var, n_neighbours, stream);
}

extern "C" int gsm_debug_special(int32_t which, int32_t vtype, int64_t n, const double* x0, const double* x1, const double* x2,
                                 const double* x3, const double* x4, double* out, int32_t* flag, void* stream) {
  if (which == GSM_SPECIAL_LOCAL_COV && vtype != GSM_VTYPE_EXPONENTIAL && vtype != GSM_VTYPE_GAUSSIAN && vtype != GSM_VTYPE_SPHERICAL)
    return GSM_E_ARG;
  const hipError_t e = launch_debug_special(which, vtype, n, x0, x1, x2, x3, x4, out, flag, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) return GSM_E_ARG;
  if (e != hipSuccess || hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return GSM_E_HIP;
  return GSM_OK;
}

extern "C" int gsm_sgs_check(gsm_handle h, void* stream) {
  GSM_GRID_HANDLE(h);
  HIPCHK(h, hipSetDevice(h->device));
  return sgs_report_flags(h, (hipStream_t)stream, "gsm_sgs_check", kBlockFlags, kBlockFlagsRest);
}

// the block size ranges and cell capacity that both gsm_sgs_draw_* entry points take
static int sgs_check_ranges(gsm_handle h, const std::string& w, int32_t min_x, int32_t max_x, int32_t min_y, int32_t max_y, int32_t max_cells) {
  if (min_x < 1 || max_x <= min_x || min_y < 1 || max_y <= min_y) return fail(h, GSM_E_ARG, w + ": block size ranges must be 1 <= min < max");
  if (max_cells < (max_x - 1) * (max_y - 1) || max_cells > 1024) return fail(h, GSM_E_ARG, w + ": max_cells must hold the largest block and be <= 1024");
  return GSM_OK;
}

extern "C" int gsm_sgs_draw_philox(gsm_handle h, const uint64_t* seeds, int64_t iter0, int32_t n_iters, const uint8_t* region_mask,
                                   const uint8_t* is_data, int32_t min_x, int32_t max_x, int32_t min_y, int32_t max_y, int32_t max_cells,
                                   int32_t* windows, int32_t* blocks, int32_t* cell_off, int32_t* cell_cnt, int32_t* cells, double* z,
                                   double* u, void* stream) {
  GSM_GRID_HANDLE(h);
  if (!seeds || !is_data || !windows || !blocks || !cell_off || !cell_cnt || !cells || !z || !u)
    return fail(h, GSM_E_ARG, "gsm_sgs_draw_philox: NULL pointer");
  if (n_iters < 1 || n_iters > 65535 || iter0 < 0) return fail(h, GSM_E_ARG, "gsm_sgs_draw_philox: n_iters must be in [1, 65535], iter0 >= 0");
  if (int rc = sgs_check_ranges(h, "gsm_sgs_draw_philox", min_x, max_x, min_y, max_y, max_cells)) return rc;
  if ((int64_t)n_iters * h->n_chains * max_cells >= (1LL << 31)) return fail(h, GSM_E_ARG, "gsm_sgs_draw_philox: n_iters * n_chains * max_cells must stay below 2^31 (32-bit cell offsets)");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, ensure_mathtab(h->d_mathtab));
  SgsDrawArgs a{};
  a.H = h->H; a.W = h->W; a.n_chains = h->n_chains; a.n_iters = n_iters; a.iter0 = iter0; a.seeds = seeds;
  a.region_mask = region_mask; a.is_data = is_data; a.min_x = min_x; a.max_x = max_x; a.min_y = min_y; a.max_y = max_y;
  a.max_cells = max_cells; a.mathtab = h->d_mathtab.get();
  a.win = windows; a.blk = blocks; a.cell_off = cell_off; a.cell_cnt = cell_cnt; a.cells = cells; a.z = z; a.u = u; a.err = h->d_err.get();
  HIPCHK(h, launch_sgs_draw(a, (hipStream_t)stream));
  return GSM_OK;
}

extern "C" int gsm_sgs_draw_pcg64(gsm_handle h, uint64_t* chain_state, int32_t n_iters, const uint8_t* region_mask,
                                  const uint8_t* is_data, int32_t min_x, int32_t max_x, int32_t min_y, int32_t max_y, int32_t max_cells,
                                  int32_t* windows, int32_t* blocks, int32_t* cell_off, int32_t* cell_cnt, int32_t* cells, double* z,
                                  double* u, void* stream) {
  GSM_GRID_HANDLE(h);
  if (!chain_state || !is_data || !windows || !blocks || !cell_off || !cell_cnt || !cells || !z || !u)
    return fail(h, GSM_E_ARG, "gsm_sgs_draw_pcg64: NULL pointer");
  if (n_iters < 1 || n_iters > 65535) return fail(h, GSM_E_ARG, "gsm_sgs_draw_pcg64: n_iters must be in [1, 65535]");
  if (int rc = sgs_check_ranges(h, "gsm_sgs_draw_pcg64", min_x, max_x, min_y, max_y, max_cells)) return rc;
  if (h->H > 32767 || h->W > 32767) return fail(h, GSM_E_UNSUPPORTED, "gsm_sgs_draw_pcg64: grid sides up to 32767 (cells are packed as row << 16 | col)");
  if ((int64_t)n_iters * h->n_chains * max_cells >= (1LL << 31)) return fail(h, GSM_E_ARG, "gsm_sgs_draw_pcg64: n_iters * n_chains * max_cells must stay below 2^31 (32-bit cell offsets)");
  HIPCHK(h, hipSetDevice(h->device));
  { int rc = ensure_pcg_tables(h); if (rc) return rc; }
  SgsDrawArgs a{};
  a.H = h->H; a.W = h->W; a.n_chains = h->n_chains; a.n_iters = n_iters; a.iter0 = 0; a.seeds = nullptr;
  a.region_mask = region_mask; a.is_data = is_data; a.min_x = min_x; a.max_x = max_x; a.min_y = min_y; a.max_y = max_y;
  a.max_cells = max_cells; a.mathtab = nullptr;
  a.win = windows; a.blk = blocks; a.cell_off = cell_off; a.cell_cnt = cell_cnt; a.cells = cells; a.z = z; a.u = u; a.err = h->d_err.get();
  HIPCHK(h, launch_sgs_draw_pcg64(a, chain_state, h->d_pcg_tab.get(), h->d_pcg_tab.get() + kPcgJumpWords, (hipStream_t)stream));
  return GSM_OK;
}

extern "C" int gsm_sgs_grid_draw_pcg64(gsm_handle h, uint64_t* states, const int32_t* cells, int32_t n_cells, const uint8_t* has_value,
                                       const double* lower, const double* upper, int32_t draw_kind, int32_t* work, int32_t* path,
                                       double* draws, int32_t path_len, void* stream) {
  GSM_GRID_HANDLE(h);
  const std::string w = "gsm_sgs_grid_draw_pcg64";
  const int64_t n_grid = (int64_t)h->H * h->W;
  if (n_grid > INT32_MAX) return fail(h, GSM_E_ARG, w + ": flat cell indices are 32-bit (H * W < 2^31)");
  if (n_cells < 0 || (int64_t)n_cells > n_grid) return fail(h, GSM_E_ARG, w + ": n_cells must be in [0, H * W]");
  if (path_len < 0 || path_len > n_cells) return fail(h, GSM_E_ARG, w + ": path_len must be in [0, n_cells]");
  if (draw_kind != GSM_DRAW_NORMAL && draw_kind != GSM_DRAW_TRUNCATED) return fail(h, GSM_E_ARG, w + ": draw_kind must be GSM_DRAW_NORMAL or GSM_DRAW_TRUNCATED");
  if (draw_kind == GSM_DRAW_TRUNCATED && (!lower || !upper)) return fail(h, GSM_E_ARG, w + ": GSM_DRAW_TRUNCATED needs both bounds (lower and upper)");
  if (!states || (n_cells > 0 && (!cells || !has_value || !work)) || (path_len > 0 && (!path || !draws))) return fail(h, GSM_E_ARG, w + ": NULL pointer");
  HIPCHK(h, hipSetDevice(h->device));
  { int rc = ensure_pcg_tables(h); if (rc) return rc; }
  hipStream_t st = (hipStream_t)stream;
  SgsGridDrawArgs a{};
  a.H = h->H; a.W = h->W; a.n_real = h->n_chains; a.states = states; a.cells = cells; a.n_cells = n_cells; a.has_value = has_value;
  a.lo = lower; a.hi = upper; a.draw_kind = draw_kind; a.work = work; a.path = path; a.draws = draws; a.path_len = path_len;
  a.jump = h->d_pcg_tab.get(); a.zig = h->d_pcg_tab.get() + kPcgJumpWords; a.err = h->d_err.get();
  HIPCHK(h, launch_sgs_grid_draw_pcg64(a, st));
  return sgs_report_flags(h, st, w, kGridDrawFlags);
}

// scratch of the loss kernels: a partial sum and bad-cell count per (chain, part), and per chain the ticket of sgs_loss_tail_kernel
// (zero between launches: the kernel resets it)
static int sgs_parts_ensure(gsm_handle h) {
  const size_t need = (size_t)h->n_chains * sgs_loss_parts(h->S);
  auto& p = h->sgs_parts;
  if (p.cap >= need) return GSM_OK;
  p = gsm_context::SgsParts();                // cap stays 0 until every buffer of the set exists
  HIPCHK(h, p.sum.ensure(need));
  HIPCHK(h, p.bad.ensure(need));
  HIPCHK(h, p.ticket.ensure((size_t)h->n_chains));
  HIPCHK(h, hipMemset(p.ticket.get(), 0, (size_t)h->n_chains * sizeof(int32_t)));
  p.cap = need;
  return GSM_OK;
}

extern "C" int gsm_sgs_loss(gsm_handle h, const double* beds, const double* trend, double* loss, int32_t* bad, void* stream) {
  GSM_GRID_HANDLE(h);
  if (!h->have_static) return fail(h, GSM_E_STATE, "gsm_sgs_loss: call gsm_set_static first");
  if (h->f32_state) return fail(h, GSM_E_UNSUPPORTED, "gsm_sgs_loss: fp64 beds only");
  if (!beds || !loss || !bad) return fail(h, GSM_E_ARG, "gsm_sgs_loss: NULL pointer");
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = sgs_parts_ensure(h)) return rc;
  HIPCHK(h, launch_sgs_loss(h->S, h->n_chains, beds, trend, loss, bad, h->sgs_parts.sum.get(), h->sgs_parts.bad.get(), h->sgs_group(),
                            (hipStream_t)stream));
  return GSM_OK;
}

extern "C" int gsm_sgs_decide(gsm_handle h, const double* loss_next, const int32_t* bad, const double* u, double* loss_prev,
                              uint8_t* accept, double* loss_rec, uint8_t* acc_rec, int64_t rec_stride, void* stream) {
  GSM_GRID_HANDLE(h);
  if (!loss_next || !bad || !u || !loss_prev || !accept) return fail(h, GSM_E_ARG, "gsm_sgs_decide: NULL pointer");
  if ((loss_rec || acc_rec) && rec_stride < 1) return fail(h, GSM_E_ARG, "gsm_sgs_decide: rec_stride must be >= 1");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, launch_sgs_decide(h->n_chains, loss_next, bad, u, loss_prev, accept, loss_rec, acc_rec, rec_stride, (hipStream_t)stream));
  return GSM_OK;
}

extern "C" int gsm_sgs_state_init(gsm_handle h, const double* beds, const double* trend, double* energy, double* state, void* stream) {
  GSM_GRID_HANDLE(h);
  if (!h->have_static) return fail(h, GSM_E_STATE, "gsm_sgs_state_init: call gsm_set_static first");
  if (h->f32_state) return fail(h, GSM_E_UNSUPPORTED, "gsm_sgs_state_init: fp64 beds only");
  if (!beds || !energy || !state) return fail(h, GSM_E_ARG, "gsm_sgs_state_init: NULL pointer");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, launch_sgs_state_init(h->S, h->n_chains, beds, trend, energy, state, h->sgs_group(), (hipStream_t)stream));
  return GSM_OK;
}

extern "C" int gsm_sgs_finish(gsm_handle h, double* cur, double* next, const double* trend, double* energy, double* state,
                              const int32_t* windows, const double* u, uint32_t* resampled, uint8_t* accept, double* loss_rec,
                              uint8_t* acc_rec, int64_t rec_stride, void* stream) {
  GSM_GRID_HANDLE(h);
  if (!h->have_static) return fail(h, GSM_E_STATE, "gsm_sgs_finish: call gsm_set_static first");
  if (h->f32_state) return fail(h, GSM_E_UNSUPPORTED, "gsm_sgs_finish: fp64 beds only");
  if (!cur || !next || !energy || !state || !windows || !u || !resampled || !accept) return fail(h, GSM_E_ARG, "gsm_sgs_finish: NULL pointer");
  if ((loss_rec || acc_rec) && rec_stride < 1) return fail(h, GSM_E_ARG, "gsm_sgs_finish: rec_stride must be >= 1");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, launch_sgs_finish(h->S, h->n_chains, cur, next, trend, energy, state, windows, u, resampled, accept, loss_rec, acc_rec, rec_stride,
                              h->d_err.get(), h->sgs_group(), (hipStream_t)stream));
  return GSM_OK;
}

extern "C" int gsm_sgs_commit_map(gsm_handle h, double* cur, const double* proposed, uint32_t* resampled, const int32_t* windows,
                                  const uint8_t* accept, void* stream) {
  GSM_GRID_HANDLE(h);
  if (!cur || !proposed || !resampled || !windows || !accept) return fail(h, GSM_E_ARG, "gsm_sgs_commit_map: NULL pointer");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, launch_sgs_commit_map(h->H, h->W, h->n_chains, cur, proposed, resampled, windows, accept, (hipStream_t)stream));
  return GSM_OK;
}

extern "C" int gsm_sgs_commit(gsm_handle h, double* cur, double* next, uint32_t* resampled, const int32_t* windows,
                              const uint8_t* accept, void* stream) {
  GSM_GRID_HANDLE(h);
  if (!cur || !next || !resampled || !windows || !accept) return fail(h, GSM_E_ARG, "gsm_sgs_commit: NULL pointer");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, launch_sgs_commit(h->H, h->W, h->n_chains, cur, next, resampled, windows, accept, (hipStream_t)stream));
  return GSM_OK;
}

// ---- one batch of small-scale iterations in ONE call ------------------------------------------------------------------------
static int sgs_issue(gsm_handle h, const gsm_sgs_batch* b, int32_t n_iters, void* st) {
  const int64_t n = h->n_chains;
  const bool qt = b->qt_n > 0;
  const int64_t map = n * (int64_t)h->H * h->W;
  hipStream_t main_st = (hipStream_t)st;
  // The kriging weights of an iteration do not depend on the values of the grid, only on where values are: when the caller
  // promises that every cell holds one (grid_finite), the records of the iterations ahead (sgs_rank_kernel, sgs_weights_kernel) are made on a
  // second stream while the current iteration runs its value pass, transforms, loss and decision -- the longest kernel of an iteration
  // leaves the critical path.  `depth` sets of record scratch (iteration j uses set j mod depth; <= 512 MiB in all): the second stream
  // runs up to depth - 1 iterations ahead and waits for the main stream only every depth / 2 iterations -- a wait between two kernels of
  // a stream costs ~10 us even when it is satisfied (rocprofv3 timeline of the two-set version), more than a quarter of the kernel it precedes.
  const bool overlap = b->grid_finite != 0 && n_iters > 1;
  int depth = 1;
  if (overlap) {
    const size_t set_bytes = (size_t)n * (size_t)((b->max_cells + 63) & ~63) * (sizeof(SgsCellHdr) + 48 * sizeof(double2)) + (size_t)n * 4100;
    depth = (int)std::min<size_t>(gsm_context::kSgsDepth, std::max<size_t>(2, ((size_t)512 << 20) / std::max<size_t>(set_bytes, 1)));
    depth = std::min(depth, (int)n_iters);
    if (depth >= 4) depth &= ~1;                                      // an even depth: the waits fall every depth / 2 iterations
  }
  if (overlap) {                                             // created by the first overlapped batch of the handle
    HIPCHK(h, h->sgs_side.ensure(hipStreamNonBlocking));
    HIPCHK(h, h->sgs_side2.ensure(hipStreamNonBlocking));
    for (Event& e : h->sgs_ev) HIPCHK(h, e.ensure(hipEventDisableTiming));
  }
  // two record streams, even and odd iterations: with few chains a launch of sgs_weights_kernel leaves most of the chip idle
  hipStream_t rec_st[2] = {h->sgs_side.get(), depth >= 4 ? h->sgs_side2.get() : h->sgs_side.get()};
  bool must_wait[2] = {false, false};                         // the stream has not yet been told of the main stream's latest sync point
  auto fill = [&](int32_t j, SgsArgs& a) -> int {
    const int64_t base = b->cell_base ? b->cell_base[j] : 0;
    int rc = sgs_fill(h, a, b->next, b->zcond, b->windows + 4 * n * j, b->x_axis, b->y_axis, b->lag_cov, b->lag_mi, b->lag_mj, b->hw, b->radius,
                      b->num_points, b->sill, b->cell_off + b->cell_off_stride * j, b->cells + 2 * base, b->z + base, b->max_cells,
                      "gsm_sgs_iterate", overlap ? (j % depth) : 0);
    if (rc) return rc;
    a.cell_cnt = b->cell_cnt ? b->cell_cnt + n * j : nullptr; a.trace = nullptr; a.nbr_trace = nullptr;
    a.defer = overlap ? 1 : 0;
    return GSM_OK;
  };
  const Event* ev_w = h->sgs_ev;                                    // [depth] the records of set s are complete
  hipEvent_t ev_fork = h->sgs_ev[gsm_context::kSgsDepth].get();    // the draws are there
  hipEvent_t ev_seq = h->sgs_ev[gsm_context::kSgsDepth + 1].get(); // the main stream has finished the value pass of some iteration
  std::vector<SgsArgs> args(overlap ? n_iters : 1);
  int rc;
  const int half = std::max(1, depth / 2);
  int32_t issued = 0;                                         // iterations whose records have been enqueued on the second stream
  auto enqueue_records = [&](int32_t upto) -> int {          // records of iterations issued .. upto - 1
    for (; issued < upto; ++issued) {
      const int q = issued & 1;
      if (must_wait[q]) { HIPCHK(h, hipStreamWaitEvent(rec_st[q], ev_seq, 0)); must_wait[q] = false; if (rec_st[0] == rec_st[1]) must_wait[q ^ 1] = false; }
      HIPCHK(h, launch_sgs_weights(args[issued], args[issued].max_cells, rec_st[q]));
      HIPCHK(h, hipEventRecord(ev_w[issued % depth].get(), rec_st[q]));
    }
    return GSM_OK;
  };
  if (overlap) {
    for (int32_t j = 0; j < n_iters; ++j)
      if ((rc = fill(j, args[j]))) return rc;                 // every set of scratch exists before anything is enqueued
    HIPCHK(h, hipEventRecord(ev_fork, main_st));              // fork: whatever made the draws is on the main stream
    HIPCHK(h, hipStreamWaitEvent(rec_st[0], ev_fork, 0));
    if (rec_st[1] != rec_st[0] && n_iters > 1) HIPCHK(h, hipStreamWaitEvent(rec_st[1], ev_fork, 0));
    if ((rc = enqueue_records(std::min<int32_t>(n_iters, depth - 1 > 0 ? depth - 1 : 1)))) return rc;
  }
  // with a transformer: both transforms of an iteration inside the tail launch where its tables and the map's parts fit
  // (sgs_loss_tail_kernel<true>); the forward transform of the batch's first iteration is the stand-alone launch
  // Measured (same box): 16 chains +4.8 %, 32 chains +9.5 %, 64 chains +4.1 %, 256 chains +2.9 %, 8 chains -7 %, 4 chains -19 % (a thread of the tail launch then makes ~8 transforms one after
  // the other where the stand-alone launches make one per thread: with a few chains latency is what counts).  batch->tail_qt = GSM_TAIL_QT_ON / GSM_TAIL_QT_OFF forces.
  const bool tail_qt_wanted = b->tail_qt == GSM_TAIL_QT_AUTO ? h->n_chains >= 12 : b->tail_qt == GSM_TAIL_QT_ON;
  const bool tail_qt = qt && !b->windowed && tail_qt_wanted && h->have_static && sgs_tail_takes_qt(h->S, b->qt_n);
  const auto [qt_clip_min, qt_clip_max] = tail_qt ? qt_clip() : std::pair<double, double>(0.0, 0.0);
  if (tail_qt) HIPCHK(h, h->d_sgs_next_acc.ensure((size_t)map));
  for (int32_t j = 0; j < n_iters; ++j) {
    const int32_t* win = b->windows + 4 * n * j;
    const double* u = b->u + n * j;
    if (qt && (!tail_qt || j == 0) && (rc = gsm_qt_transform(h, b->qt_quantiles, b->qt_references, b->qt_n, b->cur, b->next, map, 0, st))) return rc;   // MCMC.py:1766
    if (overlap) {
      HIPCHK(h, hipStreamWaitEvent(main_st, ev_w[j % depth].get(), 0));
      HIPCHK(h, launch_sgs_sequence(args[j], main_st));
      // set j mod depth is free again once this value pass is over: every `half` iterations the second stream is told so and
      // takes the next `half` iterations' records (it then runs between depth - half and depth - 1 iterations ahead)
      if ((j + 1) % half == 0 && issued < n_iters) {
        HIPCHK(h, hipEventRecord(ev_seq, main_st));
        must_wait[0] = must_wait[1] = true;                    // (a stream waits when it next gets work)
        if ((rc = enqueue_records(std::min<int32_t>(n_iters, j + depth)))) return rc;
      }
    } else {
      if ((rc = fill(j, args[0]))) return rc;
      HIPCHK(h, launch_sgs_blocks(args[0], args[0].max_cells, main_st));
    }
    if (b->windowed) {
      if ((rc = gsm_sgs_finish(h, b->cur, b->next, b->trend, b->energy, b->state, win, u, b->resampled, b->accept,
                               b->loss_rec ? b->loss_rec + j : nullptr, b->acc_rec ? b->acc_rec + j : nullptr, n_iters, st))) return rc;
      continue;
    }
    if (qt && !tail_qt && (rc = gsm_qt_transform(h, b->qt_quantiles, b->qt_references, b->qt_n, b->next, b->proposed, map, 1, st))) return rc;  // MCMC.py:1777
    // loss of the proposal, decision and commit (gsm_sgs_loss, gsm_sgs_decide, gsm_sgs_commit_map / gsm_sgs_commit) in one launch
    if (!h->have_static) return fail(h, GSM_E_STATE, "gsm_sgs_iterate: call gsm_set_static first");
    if (h->f32_state) return fail(h, GSM_E_UNSUPPORTED, "gsm_sgs_iterate: fp64 beds only");
    if ((rc = sgs_parts_ensure(h))) return rc;
    SgsTailArgs t{};
    t.group = h->sgs_group(); t.trend = b->trend; t.part_sum = h->sgs_parts.sum.get(); t.part_bad = h->sgs_parts.bad.get(); t.ticket = h->sgs_parts.ticket.get();
    t.loss = b->loss; t.bad = b->bad; t.u = u; t.loss_prev = b->loss_prev; t.accept = b->accept;
    t.loss_rec = b->loss_rec ? b->loss_rec + j : nullptr; t.acc_rec = b->acc_rec ? b->acc_rec + j : nullptr; t.rec_stride = n_iters;
    t.mode = qt ? 1 : 2; t.cur = b->cur; t.beds = qt ? b->proposed : b->next; t.resampled = b->resampled; t.win = win;
    t.qt_q = tail_qt ? b->qt_quantiles : nullptr; t.qt_ref = b->qt_references; t.qt_n = b->qt_n; t.clip_min = qt_clip_min; t.clip_max = qt_clip_max;
    t.next = b->next; t.next_acc = h->d_sgs_next_acc.get();
    HIPCHK(h, launch_sgs_loss_tail(h->S, h->n_chains, t, main_st));
  }
  return GSM_OK;
}

extern "C" int gsm_sgs_iterate(gsm_handle h, const gsm_sgs_batch* b, int32_t n_iters, void* stream) {
  GSM_GRID_HANDLE(h);
  if (!b || n_iters < 1) return fail(h, GSM_E_ARG, "gsm_sgs_iterate: NULL batch / n_iters < 1");
  if (!b->cur || !b->next || !b->windows || !b->cell_off || !b->cells || !b->z || !b->u || !b->resampled || !b->accept)
    return fail(h, GSM_E_ARG, "gsm_sgs_iterate: NULL pointer");
  if (b->qt_n < 0 || (b->qt_n > 0 && (!b->qt_quantiles || !b->qt_references || !b->proposed)))
    return fail(h, GSM_E_ARG, "gsm_sgs_iterate: a transformer needs qt_quantiles, qt_references and the `proposed` planes");
  if (b->windowed && (b->qt_n > 0 || !b->energy || !b->state))
    return fail(h, GSM_E_ARG, "gsm_sgs_iterate: the windowed finish needs energy / state and no transformer");
  if (!b->windowed && (!b->loss || !b->bad || !b->loss_prev)) return fail(h, GSM_E_ARG, "gsm_sgs_iterate: loss / bad / loss_prev are NULL");
  if (b->cell_off_stride < h->n_chains) return fail(h, GSM_E_ARG, "gsm_sgs_iterate: cell_off_stride must be >= n_chains");
  if (b->tail_qt < GSM_TAIL_QT_AUTO || b->tail_qt > GSM_TAIL_QT_OFF) return fail(h, GSM_E_ARG, "gsm_sgs_iterate: tail_qt must be GSM_TAIL_QT_AUTO, _ON or _OFF");
  HIPCHK(h, hipSetDevice(h->device));
  return sgs_issue(h, b, n_iters, stream);
}
