// C ABI of libgsm_hip.so, the posterior accumulator (posterior_kernel.hip, posterior_hist_kernel.hip, posterior_lag_kernel.hip,
// posterior_cov_kernel.hip, posterior_residual_kernel.hip, posterior_local_kernel.hip, posterior_regions_kernel.hip).  Every
// argument is validated here, once, where the error text is; the launchers take what they are given.
#include "gsm_context.h"
#include "posterior_device.h"
#include <cmath>

using namespace gsm;

// selects the device and makes sure h->n_cu is known (grid sizing, the cut of the chain axis)
static int posterior_device(gsm_handle h) {
  HIPCHK(h, hipSetDevice(h->device));
  if (!h->n_cu) {
    HIPCHK(h, hipDeviceGetAttribute(&h->n_cu, hipDeviceAttributeMultiprocessorCount, h->device));
    if (h->n_cu < 1) h->n_cu = 1;
  }
  return GSM_OK;
}

// *parts of the chain axis for a pass of plane / vec cells per chain, and the slab of *parts x n_fields planes
static int posterior_slab(gsm_handle h, int vec, int n_fields, int* parts) {
  int rc = posterior_device(h);
  if (rc != GSM_OK) return rc;
  const int64_t plane = (int64_t)h->H * h->W;
  *parts = posterior_parts(posterior_cell_blocks(plane, vec), h->n_chains, h->n_cu);
  HIPCHK(h, h->d_post_slab.ensure((size_t)*parts * n_fields * plane));
  return GSM_OK;
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static int posterior_sample(gsm_handle h, const char* who, const void* beds, const int32_t* sample_cells, int32_t n_samples,
                            double* sample_out, hipStream_t st) {
  if (!sample_out) return GSM_OK;
  if (!sample_cells || n_samples < 1) return fail(h, GSM_E_ARG, std::string(who) + ": sample_out without sample_cells / n_samples >= 1");
  HIPCHK(h, launch_posterior_sample(beds, sample_cells, n_samples, h->n_chains, (int64_t)h->H * h->W, h->f32_state, sample_out, st));
  return GSM_OK;
}

extern "C" int gsm_posterior_accumulate(gsm_handle h, const void* beds, void* ref, double* s1, double* s2, int32_t first,
                                        const int32_t* sample_cells, int32_t n_samples, double* sample_out, void* stream) {
  GSM_GRID_HANDLE(h);
  if (!beds || !ref || !s1 || !s2) return fail(h, GSM_E_ARG, "gsm_posterior_accumulate: NULL pointer");
  if (!aligned16(beds) || !aligned16(ref) || !aligned16(s1) || !aligned16(s2))
    return fail(h, GSM_E_ARG, "gsm_posterior_accumulate: beds, ref, s1 and s2 must be 16-byte aligned");
  int rc = posterior_device(h);
  if (rc != GSM_OK) return rc;
  HIPCHK(h, launch_posterior_accumulate(beds, ref, s1, s2, (int64_t)h->n_chains * h->H * h->W, h->f32_state, first != 0, h->n_cu,
                                        (hipStream_t)stream));
  return posterior_sample(h, "gsm_posterior_accumulate", beds, sample_cells, n_samples, sample_out, (hipStream_t)stream);
}

extern "C" int gsm_posterior_accumulate_pooled(gsm_handle h, const void* beds, const double* g, double* s1, double* s2,
                                               const int32_t* sample_cells, int32_t n_samples, double* sample_out, void* stream) {
  GSM_GRID_HANDLE(h);
  if (!beds || !g || !s1 || !s2) return fail(h, GSM_E_ARG, "gsm_posterior_accumulate_pooled: NULL pointer");
  if (!aligned16(beds)) return fail(h, GSM_E_ARG, "gsm_posterior_accumulate_pooled: beds must be 16-byte aligned");
  const int64_t plane = (int64_t)h->H * h->W;
  int parts = 1;
  int rc = posterior_slab(h, posterior_vec(plane, h->f32_state), 2, &parts);
  if (rc != GSM_OK) return rc;
  HIPCHK(h, launch_posterior_pooled(beds, g, s1, s2, h->d_post_slab.get(), plane, h->n_chains, parts, h->f32_state, h->n_cu, (hipStream_t)stream));
  return posterior_sample(h, "gsm_posterior_accumulate_pooled", beds, sample_cells, n_samples, sample_out, (hipStream_t)stream);
}

extern "C" int gsm_posterior_sample(gsm_handle h, const void* beds, const int32_t* sample_cells, int32_t n_samples, double* sample_out,
                                    void* stream) {
  GSM_GRID_HANDLE(h);
  if (!beds || !sample_out) return fail(h, GSM_E_ARG, "gsm_posterior_sample: NULL pointer");
  HIPCHK(h, hipSetDevice(h->device));
  return posterior_sample(h, "gsm_posterior_sample", beds, sample_cells, n_samples, sample_out, (hipStream_t)stream);
}

extern "C" int gsm_posterior_close(gsm_handle h, const void* ref, const double* g, double* s1, double* s2, int32_t n_per_seq, void* stream) {
  GSM_GRID_HANDLE(h);
  if (!ref || !g || !s1 || !s2) return fail(h, GSM_E_ARG, "gsm_posterior_close: NULL pointer");
  if (n_per_seq < 2) return fail(h, GSM_E_ARG, "gsm_posterior_close: n_per_seq must be >= 2 (a variance needs two snapshots)");
  if (h->n_chains > 65535) return fail(h, GSM_E_UNSUPPORTED, "gsm_posterior_close: more than 65535 chains");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, launch_posterior_close(ref, g, s1, s2, (int64_t)h->H * h->W, h->n_chains, n_per_seq, h->f32_state, (hipStream_t)stream));
  return GSM_OK;
}

extern "C" int gsm_posterior_histogram(gsm_handle h, const void* beds, const double* g, double inv_width, int32_t n_bins, const double* levels,
                                       int32_t n_levels, int32_t* counts, void* stream) {
  GSM_GRID_HANDLE(h);
  if (!beds || !g || !counts) return fail(h, GSM_E_ARG, "gsm_posterior_histogram: NULL pointer");
  if (n_bins < 2 || n_bins > kHistMaxBins || n_bins % 2) return fail(h, GSM_E_ARG, "gsm_posterior_histogram: n_bins must be even and in [2, 128]");
  if (n_levels < 0 || n_levels > kHistMaxLevels) return fail(h, GSM_E_ARG, "gsm_posterior_histogram: n_levels must be in [0, 8]");
  if (n_levels > 0 && !levels) return fail(h, GSM_E_ARG, "gsm_posterior_histogram: NULL levels with n_levels > 0");
  if (!(inv_width > 0.0) || !std::isfinite(inv_width)) return fail(h, GSM_E_ARG, "gsm_posterior_histogram: inv_width must be finite and > 0");
  int rc = posterior_device(h);
  if (rc != GSM_OK) return rc;
  HIPCHK(h, launch_posterior_histogram(beds, g, inv_width, n_bins, levels, n_levels, counts, (int64_t)h->H * h->W, h->n_chains, h->f32_state, h->n_cu,
                                       (hipStream_t)stream));
  return GSM_OK;
}

extern "C" int gsm_posterior_lagged(gsm_handle h, const void* beds, void* ring, int32_t n_lags, int32_t head, int32_t n_valid,
                                    double* lag_sqdiff, void* stream) {
  GSM_GRID_HANDLE(h);
  if (!beds || !ring || !lag_sqdiff) return fail(h, GSM_E_ARG, "gsm_posterior_lagged: NULL pointer");
  if (n_lags < 1 || n_lags > kLagMaxLags) return fail(h, GSM_E_ARG, "gsm_posterior_lagged: n_lags must be in [1, 15]");
  if (head < 0 || head >= n_lags) return fail(h, GSM_E_ARG, "gsm_posterior_lagged: head must be in [0, n_lags)");
  if (n_valid < 0 || n_valid > n_lags) return fail(h, GSM_E_ARG, "gsm_posterior_lagged: n_valid must be in [0, n_lags]");
  if (!aligned16(beds) || !aligned16(ring)) return fail(h, GSM_E_ARG, "gsm_posterior_lagged: beds and ring must be 16-byte aligned");
  const int64_t plane = (int64_t)h->H * h->W;
  int parts = 1;
  int rc = posterior_slab(h, posterior_vec(plane, h->f32_state), n_lags, &parts);
  if (rc != GSM_OK) return rc;
  HIPCHK(h, launch_posterior_lagged(beds, ring, h->d_post_slab.get(), lag_sqdiff, plane, h->n_chains, parts, n_lags, head, n_valid, h->f32_state,
                                    h->n_cu, (hipStream_t)stream));
  return GSM_OK;
}

// the slab of the two covariance passes, sized for the larger of them so that their alternating calls never reallocate it:
// project holds n_chains * plane parts * n_probes partial projections, cross *parts x n_probes planes
static int posterior_cov_slab(gsm_handle h, int n_probes, int* parts) {
  int rc = posterior_device(h);
  if (rc != GSM_OK) return rc;
  const int64_t plane = (int64_t)h->H * h->W;
  *parts = posterior_parts(posterior_cell_blocks(plane, posterior_vec(plane, h->f32_state)), h->n_chains, h->n_cu);
  const size_t project = (size_t)h->n_chains * posterior_project_parts(plane, h->n_chains, h->n_cu) * n_probes;
  HIPCHK(h, h->d_post_slab.ensure(std::max(project, (size_t)*parts * n_probes * plane)));
  return GSM_OK;
}

extern "C" int gsm_posterior_project(gsm_handle h, const void* beds, const double* g, const double* probes, int32_t n_probes, double* proj,
                                     void* stream) {
  GSM_GRID_HANDLE(h);
  if (!beds || !g || !probes || !proj) return fail(h, GSM_E_ARG, "gsm_posterior_project: NULL pointer");
  if (n_probes < 1 || n_probes > kLagMaxLags) return fail(h, GSM_E_ARG, "gsm_posterior_project: n_probes must be in [1, 15]");
  if (!aligned16(beds)) return fail(h, GSM_E_ARG, "gsm_posterior_project: beds must be 16-byte aligned");
  if (h->n_chains > 65535) return fail(h, GSM_E_UNSUPPORTED, "gsm_posterior_project: more than 65535 chains");
  int parts = 1;
  int rc = posterior_cov_slab(h, n_probes, &parts);
  if (rc != GSM_OK) return rc;
  HIPCHK(h, launch_posterior_project(beds, g, probes, h->d_post_slab.get(), proj, (int64_t)h->H * h->W, h->n_chains, n_probes, h->f32_state,
                                     h->n_cu, (hipStream_t)stream));
  return GSM_OK;
}

extern "C" int gsm_posterior_cross(gsm_handle h, const void* beds, const double* g, const double* proj, int32_t n_probes, double* cross,
                                   void* stream) {
  GSM_GRID_HANDLE(h);
  if (!beds || !g || !proj || !cross) return fail(h, GSM_E_ARG, "gsm_posterior_cross: NULL pointer");
  if (n_probes < 1 || n_probes > kLagMaxLags) return fail(h, GSM_E_ARG, "gsm_posterior_cross: n_probes must be in [1, 15]");
  if (!aligned16(beds)) return fail(h, GSM_E_ARG, "gsm_posterior_cross: beds must be 16-byte aligned");
  int parts = 1;
  int rc = posterior_cov_slab(h, n_probes, &parts);
  if (rc != GSM_OK) return rc;
  HIPCHK(h, launch_posterior_cross(beds, g, proj, h->d_post_slab.get(), cross, (int64_t)h->H * h->W, h->n_chains, parts, n_probes, h->f32_state,
                                   h->n_cu, (hipStream_t)stream));
  return GSM_OK;
}

extern "C" int gsm_posterior_residual(gsm_handle h, const void* beds, const double* rg, const double* levels, int32_t n_levels,
                                      double* sums, void* stream) {
  GSM_GRID_HANDLE(h);
  if (!beds || !rg || !sums) return fail(h, GSM_E_ARG, "gsm_posterior_residual: NULL pointer");
  if (n_levels < 0 || n_levels > kResMaxLevels) return fail(h, GSM_E_ARG, "gsm_posterior_residual: n_levels must be in [0, 4]");
  if (n_levels > 0 && !levels) return fail(h, GSM_E_ARG, "gsm_posterior_residual: NULL levels with n_levels > 0");
  for (int l = 0; l < n_levels; ++l)
    if (!(levels[l] >= 0.0) || !std::isfinite(levels[l])) return fail(h, GSM_E_ARG, "gsm_posterior_residual: levels must be finite and >= 0");
  if (!aligned16(beds)) return fail(h, GSM_E_ARG, "gsm_posterior_residual: beds must be 16-byte aligned");
  if (!h->have_static) return fail(h, GSM_E_STATE, "gsm_posterior_residual: call gsm_set_static first");
  int rc = posterior_device(h);
  if (rc != GSM_OK) return rc;
  const int parts = posterior_residual_parts(posterior_residual_tile(h->H, h->W, h->f32_state), h->n_chains, h->n_cu);
  HIPCHK(h, h->d_post_slab.ensure((size_t)parts * (3 + n_levels) * h->H * h->W));
  HIPCHK(h, launch_posterior_residual(h->S, beds, rg, levels, n_levels, h->d_post_slab.get(), sums, h->n_chains, parts, h->f32_state, h->n_cu,
                                      (hipStream_t)stream));
  return GSM_OK;
}

extern "C" int gsm_posterior_local(gsm_handle h, const void* beds, const double* g, int32_t reach, double* cross, void* stream) {
  GSM_GRID_HANDLE(h);
  if (!beds || !g || !cross) return fail(h, GSM_E_ARG, "gsm_posterior_local: NULL pointer");
  if (reach < 1 || reach > kLocalMaxReach) return fail(h, GSM_E_ARG, "gsm_posterior_local: reach must be in [1, 4]");
  if (!aligned16(beds)) return fail(h, GSM_E_ARG, "gsm_posterior_local: beds must be 16-byte aligned");
  int rc = posterior_device(h);
  if (rc != GSM_OK) return rc;
  const int K = 2 * reach * reach + 2 * reach;
  const int parts = posterior_local_parts(h->H, h->W, reach, h->n_chains, h->n_cu);
  if (parts < 1)
    return fail(h, GSM_E_UNSUPPORTED, "gsm_posterior_local: the K planes of one part of the chain axis exceed the 1 GiB the part merge may take: "
                                      "use a shorter reach");
  if (posterior_local_tiles(h->H, h->W) * parts > INT32_MAX) return fail(h, GSM_E_UNSUPPORTED, "gsm_posterior_local: more than 2^31 - 1 workgroups");
  HIPCHK(h, h->d_post_slab.ensure((size_t)parts * K * h->H * h->W));
  HIPCHK(h, launch_posterior_local(beds, g, h->d_post_slab.get(), cross, h->H, h->W, h->n_chains, parts, reach, h->f32_state, h->n_cu,
                                   (hipStream_t)stream));
  return GSM_OK;
}

extern "C" int gsm_posterior_regions(gsm_handle h, const void* beds, const uint8_t* region_bits, int32_t n_regions, double sea_level,
                                     double density_ratio, double* func, double hyps_lo, double hyps_inv_width, int32_t n_bins,
                                     int32_t* hyps, void* stream) {
  GSM_GRID_HANDLE(h);
  if (!beds || !region_bits || !func) return fail(h, GSM_E_ARG, "gsm_posterior_regions: NULL pointer");
  if (n_regions < 1 || n_regions > kRegMaxRegions) return fail(h, GSM_E_ARG, "gsm_posterior_regions: n_regions must be in [1, 8]");
  if (n_bins != 0 && (n_bins < 2 || n_bins > kRegMaxBins || n_bins % 2))
    return fail(h, GSM_E_ARG, "gsm_posterior_regions: n_bins must be 0 or even and in [2, 64]");
  if (n_bins > 0 && !hyps) return fail(h, GSM_E_ARG, "gsm_posterior_regions: NULL hyps with n_bins > 0");
  if (!std::isfinite(sea_level)) return fail(h, GSM_E_ARG, "gsm_posterior_regions: sea_level must be finite");
  if (!(density_ratio > 0.0) || !std::isfinite(density_ratio))
    return fail(h, GSM_E_ARG, "gsm_posterior_regions: density_ratio must be finite and > 0");
  if (n_bins > 0 && (!(hyps_inv_width > 0.0) || !std::isfinite(hyps_inv_width) || !std::isfinite(hyps_lo)))
    return fail(h, GSM_E_ARG, "gsm_posterior_regions: hyps_inv_width must be finite and > 0 and hyps_lo finite");
  if (!aligned16(beds)) return fail(h, GSM_E_ARG, "gsm_posterior_regions: beds must be 16-byte aligned");
  if (!h->have_static) return fail(h, GSM_E_STATE, "gsm_posterior_regions: call gsm_set_static first");
  if (h->n_chains > 65535) return fail(h, GSM_E_UNSUPPORTED, "gsm_posterior_regions: more than 65535 chains");
  int rc = posterior_device(h);
  if (rc != GSM_OK) return rc;
  const int64_t plane = (int64_t)h->H * h->W;
  HIPCHK(h, h->d_post_slab.ensure((size_t)h->n_chains * posterior_regions_parts(plane, h->n_chains, h->f32_state, h->n_cu) * n_regions * 8));
  HIPCHK(h, launch_posterior_regions(beds, h->S.surf, region_bits, n_regions, sea_level, density_ratio, h->d_post_slab.get(), func, hyps_lo,
                                     hyps_inv_width, n_bins, hyps, plane, h->n_chains, h->f32_state, h->n_cu, (hipStream_t)stream));
  return GSM_OK;
}

extern "C" int gsm_posterior_partials(gsm_handle h, const void* ref, const double* g, const double* s1, const double* s2,
                                      int32_t n_seq_per_chain, int64_t seq_stride, int32_t n_closed, int32_t n_per_seq, double* partials,
                                      void* stream) {
  GSM_GRID_HANDLE(h);
  if (!ref || !g || !s1 || !s2 || !partials) return fail(h, GSM_E_ARG, "gsm_posterior_partials: NULL pointer");
  if (n_seq_per_chain != 1 && n_seq_per_chain != 2) return fail(h, GSM_E_ARG, "gsm_posterior_partials: n_seq_per_chain must be 1 or 2");
  if (n_per_seq < 2) return fail(h, GSM_E_ARG, "gsm_posterior_partials: n_per_seq must be >= 2 (a variance needs two snapshots)");
  if (n_closed < 0 || n_closed > n_seq_per_chain) return fail(h, GSM_E_ARG, "gsm_posterior_partials: n_closed must be in [0, n_seq_per_chain]");
  const int64_t plane = (int64_t)h->H * h->W;
  if (n_seq_per_chain == 2 && seq_stride < (int64_t)h->n_chains * plane)
    return fail(h, GSM_E_ARG, "gsm_posterior_partials: seq_stride smaller than n_chains * H * W");
  int parts = 1;
  int rc = posterior_slab(h, 1, 3, &parts);
  if (rc != GSM_OK) return rc;
  HIPCHK(h, launch_posterior_partials(ref, g, s1, s2, h->d_post_slab.get(), partials, plane, h->n_chains, n_seq_per_chain, seq_stride, n_closed, n_per_seq,
                                      parts, h->f32_state, h->n_cu, (hipStream_t)stream));
  return GSM_OK;
}
