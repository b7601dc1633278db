// C ABI of libgsm_hip.so, the variogram map of gridded fields (variogram_kernel.hip).
#include "gsm_context.h"
#include <algorithm>

using namespace gsm;

extern "C" int gsm_variogram_map(gsm_handle h, const double* fields, int32_t n_fields, const uint8_t* mask, int32_t mi, int32_t mj,
                                 int32_t rows_per_part, double* sum, int64_t* count, void* stream) {
  GSM_GRID_HANDLE(h);
  if (!fields || !sum || !count) return fail(h, GSM_E_ARG, "gsm_variogram_map: NULL pointer (fields, sum, count)");
  if (n_fields < 1) return fail(h, GSM_E_ARG, "gsm_variogram_map: n_fields must be >= 1");
  if (mi < 0 || mj < 0) return fail(h, GSM_E_ARG, "gsm_variogram_map: mi and mj must be >= 0");
  if (rows_per_part < 0) return fail(h, GSM_E_ARG, "gsm_variogram_map: rows_per_part must be >= 0 (0 = library default)");
  const int H = h->H, W = h->W;
  if (mi > kVariogramMaxLag || mj > kVariogramMaxLag || variogram_workgroups(mi, mj) > (1 << 26))
    return fail(h, GSM_E_UNSUPPORTED, "gsm_variogram_map: offset table too large (mi, mj <= 2^20 and (mi / 4 + 1) * (mj / 32 + 1) <= 2^26)");
  const int rpp = std::min(H, rows_per_part ? rows_per_part : variogram_default_rows_per_part(H, W, mi, mj));
  const int parts = variogram_parts(H, rpp);
  if (parts > 65535) return fail(h, GSM_E_ARG, "gsm_variogram_map: more than 65535 parts (raise rows_per_part)");
  HIPCHK(h, hipSetDevice(h->device));
  // fields per launch: the grid's z extent, and with several parts a slab of partials of at most 256 MiB (or one field's).  A field's
  // result does not depend on which launch carries it.
  const int64_t n_off = (int64_t)(mi + 1) * (2 * (int64_t)mj + 1);
  int64_t per_launch = 65535;
  if (parts > 1) per_launch = std::clamp<int64_t>((int64_t(256) << 20) / (16 * n_off * parts), 1, per_launch);
  per_launch = std::min<int64_t>(per_launch, n_fields);
  if (parts > 1) {
    const size_t need = (size_t)per_launch * parts * n_off;
    HIPCHK(h, h->d_vario_sum.ensure(need));
    HIPCHK(h, h->d_vario_count.ensure(need));
  }
  for (int64_t r0 = 0; r0 < n_fields; r0 += per_launch) {
    const int n = (int)std::min<int64_t>(per_launch, n_fields - r0);
    HIPCHK(h, launch_variogram_map(fields + r0 * H * W, n, mask, H, W, mi, mj, rpp, h->d_vario_sum.get(), h->d_vario_count.get(),
                                   sum + r0 * n_off, count + r0 * n_off, (hipStream_t)stream));
  }
  return GSM_OK;
}

extern "C" int gsm_variogram_local(gsm_handle h, const double* fields, int32_t n_fields, const uint8_t* mask, int32_t mi, int32_t mj,
                                   int32_t tile, int32_t half_window, double* sum, int64_t* count, void* stream) {
  GSM_GRID_HANDLE(h);
  if (!fields || !sum || !count) return fail(h, GSM_E_ARG, "gsm_variogram_local: NULL pointer (fields, sum, count)");
  if (n_fields < 1) return fail(h, GSM_E_ARG, "gsm_variogram_local: n_fields must be >= 1");
  if (mi < 0 || mj < 0) return fail(h, GSM_E_ARG, "gsm_variogram_local: mi and mj must be >= 0");
  if (tile < 2) return fail(h, GSM_E_ARG, "gsm_variogram_local: tile must be >= 2");
  if (half_window < 0) return fail(h, GSM_E_ARG, "gsm_variogram_local: half_window must be >= 0");
  const int H = h->H, W = h->W;
  const int T = std::min(tile, std::max(H, W));               // a tile beyond the grid is one tile, as any tile >= the grid
  const int64_t Ty = (H + T - 1) / T, Tx = (W + T - 1) / T;
  const int k = (int)std::min<int64_t>(half_window, std::max(Ty, Tx));     // a window beyond the lattice is the whole lattice
  if (mi > kVariogramMaxLag || mj > kVariogramMaxLag)
    return fail(h, GSM_E_UNSUPPORTED, "gsm_variogram_local: offset table too large (mi, mj <= 2^20)");
  const int64_t n_off = (int64_t)(mi + 1) * (2 * (int64_t)mj + 1);
  const int64_t per_field = Ty * Tx * n_off;
  if (per_field > (int64_t(1) << 31))
    return fail(h, GSM_E_UNSUPPORTED, "gsm_variogram_local: more than 2^31 entries per field (" + std::to_string(Ty) + " x " + std::to_string(Tx) +
                                          " tiles x " + std::to_string(n_off) + " offsets)");
  if (Ty > 65535 || variogram_local_workgroups(mi, mj, (int)Tx) > (int64_t(1) << 30) || (n_off + 255) / 256 * Ty * Tx > (int64_t(1) << 30) ||
      (int64_t)std::min(T + 1, H) * std::min(T, W) >= (int64_t(1) << 31))
    return fail(h, GSM_E_UNSUPPORTED, "gsm_variogram_local: grid beyond the launch geometry (at most 65535 tile rows, 2^30 workgroups per "
                                      "tile row and field, 2^31 cells per tile)");
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  // fields per launch: the grid's z extent, and with windows a scratch of tile tables of at most 1 GiB (or one field's).  A field's
  // result does not depend on which launch carries it.
  int64_t per_launch = 65535;
  if (k > 0) per_launch = std::clamp<int64_t>((int64_t(1) << 30) / (16 * per_field), 1, per_launch);
  per_launch = std::min<int64_t>(per_launch, n_fields);
  DevBuf<char> scratch;                                       // tile tables of one launch: sums, then counts
  if (k > 0) {
    const size_t bytes = (size_t)per_launch * per_field * 16;
    hipError_t e = scratch.ensure(bytes);
    if (e != hipSuccess) return fail(h, GSM_E_HIP, "gsm_variogram_local: tile tables of " + std::to_string(bytes) + " bytes: " + hipGetErrorString(e));
  }
  double* tsum = (double*)scratch.get();
  int64_t* tcount = k > 0 ? (int64_t*)(tsum + per_launch * per_field) : nullptr;
  for (int64_t r0 = 0; r0 < n_fields; r0 += per_launch) {
    const int n = (int)std::min<int64_t>(per_launch, n_fields - r0);
    hipError_t e = launch_variogram_local(fields + r0 * H * W, n, mask, H, W, mi, mj, T, k, tsum, tcount, sum + r0 * per_field,
                                          count + r0 * per_field, st);
    if (e != hipSuccess) { (void)hipStreamSynchronize(st); return fail(h, GSM_E_HIP, std::string("gsm_variogram_local: ") + hipGetErrorString(e)); }
  }
  if (k > 0) HIPCHK(h, hipStreamSynchronize(st));             // the scratch lives until the stream has drained
  return GSM_OK;
}
