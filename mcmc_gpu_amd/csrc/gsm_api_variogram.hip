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
