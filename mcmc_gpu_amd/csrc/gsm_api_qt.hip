// C ABI of libgsm_hip.so, the fit of the normal-score transformers of a stack of fields (qt_fit_kernel.hip).
#include "gsm_context.h"

using namespace gsm;

extern "C" int gsm_qt_fit(gsm_handle h, const double* x, int32_t n, int64_t cells, const double* q, int32_t nq, double* quantiles,
                          int64_t* n_valid, int64_t* n_inf, double* sorted, void* stream) {
  if (!h) return GSM_E_ARG;                             // `cells` is the call's own: nothing here reads the handle's grid
  if (!x || !q || !quantiles || !n_valid || !n_inf) return fail(h, GSM_E_ARG, "gsm_qt_fit: NULL pointer (x, q, quantiles, n_valid, n_inf)");
  if ((const void*)quantiles == (const void*)x || (const void*)sorted == (const void*)x)
    return fail(h, GSM_E_ARG, "gsm_qt_fit: quantiles and sorted must not alias x");
  if (n < 1) return fail(h, GSM_E_ARG, "gsm_qt_fit: n must be >= 1");
  if (cells < 1 || cells > kQtFitMaxCells) return fail(h, GSM_E_ARG, "gsm_qt_fit: cells must be in [1, 2^24]");
  if (nq < 2 || nq > kQtFitMaxQuantiles) return fail(h, GSM_E_ARG, "gsm_qt_fit: nq must be in [2, 2^20]");
  for (int k = 0; k < nq; ++k)
    if (!(q[k] >= 0.0 && q[k] <= 1.0) || (k && q[k] < q[k - 1]))
      return fail(h, GSM_E_ARG, "gsm_qt_fit: q must ascend within [0, 1] (entry " + std::to_string(k) + ")");
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  const size_t total = (size_t)n * (size_t)cells;
  HIPCHK(h, h->d_sort_keys[0].ensure(total));
  if (cells > 4096) HIPCHK(h, h->d_sort_keys[1].ensure(total));       // one tile per field: no merge pass, no second buffer
  HIPCHK(h, h->d_qt_fit_q.ensure((size_t)nq));
  HIPCHK(h, hipMemcpyAsync(h->d_qt_fit_q.get(), q, (size_t)nq * sizeof(double), hipMemcpyHostToDevice, st));
  const hipError_t e = launch_qt_fit(x, n, cells, h->d_qt_fit_q.get(), nq, h->d_sort_keys[0].get(), h->d_sort_keys[1].get(), quantiles,
                                     n_valid, n_inf, sorted, st);
  if (e == hipErrorInvalidValue) return fail(h, GSM_E_ARG, "gsm_qt_fit: n * cells is more than one launch takes (2^31 workgroups of 4096 keys)");
  HIPCHK(h, e);
  return GSM_OK;
}
