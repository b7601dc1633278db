// Host build of mcmc_gpu_amd/csrc/truncnorm.h as a tiny shared library for tests/test_interp_sgs_host.py (ctypes).
#include "truncnorm.h"
extern "C" {
void tn_ppf(const double* q, const double* a, const double* b, double* out, int n) {
  for (int i = 0; i < n; ++i) out[i] = gsm::tn::ppf(q[i], a[i], b[i]);
}
void tn_log_ndtr(const double* x, double* out, int n) { for (int i = 0; i < n; ++i) out[i] = gsm::tn::log_ndtr(x[i]); }
void tn_ndtri_exp(const double* x, double* out, int n) { for (int i = 0; i < n; ++i) out[i] = gsm::tn::ndtri_exp(x[i]); }
void tn_erfcx_pos(const double* x, double* out, int n) { for (int i = 0; i < n; ++i) out[i] = gsm::tn::erfcx_pos(x[i]); }
void tn_log_gauss_mass(const double* a, const double* b, double* out, int n) {
  for (int i = 0; i < n; ++i) out[i] = gsm::tn::log_gauss_mass(a[i], b[i]);
}
}
