// Host restatement of the scalar arithmetic of the Philox proposal path, built with g++ -ffp-contract=off and run by
// tests/test_proposal_math_host.py: log_tab / sincos_tab / build_math_tables are mcmc_gpu_amd/csrc/math_tables.h itself (it compiles
// for the host); exp_lean, sqrt_lean, the two Box-Muller bodies and spectral_amp of csrc/proposal_device.h are restated with the same
// operations and the same fmas (sqrt_lean: the true 1 / sqrt in place of the hardware's estimate), the uniforms are csrc/philox.h's.
//   usage: proposal_math_host SELECTOR MODEL SMOOTHNESS N  < input arrays (raw, one after the other)  > N x values-per-element doubles (raw)
// SELECTOR as GSM_PMATH_* of include/gsm.h (1 .. 7; Philox itself has gsm_philox_selftest).
#include "math_tables.h"
#include "philox.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

static double exp_lean(double x) {
  x = fmax(x, -1100.0);
  const double kf = __builtin_rint(x * 1.44269504088896338700e+00);
  const double r = __builtin_fma(kf, -1.90821492927058770002e-10, __builtin_fma(kf, -6.93147180369123816490e-01, x));
  double p = __builtin_fma(r, 2.08767569878680989792e-09, 2.50521083854417187751e-08);
  const double c[] = {2.75573192239858906526e-07, 2.75573192239858906526e-06, 2.48015873015873015873e-05, 1.98412698412698412698e-04,
                      1.38888888888888888889e-03, 8.33333333333333333333e-03, 4.16666666666666666667e-02, 1.66666666666666666667e-01,
                      0.5, 1.0, 1.0};
  for (double cc : c) p = __builtin_fma(r, p, cc);
  return ldexp(p, (int)kf);
}

static double sqrt_lean(double t) {
  t = fmax(t, 1e-300);
  const double y = 1.0 / sqrt(t);
  double g = t * y, h = 0.5 * y;
  const double r = __builtin_fma(-h, g, 0.5);
  g = __builtin_fma(g, r, g);
  h = __builtin_fma(h, r, h);
  return __builtin_fma(__builtin_fma(-g, g, t), h, g);
}

static void normals2_words(const uint32_t* w, double* g, const double* mt) {
  const double u1 = gsm::u01_open0_from(w[0], w[1]);
  const double u2 = gsm::u01_from(w[2], w[3]);
  const double rad = sqrt_lean(-2.0 * gsm::log_tab(u1, mt));
  double s, c;
  gsm::sincos_tab(u2, mt, s, c);
  g[0] = rad * c; g[1] = rad * s;
}

static void normals4_words(const uint32_t* w, double* g, const double* mt) {
  const double ra = sqrt_lean(-2.0 * gsm::log_tab(gsm::u01_open0_from32(w[0]), mt));
  const double rb = sqrt_lean(-2.0 * gsm::log_tab(gsm::u01_open0_from32(w[2]), mt));
  double s, c;
  gsm::sincos_tab(gsm::u01_from32(w[1]), mt, s, c);
  g[0] = ra * c; g[1] = ra * s;
  gsm::sincos_tab(gsm::u01_from32(w[3]), mt, s, c);
  g[2] = rb * c; g[3] = rb * s;
}

static double spectral_amp(int model, double smoothness, double aa, double m_kappa, double m_const, double k2, const double* mt) {
  if (model == 0) return exp_lean(-0.25 * ((aa * aa) * k2));
  if (model == 1) return exp_lean(-0.75 * gsm::log_tab(1.0 + (aa * aa) * k2, mt));
  const double nu = (smoothness != 0.0) ? smoothness : 1.0;
  return exp_lean(__builtin_fma(-0.5 * (nu + 1.0), gsm::log_tab(m_kappa + 4.0 * M_PI * k2, mt), m_const));
}

template <class T> static std::vector<T> read_n(size_t n) {
  std::vector<T> v(n);
  if (fread(v.data(), sizeof(T), n, stdin) != n) { fprintf(stderr, "short input\n"); exit(2); }
  return v;
}

int main(int argc, char** argv) {
  if (argc != 5) return 2;
  const int which = atoi(argv[1]), model = atoi(argv[2]);
  const double smoothness = atof(argv[3]);
  const size_t n = (size_t)atoll(argv[4]);
  double mt[gsm::kMathTabDoubles];
  gsm::build_math_tables(mt);
  std::vector<double> out;
  if (which == 5 || which == 6) {
    const std::vector<uint32_t> w = read_n<uint32_t>(4 * n);
    const int per = (which == 5) ? 4 : 2;
    out.resize(per * n);
    for (size_t i = 0; i < n; ++i) {
      if (which == 5) normals4_words(&w[4 * i], &out[4 * i], mt);
      else normals2_words(&w[4 * i], &out[2 * i], mt);
    }
  } else if (which == 7) {
    const std::vector<double> aa = read_n<double>(n), ka = read_n<double>(n), co = read_n<double>(n), k2 = read_n<double>(n);
    out.resize(n);
    for (size_t i = 0; i < n; ++i) out[i] = spectral_amp(model, smoothness, aa[i], ka[i], co[i], k2[i], mt);
  } else if (which >= 1 && which <= 4) {
    const std::vector<double> x = read_n<double>(n);
    out.resize((which == 2) ? 2 * n : n);
    for (size_t i = 0; i < n; ++i) {
      if (which == 1) out[i] = gsm::log_tab(x[i], mt);
      else if (which == 2) gsm::sincos_tab(x[i], mt, out[2 * i], out[2 * i + 1]);
      else if (which == 3) out[i] = sqrt_lean(x[i]);
      else out[i] = exp_lean(x[i]);
    }
  } else {
    return 2;
  }
  return fwrite(out.data(), sizeof(double), out.size(), stdout) == out.size() ? 0 : 1;
}
