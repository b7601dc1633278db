// Truncated-normal quantile on the host and the device: scipy.stats.truncnorm.ppf(q, a, b) as scipy 1.15 computes it, for
// the bounded draws of interpolate.sgs (gstatsim_custom/interpolate.py:240-261, truncnorm.rvs = ppf(uniform) * scale + loc:
// truncnorm has no _rvs of its own).  Restated from the published algorithms:
//   * truncnorm._ppf (scipy/stats/_continuous_distns.py): ppf_left for a < 0, ppf_right otherwise, on _log_gauss_mass(a, b)
//     with its three cases (both bounds left of 0, both right of 0, central);
//   * _log_sum / _log_diff: scipy's logsumexp of two terms (log1p(exp(min - max)) + max), and log(exp(p) - exp(q)) written in
//     real arithmetic where scipy goes through a complex logsumexp;
//   * scipy.special.log_ndtr (Faddeeva package, S. G. Johnson): log(erfcx(-t) / 2) - t^2 for x < -1, log1p(-erfc(t) / 2)
//     otherwise, t = x / sqrt(2).  erfcx(y) for y >= 1 is Cephes erfc's rational function without its exp(-y^2) factor;
//   * scipy.special.ndtri_exp (scipy/special/_ndtri_exp.pxd): Cephes ndtri's asymptotic branch fed with log(y) directly for
//     y < -2, ndtri(exp(y)) / -ndtri(-expm1(y)) above.
// The file compiles for the host too: tests/test_interp_sgs_host.py checks it against scipy with g++.
#pragma once
#include "normal_score.h"
#include <cfloat>

namespace gsm {
namespace tn {

constexpr double kSqrt1_2 = 0.70710678118654752440;

// erfc(y) * exp(y^2) for y >= 0
GSM_NS_FN double erfcx_pos(double y) {
  const double P[] = {2.46196981473530512524E-10, 5.64189564831068821977E-1, 7.46321056442269912687E0, 4.86371970985681366614E1,
                      1.96520832956077098242E2, 5.26445194995477358631E2, 9.34528527171957607540E2, 1.02755188689515710272E3,
                      5.57535335369399327526E2};
  const double Q[] = {1.32281951154744992508E1, 8.67072140885989742329E1, 3.54937778887819891062E2, 9.75708501743205489753E2,
                      1.82390916687909736289E3, 2.24633760818710981792E3, 1.65666309194161350182E3, 5.57535340817727675546E2};
  const double R[] = {5.64189583547755073984E-1, 1.27536670759978104416E0, 5.01905042251180477414E0, 6.16021097993053585195E0,
                      7.40974269950448939160E0, 2.97886665372100240670E0};
  const double S[] = {2.26052863220117276590E0, 9.39603524938001434673E0, 1.20489539808096656605E1, 1.70814450747565897222E1,
                      9.60896809063285878198E0, 3.36907645100081516050E0};
  if (y < 1.0) return ns::erfc_c(y) * std::exp(y * y);
  if (y < 8.0) return ns::polevl(y, P, 8) / ns::p1evl(y, Q, 8);
  if (y > 1e50) return R[0] / y;          // the limit of the quotient below, before y^6 overflows there (y > 1.5e51: inf / inf)
  return ns::polevl(y, R, 5) / ns::p1evl(y, S, 6);
}

// scipy.special.log_ndtr = log(norm.cdf(x))
GSM_NS_FN double log_ndtr(double x) {
  if (std::isnan(x)) return x;
  if (x == -INFINITY) return -INFINITY;
  const double t = x * kSqrt1_2;
  if (x < -1.0) return std::log(erfcx_pos(-t) / 2.0) - t * t;
  return std::log1p(-ns::erfc_c(t) / 2.0);
}

// scipy.special.ndtri_exp: the x with log_ndtr(x) = y
GSM_NS_FN double ndtri_exp(double y) {
  const double P1[] = {4.05544892305962419923E0, 3.15251094599893866154E1, 5.71628192246421288162E1, 4.40805073893200834700E1,
                       1.46849561928858024014E1, 2.18663306850790267539E0, -1.40256079171354495875E-1, -3.50424626827848203418E-2,
                       -8.57456785154685413611E-4};
  const double Q1[] = {1.57799883256466749731E1, 4.53907635128879210584E1, 4.13172038254672030440E1, 1.50425385692907503408E1,
                       2.50464946208309415979E0, -1.42182922854787788574E-1, -3.80806407691578277194E-2, -9.33259480895457427372E-4};
  const double P2[] = {3.23774891776946035970E0, 6.91522889068984211695E0, 3.93881025292474443415E0, 1.33303460815807542389E0,
                       2.01485389549179081538E-1, 1.23716634817820021358E-2, 3.01581553508235416007E-4, 2.65806974686737550832E-6,
                       6.23974539184983293730E-9};
  const double Q2[] = {6.02427039364742014255E0, 3.67983563856160859403E0, 1.37702099489081330271E0, 2.16236993594496635890E-1,
                       1.34204006088543189037E-2, 3.28014464682127739104E-4, 2.89247864745380683936E-6, 6.79019408009981274425E-9};
  if (std::isnan(y)) return y;
  if (y < -DBL_MAX) return -INFINITY;
  if (y < -2.0) {
    const double x = (y >= -DBL_MAX * 0.5) ? std::sqrt(-2.0 * y) : 1.41421356237309504880 * std::sqrt(-y);
    const double x0 = x - std::log(x) / x;
    const double z = 1.0 / x;
    const double x1 = (x < 8.0) ? z * ns::polevl(z, P1, 8) / ns::p1evl(z, Q1, 8) : z * ns::polevl(z, P2, 8) / ns::p1evl(z, Q2, 8);
    return x1 - x0;
  }
  if (y > -0.14541345786885906) return -ns::ndtri(-std::expm1(y));     // log1p(-exp(-2))
  return ns::ndtri(std::exp(y));
}

// log(exp(p) + exp(q))
GSM_NS_FN double log_sum(double p, double q) {
  if (std::isnan(p) || std::isnan(q)) return p + q;                 // numpy.logaddexp gives NaN; fmax / fmin would drop it
  const double m = std::fmax(p, q), s = std::fmin(p, q);
  if (m == -INFINITY) return -INFINITY;
  return std::log1p(std::exp(s - m)) + m;
}
// log(exp(p) - exp(q)), p >= q, with scipy's rounding: logsumexp([p, q + pi i]) is log1p(exp(q - p + pi i)) + p, and numpy's
// complex log1p(z) is log(hypot(1 + Re z, Im z)) -- not the real log1p, so narrow intervals lose digits there as they do in
// scipy (Re, Im of exp(d + pi i) = -exp(d), exp(d) sin(pi))
GSM_NS_FN double log_diff(double p, double q) {
  if (q == -INFINITY) return p;
  const double e = std::exp(q - p);
  return std::log(std::hypot(1.0 + (-e), e * 1.2246467991473532e-16)) + p;
}

// log of the standard normal mass in [a, b]
GSM_NS_FN double log_gauss_mass(double a, double b) {
  if (b <= 0.0) return log_diff(log_ndtr(b), log_ndtr(a));          // left tail
  if (a > 0.0) return log_diff(log_ndtr(-a), log_ndtr(-b));         // right tail, by symmetry
  return std::log1p(-ns::ndtr(a) - ns::ndtr(-b));                    // central
}

// scipy.stats.truncnorm.ppf(q, a, b) for a < b, 0 <= q <= 1
GSM_NS_FN double ppf(double q, double a, double b) {
  if (a < b && (q == 0.0 || q == 1.0)) return (q == 0.0) ? a : b;    // rv_continuous.ppf returns the bounds there without calling _ppf
  const double m = log_gauss_mass(a, b);
  if (a < 0.0) return ndtri_exp(log_sum(log_ndtr(a), std::log(q) + m));
  return -ndtri_exp(log_sum(log_ndtr(-b), std::log1p(-q) + m));
}

}  // namespace tn
}  // namespace gsm
