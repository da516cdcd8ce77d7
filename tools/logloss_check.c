/* The device's logistic-loss term (csrc/re_evaluate_poisson.hip, ll_term: exp_neg and log_1_2 of csrc/re_device.hpp) restated in C and
 * checked against long double: fp32 scores over the whole range — every exponent, 2^25 scores spread evenly over the positive bit patterns,
 * both signs, the special values — and both labels. u = 1 + e is rounded before the logarithm, so the error of a term is absolute, not
 * relative: the figure printed is eps = max over the samples of (|ce - exact| - 2^-53 exact), the part of a term's error that is not the one
 * relative rounding of its last addition. include/gdmix_re.h, GDMIX_RE_EVAL_LL_TERM_EPS, is this figure rounded up; exit status 1 above it.
 *     cc -O2 -ffp-contract=off -o logloss_check tools/logloss_check.c -lm && ./logloss_check */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#define TERM_EPS 1.5e-16
static double rcp_approx(double u) { float f = 1.0f / (float)u; return (double)f; } /* a 24-bit seed, as the hardware reciprocal gives */
static double rcp_nr(double u) { double y = rcp_approx(u); double e = fma(-u, y, 1.0); y = fma(y, e, y); e = fma(-u, y, 1.0); y = fma(y, e, y); e = fma(-u, y, 1.0); y = fma(y, e, y); return y; }
static double exp_neg(double a) {
  const double L2E = 1.4426950408889634074, LN2_HI = 6.93147180369123816490e-01, LN2_LO = 1.90821492927058770002e-10;
  a = fmin(a, 800.0);
  const double kf = rint(a * L2E);
  double r = fma(kf, LN2_HI, -a);
  r = fma(kf, LN2_LO, r);
  static const double c[] = {1.0 / 6227020800.0, 1.0 / 479001600.0, 1.0 / 39916800.0, 1.0 / 3628800.0, 1.0 / 362880.0, 1.0 / 40320.0,
                             1.0 / 5040.0,       1.0 / 720.0,       1.0 / 120.0,      1.0 / 24.0,      1.0 / 6.0,      0.5};
  double p = c[0];
  for (int i = 1; i < 12; i++) p = fma(p, r, c[i]);
  p = fma(p, r * r, r) + 1.0;
  return ldexp(p, -(int)kf);
}
static double log_1_2(double u) {
  const double LN2_HI = 6.93147180369123816490e-01, LN2_LO = 1.90821492927058770002e-10;
  const int k = u > 1.4142135623730951;
  const double m = k ? 0.5 * u : u;
  const double num = m - 1.0, den = m + 1.0;
  const double y = rcp_nr(den);
  const double s = num * y;
  const double slo = fma(-s, den, num) * y;
  const double s2 = s * s;
  static const double q[] = {2.0 / 21.0, 2.0 / 19.0, 2.0 / 17.0, 2.0 / 15.0, 2.0 / 13.0, 2.0 / 11.0, 2.0 / 9.0, 2.0 / 7.0, 2.0 / 5.0, 2.0 / 3.0};
  double p = q[0];
  for (int i = 1; i < 10; i++) p = fma(p, s2, q[i]);
  const double lo = fma(s * s2, p, (k ? LN2_LO : 0.0) + 2.0 * slo);
  const double res = 2.0 * s + lo;
  return k ? res + LN2_HI : res;
}
static double ll_term(float s, float y) {
  const double z = (double)s;
  const double e = exp_neg(fabs(z));
  return fmax(y > 0.5f ? -z : z, 0.0) + log_1_2(1.0 + e);
}
static long double exact(float s, float y) {
  const long double z = (long double)s;
  return fmaxl(y > 0.5f ? -z : z, 0.0L) + log1pl(expl(-fabsl(z)));
}
static double eps_worst = 0.0, abs_worst = 0.0;
static float at_eps = 0.0f;
static void one(float s, float y) {
  const long double want = exact(s, y);
  const double err = (double)fabsl((long double)ll_term(s, y) - want);
  const double eps = err - 0x1p-53 * (double)want;
  if (eps > eps_worst) { eps_worst = eps; at_eps = s; }
  if ((double)want <= 1.0 && err > abs_worst) abs_worst = err;
}
int main(void) {
  long count = 0;
  for (uint32_t i = 0; i < (1u << 25); i++) {
    const uint32_t bits = (uint32_t)(((uint64_t)i * 0x7F800000ull) >> 25);   /* +0 .. just below +inf, every exponent */
    float s;
    memcpy(&s, &bits, 4);
    one(s, 0.0f); one(s, 1.0f); one(-s, 0.0f); one(-s, 1.0f);
    count += 4;
  }
  const float special[] = {0.0f, -0.0f, 1.0f, -1.0f, 3.4028234663852886e38f, -3.4028234663852886e38f, 1.401298464324817e-45f, 88.72284f, -88.72284f, 103.97f, 36.7368f, 745.2f};
  for (unsigned i = 0; i < sizeof special / sizeof *special; i++) { one(special[i], 0.0f); one(special[i], 1.0f); count += 2; }
  const int ends = ll_term(INFINITY, 1.0f) == 0.0 && ll_term(-INFINITY, 0.0f) == 0.0 && isinf(ll_term(INFINITY, 0.0f)) && isinf(ll_term(-INFINITY, 1.0f));
  printf("ll_term over %ld fp32 scores x labels: eps = max(|ce - exact| - 2^-53 exact) = %.3e (at s = %.9g); worst |ce - exact| of a term <= 1: %.3e; infinities %s\n",
         count, eps_worst, (double)at_eps, abs_worst, ends ? "ok" : "WRONG");
  return (eps_worst <= TERM_EPS && ends) ? 0 : 1;
}
