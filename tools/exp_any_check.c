/* The device's exp for arguments of either sign (csrc/re_device.hpp, exp_any) restated in C and checked against long double: a grid of
 * 4e6 points over [-745, 709.78], the ends, NaN. The bar is exp_neg's own (tools/softplus_check.c): <= 0.98 ulp on normal results; a
 * subnormal result is off by at most one of its (fixed) spacings more, from ldexp's one rounding. Prints the figures; exit status 1 above the bar.
 *     cc -O2 -ffp-contract=off -o exp_any_check tools/exp_any_check.c -lm && ./exp_any_check */
#include <float.h>
#include <math.h>
#include <stdio.h>
static double exp_any(double z) {
  const double L2E = 1.4426950408889634074, LN2_HI = 6.93147180369123816490e-01, LN2_LO = 1.90821492927058770002e-10;
  const double a = fmin(fmax(z, -1100.0), 1100.0);
  const double kf = rint(a * L2E);
  const double r0 = fma(-kf, LN2_HI, a);
  const double r = fma(-kf, LN2_LO, r0);       /* r = z - k ln2, |r| <= ln2/2 */
  const double rl = fma(-kf, LN2_LO, r0 - r);  /* what the rounding of r dropped */
  static const double c[] = {1.0 / 6227020800.0, 1.0 / 479001600.0, 1.0 / 39916800.0, 1.0 / 3628800.0, 1.0 / 362880.0, 1.0 / 40320.0,
                             1.0 / 5040.0,       1.0 / 720.0,       1.0 / 120.0,      1.0 / 24.0,      1.0 / 6.0,      0.5};
  double p = c[0];
  for (int i = 1; i < 12; i++) p = fma(p, r, c[i]);
  p = (fma(p, r * r, rl) + r) + 1.0;
  const double e = ldexp(p, (int)kf);
  return (z != z) ? z : e;
}
int main(void) {
  const long N = 4000000;
  const double lo = -745.0, hi = 709.78;
  double worst_normal = 0.0, worst_sub = 0.0, at_normal = 0.0;
  for (long i = 0; i <= N; i++) {
    const double z = lo + (hi - lo) * ((double)i / (double)N);
    const double got = exp_any(z);
    const long double want = expl((long double)z);
    if ((double)want >= DBL_MIN) {
      const double u = nextafter((double)want, INFINITY) - (double)want;
      const double e = (double)fabsl(((long double)got - want) / u);
      if (e > worst_normal) { worst_normal = e; at_normal = z; }
    } else {
      const double e = (double)fabsl(((long double)got - want) / 4.9406564584124654e-324L);
      if (e > worst_sub) worst_sub = e;
    }
  }
  const int ends = isinf(exp_any(709.79)) && exp_any(709.79) > 0 && isinf(exp_any(1e300)) && exp_any(-746.0) == 0.0 && exp_any(-1e300) == 0.0 &&
                   isnan(exp_any(NAN)) && exp_any(0.0) == 1.0 && isinf(exp_any(INFINITY)) && exp_any(-INFINITY) == 0.0;
  printf("exp_any over [%g, %g], %ld points: max %.3f ulp on normal results (at z = %.17g), max %.3f spacings on subnormal results, ends %s\n", lo, hi, N + 1,
         worst_normal, at_normal, worst_sub, ends ? "ok" : "WRONG");
  return (worst_normal <= 0.98 && worst_sub <= 1.5 && ends) ? 0 : 1;
}
