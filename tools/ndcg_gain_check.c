/* The device's NDCG gain and discount (csrc/re_evaluate_ndcg.hip, ndcg_gain and ndcg_disc: exp_any and log_1_2 of csrc/re_device.hpp) restated
 * in C and checked against long double. Gain: fp32 labels over the whole domain (0, 64] — 2^25 labels spread evenly over the positive bit
 * patterns up to 64, so every exponent from the subnormals up, and every multiple of 1/16 — with the figure
 *   eps_g = max |g - exact| / exact,   exact = 2^i expm1l(f ln 2) + (2^i - 1) for y = i + f.
 * Discount: every rank below 2^22 and 2^22 ranks spread evenly up to 2^31 - 1, eps_d = max |d - exact| / exact, exact = 1 / log2l(r + 2).
 * include/gdmix_re.h, GDMIX_RE_EVAL_NDCG_GAIN_EPS and GDMIX_RE_EVAL_NDCG_DISC_EPS, are these figures rounded up; exit status 1 above them.
 *     cc -O2 -ffp-contract=off -o ndcg_gain_check tools/ndcg_gain_check.c -lm && ./ndcg_gain_check */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#define GAIN_EPS 1.0e-15
#define DISC_EPS 5.0e-16
static const double LN2 = 6.93147180559945309417e-01, LN2_HI = 6.93147180369123816490e-01, LN2_LO = 1.90821492927058770002e-10;
static double rcp_approx(double u) { float f = 1.0f / (float)u; return (double)f; } /* a 24-bit seed, as the hardware reciprocal gives */
static double rcp_nr(double u) { double y = rcp_approx(u); double e = fma(-u, y, 1.0); y = fma(y, e, y); e = fma(-u, y, 1.0); y = fma(y, e, y); e = fma(-u, y, 1.0); y = fma(y, e, y); return y; }
static double exp_any(double z) {
  const double a = fmin(fmax(z, -1100.0), 1100.0);
  const double kf = rint(a * 1.4426950408889634074);
  const double r0 = fma(-kf, LN2_HI, a);
  const double r = fma(-kf, LN2_LO, r0);
  const double rl = fma(-kf, LN2_LO, r0 - r);
  static const double c[] = {1.0 / 6227020800.0, 1.0 / 479001600.0, 1.0 / 39916800.0, 1.0 / 3628800.0, 1.0 / 362880.0, 1.0 / 40320.0,
                             1.0 / 5040.0,       1.0 / 720.0,       1.0 / 120.0,      1.0 / 24.0,      1.0 / 6.0,      0.5};
  double p = c[0];
  for (int i = 1; i < 12; i++) p = fma(p, r, c[i]);
  p = (fma(p, r * r, rl) + r) + 1.0;
  return ldexp(p, (int)kf);
}
static double log_1_2(double u) {
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
static double ndcg_gain(double y) {
  const double fl = floor(y), f = y - fl;
  const double p = ldexp(1.0, (int)fl), whole = p - 1.0;
  if (f == 0.0) return whole;
  const double x = f * LN2;
  const double u = exp_any(x);
  const double m = (u == 1.0) ? x : (u - 1.0) * x / log_1_2(u);
  return fma(p, m, whole);
}
static double ndcg_disc(int64_t r) {
  const uint64_t x = (uint64_t)r + 2u;
  const int e = 63 - __builtin_clzll(x);
  const double m = ldexp((double)x, -e);
  const double L = (double)e * LN2_HI + fma((double)e, LN2_LO, log_1_2(m));
  return LN2 / L;
}
static double g_worst = 0.0, d_worst = 0.0;
static float g_at = 0.0f;
static int64_t d_at = 0;
static void gain_one(float yf) {
  const double y = (double)yf;
  const long double fl = floorl((long double)y), f = (long double)y - fl;
  const long double p = ldexpl(1.0L, (int)fl);
  const long double want = p * expm1l(f * 0.693147180559945309417232121458176568L) + (p - 1.0L);
  if (want <= 0.0L) return;
  const double rel = (double)(fabsl((long double)ndcg_gain(y) - want) / want);
  if (rel > g_worst) { g_worst = rel; g_at = yf; }
}
static void disc_one(int64_t r) {
  const long double want = 1.0L / log2l((long double)r + 2.0L);
  const double rel = (double)(fabsl((long double)ndcg_disc(r) - want) / want);
  if (rel > d_worst) { d_worst = rel; d_at = r; }
}
int main(void) {
  long count = 0;
  for (uint32_t i = 1; i < (1u << 25); i++) {
    const uint32_t bits = (uint32_t)(((uint64_t)i * 0x42800000ull) >> 25);   /* just above +0 .. just below 64, every exponent */
    float y;
    memcpy(&y, &bits, 4);
    gain_one(y);
    count++;
  }
  for (int i = 1; i <= 64 * 16; i++) { gain_one((float)i / 16.0f); count++; }
  int exact_ok = 1;
  for (int i = 0; i <= 53; i++) exact_ok = exact_ok && ndcg_gain((double)i) == ldexp(1.0, i) - 1.0 && (long double)ndcg_gain((double)i) == ldexpl(1.0L, i) - 1.0L;
  for (int64_t r = 0; r < (1 << 22); r++) disc_one(r);
  for (int64_t j = 0; j < (1 << 22); j++) disc_one((j * 0x7FFFFFFFll) >> 22);
  disc_one(0x7FFFFFFEll);
  printf("long double carries %d bits. ndcg_gain over %ld fp32 labels in (0, 64]: max |g - exact| / exact = %.3e (at y = %.9g); integral labels 0 .. 53 exact: %s\n",
         LDBL_MANT_DIG, count, g_worst, (double)g_at, exact_ok ? "yes" : "NO");
  printf("ndcg_disc over ranks 0 .. 2^22 - 1 and 2^22 ranks up to 2^31 - 2: max |d - exact| / exact = %.3e (at r = %lld); d(0) = %.17g\n", d_worst, (long long)d_at,
         ndcg_disc(0));
  return (g_worst <= GAIN_EPS && d_worst <= DISC_EPS && exact_ok && ndcg_disc(0) == 1.0) ? 0 : 1;
}
