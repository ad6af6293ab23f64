// srt_fastmath.hpp -- device-only elementary functions shared by the kernels: the hot path's division and the
// range-specialised sqrt / sincos / log / exp / pow of the scattered model and the T04_s field.
#pragma once
#include <hip/hip_runtime.h>

namespace srt {

constexpr double FM_PI = 3.14159265358979323846;

// a/b for operands well inside the exponent range (every division of the hot path: frequencies, densities,
// field magnitudes, grid spacings).  This is the compiler's own fp64 division sequence -- v_rcp_f64, two Newton
// steps on the reciprocal, quotient, one residual correction -- without the v_div_scale / v_div_fmas /
// v_div_fixup wrapper that only matters for operands or quotients near the ends of the exponent range (8 instructions
// instead of 11).  Measured on the device (tests/test_gpu_fastmath.py): equal to the device's a / b and to IEEE a / b on
// every one of 1.2e6 points with the exponents of a and b in [-250, 250], edge mantissas and quotients next to rounding ties
// included (equal as numbers: the sign of a zero quotient can differ, -0 / 3 gives +0); the same test prints where it leaves IEEE
// outside that box.
// The sequence in two halves, so that divisions by the same b share the first: fdiv_recip(b) is the refined reciprocal (it
// depends on b alone), fdiv_r(a, b, r) the quotient and its correction.  fdiv(a, b) == fdiv_r(a, b, fdiv_recip(b)) bit for bit.
//
// OUTSIDE THE DOMAINS (pinned by tests/fastmath_cases.py::OUTSIDE on the device and in the host emulation; change both together):
//   fdiv      b = +-0, b = +-inf, b denormal, a = +-inf, an overflowing quotient (1e300 / 1e-300), NaN in a or b   -> NaN
//             (IEEE: +-inf, +-0, a finite or infinite quotient)
//   sqrt_pos  x < 0, x = +inf, NaN -> NaN;  x = -0 -> +0
//   log_pos   x < 0, x = +inf, NaN -> NaN;  x = +-0 -> -4.7507062... (a finite number, NOT -inf)
//   exp_any   NaN -> 0 (fmax drops the NaN);  -inf -> 0;  +inf -> NaN;  y <= -745.2 -> 0;  y >= 709.79 -> +inf
//   sincos_0pi  +-inf -> (-inf, NaN);  NaN -> (NaN, NaN)
//   sincos_mod  +-inf, NaN -> (NaN, NaN)
//   pow_pos   x <= 0, x >= 1e300, x NaN: the library's pow;  otherwise y NaN or +-inf -> NaN
__device__ __forceinline__ double fdiv_recip(double b) {
  double r = __builtin_amdgcn_rcp(b);
  r = fma(fma(-b, r, 1.0), r, r);
  r = fma(fma(-b, r, 1.0), r, r);
  return r;
}
__device__ __forceinline__ double fdiv_r(double a, double b, double r) {
  double q = a * r;
  return fma(fma(-b, q, a), r, q);
}
__device__ __forceinline__ double fdiv(double a, double b) { return fdiv_r(a, b, fdiv_recip(b)); }

// Elementary functions on the argument ranges of the scattered model's per-sample passes (srt_scattered.hpp) and of the
// T04_s field (srt_t04.hpp): each is the textbook (fdlibm) kernel without the library's range handling -- arguments there
// are never denormal, huge or NaN-by-construction -- at a third to a half of the library's instructions.  Largest errors
// measured on the device against long double, in ulp of the true value (tests/test_gpu_fastmath.py; the bar there is 2 ulp;
// tests/test_fastmath_host.py holds this header on the host, exact 1/b and 1/sqrt(x) for the hardware's seeds, to the same):
// sqrt_pos correctly rounded; sqrt_and_inv_pos 0.50 / 1.48; sincos_0pi 1.29 / 1.39; log_pos 0.72; exp_any 0.88 (0.87 of the
// denormal spacing below -708.4); sincos_mod 1.44 / 1.45; pow_pos 0.66.  Next to a zero of sin or cos the two-part pi/2 leaves
// an absolute error of (|k| + 1) 6.5e-27 (k the quadrant), not a relative one.
namespace fm {
// sqrt for 0 <= x, neither denormal nor near overflow: the compiler's own sequence (v_rsq_f64, one Goldschmidt step, two
// residual corrections) without its range scaling; equal to the device's sqrt and correctly rounded on exponents in
// [-500, 500] (measured; the residual goes denormal below about 2^-960)
__device__ __forceinline__ double sqrt_pos(double x) {
  const double y = __builtin_amdgcn_rsq(x);
  double g = x * y, h = 0.5 * y;
  const double r = fma(-h, g, 0.5);
  g = fma(g, r, g);
  h = fma(h, r, h);
  double d = fma(-g, g, x);
  g = fma(d, h, g);
  d = fma(-g, g, x);
  g = fma(d, h, g);
  return x == 0.0 ? 0.0 : g;
}
// g = sqrt(x) and inv = 1 / g for a positive normal x from ONE v_rsq_f64: the Goldschmidt pair (g, h = 1 / (2 g)) of sqrt_pos,
// then one Newton step on 2 h against the finished g (<= 1 ulp each; 13 operations against sqrt_pos + fdiv's 20)
// (no caller in the kernels -- chol_y measured no faster with it, HISTORY section 12.1; the host and GPU fastmath tests call it directly)
__device__ __forceinline__ void sqrt_and_inv_pos(double x, double &g_out, double &inv_out) {
  const double y = __builtin_amdgcn_rsq(x);
  double g = x * y, h = 0.5 * y;
  const double r = fma(-h, g, 0.5);
  g = fma(g, r, g);
  h = fma(h, r, h);
  double d = fma(-g, g, x);
  g = fma(d, h, g);
  d = fma(-g, g, x);
  g = fma(d, h, g);
  double inv = h + h;
  inv = fma(fma(-g, inv, 1.0), inv, inv);
  g_out = g;
  inv_out = inv;
}
// sin and cos of a in [0, pi (1 + 2e-3)]: quadrant k = 0, 1, 2, t = a - k pi/2 in about [-pi/4, pi/4]
__device__ __forceinline__ void sincos_0pi(double a, double &s, double &c) {
  const double PIO2_HI = 1.57079632673412561417e+00, PIO2_LO = 6.07710050650619224932e-11; // k * hi is exact (33 bits)
  const double kf = a > 0.75 * FM_PI ? 2.0 : (a > 0.25 * FM_PI ? 1.0 : 0.0);
  const double t = fma(-kf, PIO2_LO, fma(-kf, PIO2_HI, a));
  const double z = t * t;
  const double rs = 8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04 + z * (2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10)));
  const double st = t + (z * t) * (-1.66666666666666324348e-01 + z * rs);
  const double rc = z * (4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * (2.48015872894767294178e-05 + z * (-2.75573143513906633035e-07 + z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11)))));
  const double hz = 0.5 * z, w = 1.0 - hz;
  const double ct = w + (((1.0 - w) - hz) + z * rc);
  s = kf == 1.0 ? ct : (kf == 2.0 ? -st : st);
  c = kf == 1.0 ? -st : (kf == 2.0 ? -ct : ct);
}
// ln x for a positive normal x
__device__ __forceinline__ double log_pos(double x) {
  double m = __builtin_amdgcn_frexp_mant(x); // [0.5, 1)
  int e = __builtin_amdgcn_frexp_exp(x);
  const bool low = m < 0.70710678118654752440;
  m = low ? m + m : m; // [sqrt(1/2), sqrt 2)
  e = low ? e - 1 : e;
  const double f = m - 1.0, k = (double)e;
  const double sq = fdiv(f, 2.0 + f), z = sq * sq, w = z * z;
  const double t1 = w * (3.999999999940941908e-01 + w * (2.222219843214978396e-01 + w * 1.531383769920937332e-01));
  const double t2 = z * (6.666666666666735130e-01 + w * (2.857142874366239149e-01 + w * (1.818357216161805012e-01 + w * 1.479819860511658591e-01)));
  const double R = t2 + t1, hfsq = 0.5 * f * f;
  return k * 6.93147180369123816490e-01 - ((hfsq - (sq * (hfsq + R) + k * 1.90821492927058770002e-10)) - f);
}
// e^y for y <= ~700 (underflows to 0 below -745)
__device__ __forceinline__ double exp_any(double y) {
  y = fmax(y, -800.0);
  const double k = rint(y * 1.44269504088896338700e+00);
  const double r = fma(-k, 1.90821492927058770002e-10, fma(-k, 6.93147180369123816490e-01, y)); // |r| <= 0.3466
  double p = 1.0 / 6227020800.0;
  p = fma(p, r, 1.0 / 479001600.0);
  p = fma(p, r, 1.0 / 39916800.0);
  p = fma(p, r, 1.0 / 3628800.0);
  p = fma(p, r, 1.0 / 362880.0);
  p = fma(p, r, 1.0 / 40320.0);
  p = fma(p, r, 1.0 / 5040.0);
  p = fma(p, r, 1.0 / 720.0);
  p = fma(p, r, 1.0 / 120.0);
  p = fma(p, r, 1.0 / 24.0);
  p = fma(p, r, 1.0 / 6.0);
  p = fma(p, r, 0.5);
  p = fma(p, r, 1.0);
  p = fma(p, r, 1.0);
  return ldexp(p, (int)k);
}
// sin and cos of |x| up to ~1e5 (T04_s: positions in Earth radii over scale lengths, tilt angles): quadrant k = rint(x 2/pi),
// t = x - k pi/2 by a two-part pi/2 (k * hi exact, error ~k * 1e-21)
__device__ __forceinline__ void sincos_mod(double x, double &s, double &c) {
  const double k = rint(x * 0.63661977236758134308);
  double t = fma(-k, 1.57079632673412561417e+00, x);
  t = fma(-k, 6.07710050650619224932e-11, t);
  const double z = t * t;
  const double rs = 8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04 + z * (2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10)));
  const double st = t + (z * t) * (-1.66666666666666324348e-01 + z * rs);
  const double rc = z * (4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * (2.48015872894767294178e-05 + z * (-2.75573143513906633035e-07 + z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11)))));
  const double hz = 0.5 * z, w = 1.0 - hz;
  const double ct = w + (((1.0 - w) - hz) + z * rc);
  const int q = (int)k;
  const double s1 = (q & 1) ? ct : st, c1 = (q & 1) ? -st : ct;
  s = (q & 2) ? -s1 : s1;
  c = (q & 2) ? -c1 : c1;
}
__device__ __forceinline__ double sin_mod(double x) {
  double s, c;
  sincos_mod(x, s, c);
  return s;
}
__device__ __forceinline__ double cos_mod(double x) {
  double s, c;
  sincos_mod(x, s, c);
  return c;
}
// ln x = hi + lo for a positive normal x, to an absolute error of about 2^-60 (log_pos: half an ulp of the result, up to 2^-44).
// The reduction and the polynomial of log_pos, written as k ln2 + 2 s + s R(s^2) with s = f / (2 + f): k ln2_hi and 2 s_hi are
// summed exactly (Fast2Sum, |k ln2_hi| >= |2 s_hi| or k == 0), everything small -- the division's remainder, the rounding of
// 2 + f, s R and k ln2_lo -- goes into lo; |lo| <= ulp(hi) / 2 after the final renormalisation.
__device__ __forceinline__ void log_pos_hilo(double x, double &hi, double &lo) {
  double m = __builtin_amdgcn_frexp_mant(x); // [0.5, 1)
  int e = __builtin_amdgcn_frexp_exp(x);
  const bool low = m < 0.70710678118654752440;
  m = low ? m + m : m; // [sqrt(1/2), sqrt 2)
  e = low ? e - 1 : e;
  const double f = m - 1.0, k = (double)e;
  const double t = 2.0 + f, tl = (2.0 - t) + f; // 2 + f = t + tl exactly
  const double rc = fdiv_recip(t);
  const double sh = fdiv_r(f, t, rc);
  const double sl = fma(-sh, tl, fma(-sh, t, f)) * rc; // f / (t + tl) = sh + sl
  const double z = sh * sh, w = z * z;
  const double t1 = w * (3.999999999940941908e-01 + w * (2.222219843214978396e-01 + w * 1.531383769920937332e-01));
  const double t2 = z * (6.666666666666735130e-01 + w * (2.857142874366239149e-01 + w * (1.818357216161805012e-01 + w * 1.479819860511658591e-01)));
  const double A = k * 6.93147180369123816490e-01, B = sh + sh; // both exact
  const double small = fma(k, 1.90821492927058770002e-10, fma(sh, t2 + t1, sl + sl));
  const double h0 = A + B, l0 = ((A - h0) + B) + small;
  hi = h0 + l0;
  lo = (h0 - hi) + l0;
}
// e^(h + l) for |l| <= ~1e-10 |h|, h <= ~700, to 0.5 ulp + about 0.1 (exp_any: 1 ulp): the reduction of exp_any with the tail l
// and k ln2_lo folded into r = rh + e, then 1 + rh + rh^2 / 2 summed exactly (two Fast2Sums, the square's rounding error by an
// fma) and everything below -- e (1 + rh), rh^3 (1/6 + ...) -- added as one small term before the single final rounding
__device__ __forceinline__ double exp_hilo(double h, double l) {
  h = fmax(h, -800.0);
  const double k = rint(h * 1.44269504088896338700e+00);
  const double r0 = fma(-k, 6.93147180369123816490e-01, h); // exact
  const double rl = fma(-k, 1.90821492927058770002e-10, l);
  const double r = r0 + rl, e = (r0 - r) + rl; // |r| <= 0.3466
  const double zh = r * r, zl = fma(r, r, -zh);
  double p = 1.0 / 6227020800.0;
  p = fma(p, r, 1.0 / 479001600.0);
  p = fma(p, r, 1.0 / 39916800.0);
  p = fma(p, r, 1.0 / 3628800.0);
  p = fma(p, r, 1.0 / 362880.0);
  p = fma(p, r, 1.0 / 40320.0);
  p = fma(p, r, 1.0 / 5040.0);
  p = fma(p, r, 1.0 / 720.0);
  p = fma(p, r, 1.0 / 120.0);
  p = fma(p, r, 1.0 / 24.0);
  p = fma(p, r, 1.0 / 6.0);
  const double c = fma(0.5, zl, fma(zh * r, p, fma(e, r, e)));
  const double hz = 0.5 * zh;
  const double ah = 1.0 + r, al = (1.0 - ah) + r;
  const double bh = ah + hz, bl = (ah - bh) + hz;
  return ldexp(bh + ((bl + al) + c), (int)k);
}
// x**y for x > 0, to <= 1 ulp whatever |y ln x| is (within 0.6 ulp on T04's arguments): exp(y ln x) with ln x in two parts,
// the product y (hi + lo) = ph + pl with the multiplication's rounding error recovered by one fma, and the exponential of the
// pair.  x <= 0 or not finite: the library's.
// Tested for |y ln x| up to about 250 (x in [1e-12, 1e5], y in [-1, 9]); a result that overflows or underflows double is
// outside the domain (exp_hilo clamps its argument from below only, and (int)k leaves int for a huge one), as is y = +-inf.
__device__ __forceinline__ double pow_pos(double x, double y) {
  if (!(x > 0.0) || !(x < 1.0e300)) return pow(x, y);
  double hi, lo;
  log_pos_hilo(x, hi, lo);
  const double ph = y * hi;
  return exp_hilo(ph, fma(y, lo, fma(y, hi, -ph)));
}
} // namespace fm

} // namespace srt
