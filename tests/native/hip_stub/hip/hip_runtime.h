// Stand-in for <hip/hip_runtime.h> when tests/native/fastmath_host.cpp compiles the UNMODIFIED srt_fastmath.hpp with g++
// (tests/test_fastmath_host.py puts this directory first on the include path).  It supplies the two qualifiers and the four
// hardware builtins the header uses, with exact host values for the hardware's approximate seeds: what is held on the host
// is the polynomials, the reductions and the selects, everything but v_rcp_f64 / v_rsq_f64 themselves.
#pragma once
#include <math.h>

#define __device__
#define __forceinline__ inline

static inline double __builtin_amdgcn_rcp(double b) { return 1.0 / b; }
static inline double __builtin_amdgcn_rsq(double x) { return (double)(1.0L / sqrtl((long double)x)); }
// v_frexp_mant_f64 / v_frexp_exp_i32_f64: mantissa in [0.5, 1) with the argument's sign; +-0, +-inf and NaN are
// returned as they are, with exponent 0
static inline double __builtin_amdgcn_frexp_mant(double x) {
  int e;
  return (x == 0.0 || !(fabs(x) <= 1.7976931348623157e308)) ? x : frexp(x, &e);
}
static inline int __builtin_amdgcn_frexp_exp(double x) {
  int e = 0;
  if (x == 0.0 || !(fabs(x) <= 1.7976931348623157e308)) return 0;
  frexp(x, &e);
  return e;
}
