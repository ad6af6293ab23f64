// One switch over the functions of srt_fastmath.hpp, (a, b) -> (o0, o1), shared by the device probe
// (fastmath_probe.hip) and the host emulation (fastmath_host.cpp) so that both answer the same op codes
// (tests/fastmath_cases.py::OPS mirrors them).  Include srt_fastmath.hpp first.
#pragma once

#ifndef FMO_HD
#define FMO_HD
#endif

enum {
  FMO_FDIV = 0,          // o0 = fdiv(a, b)                      o1 = the compiler's a / b
  FMO_FDIV_R = 1,        // o0 = fdiv_r(a, b, fdiv_recip(b))     o1 = fdiv_recip(b)
  FMO_SQRT_POS = 2,      // o0 = sqrt_pos(a)                     o1 = the compiler's sqrt(a)
  FMO_SQRT_AND_INV = 3,  // o0, o1 = sqrt_and_inv_pos(a)
  FMO_SINCOS_0PI = 4,    // o0, o1 = sincos_0pi(a)
  FMO_LOG_POS = 5,       // o0 = log_pos(a)
  FMO_EXP_ANY = 6,       // o0 = exp_any(a)
  FMO_SINCOS_MOD = 7,    // o0, o1 = sincos_mod(a)
  FMO_SIN_COS_MOD = 8,   // o0 = sin_mod(a)                      o1 = cos_mod(a)
  FMO_POW_POS = 9,       // o0 = pow_pos(a, b)
  FMO_COUNT = 10
};

FMO_HD static inline void fm_op(int op, double a, double b, double &o0, double &o1) {
  o0 = 0.0;
  o1 = 0.0;
  switch (op) {
  case FMO_FDIV:
    o0 = ::srt::fdiv(a, b);
    o1 = a / b;
    break;
  case FMO_FDIV_R:
    o1 = ::srt::fdiv_recip(b);
    o0 = ::srt::fdiv_r(a, b, o1);
    break;
  case FMO_SQRT_POS:
    o0 = ::srt::fm::sqrt_pos(a);
    o1 = sqrt(a);
    break;
  case FMO_SQRT_AND_INV:
    ::srt::fm::sqrt_and_inv_pos(a, o0, o1);
    break;
  case FMO_SINCOS_0PI:
    ::srt::fm::sincos_0pi(a, o0, o1);
    break;
  case FMO_LOG_POS:
    o0 = ::srt::fm::log_pos(a);
    break;
  case FMO_EXP_ANY:
    o0 = ::srt::fm::exp_any(a);
    break;
  case FMO_SINCOS_MOD:
    ::srt::fm::sincos_mod(a, o0, o1);
    break;
  case FMO_SIN_COS_MOD:
    o0 = ::srt::fm::sin_mod(a);
    o1 = ::srt::fm::cos_mod(a);
    break;
  case FMO_POW_POS:
    o0 = ::srt::fm::pow_pos(a, b);
    break;
  default:
    break;
  }
}
