// srt_rows.hpp -- the packed-row layout (offsets[nrays + 1], rows[offsets[nrays]][SRT_ROW]; include/srt.h) and the curve through
// two consecutive kept rows, as every consumer of packed rows reads them (srt_crossings.hpp, srt_approaches.hpp,
// srt_binning.hpp): which pairs of rows are an interval of one ray, whether an interval can be used at all, the cubic Hermite
// curve with end slopes C * vgrel (the right-hand side of the position equation the rows already carry), and a point of it
// as a row of the kept-row layout.
//
// Everything here is __host__ __device__ and spells out every operation with contraction off (as srt_xform.hpp does), so that
// a host build (tests/native/*_host.cpp) and the device give the same bits.
//
// Compiles for the device (hipcc) and for the host.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/srt.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ROWS_HD __host__ __device__
#else
#define ROWS_HD
#endif
#if defined(__clang__)
#define ROWS_NOCONTRACT _Pragma("clang fp contract(off)")
#else
#define ROWS_NOCONTRACT // (g++: built with -ffp-contract=off)
#endif

namespace srt {
namespace rows {

constexpr int BISECTIONS = 52; // the bracket [0, 1] halves to 2^-52: sigma* is within 2^-50 of the sign change, with room
constexpr double EARTH_RADIUS = 6371.2e3; // constants.f95:8

// C, the speed of light as the library's models compute it
inline double light_speed() {
  ROWS_NOCONTRACT
  const double EPS0 = 8.854187817e-12, PI = 3.141592653589793238462643; // constants.f95:4-5
  const double MU0 = PI * 4e-7;                                        // constants.f95:6
  return sqrt(1.0 / EPS0 / MU0);                                       // constants.f95:7
}

// can the interval between two kept rows hold events at all: t, pos and vgrel finite at both ends, and t1 != t0
ROWS_HD inline bool interval_usable(const double *r0, const double *r1) {
  bool ok = __builtin_isfinite(r0[0]) && __builtin_isfinite(r1[0]) && r1[0] != r0[0];
  for (int c = 0; c < 3; ++c)
    ok = ok && __builtin_isfinite(r0[1 + c]) && __builtin_isfinite(r1[1 + c]) && __builtin_isfinite(r0[7 + c]) && __builtin_isfinite(r1[7 + c]);
  return ok;
}

// The cubic Hermite curve in its Delta form (the basis-function form cancels at 1e7 m):
//   p(sigma) = p0 + sigma m0 + sigma^2 (3 D - 2 m0 - m1) + sigma^3 (m0 + m1 - 2 D),  D = p1 - p0,  m = C vgrel h
struct Interval {
  double t0, h;
  double p0[3], m0[3], c2[3], c3[3];
};
ROWS_HD inline void interval_setup(const double *r0, const double *r1, double C, Interval &iv) {
  ROWS_NOCONTRACT
  iv.t0 = r0[0];
  iv.h = r1[0] - r0[0];
  for (int c = 0; c < 3; ++c) {
    const double d = r1[1 + c] - r0[1 + c];
    const double m0 = C * r0[7 + c] * iv.h, m1 = C * r1[7 + c] * iv.h;
    iv.p0[c] = r0[1 + c];
    iv.m0[c] = m0;
    iv.c2[c] = 3.0 * d - 2.0 * m0 - m1;
    iv.c3[c] = m0 + m1 - 2.0 * d;
  }
}
ROWS_HD inline void hermite(const Interval &iv, double sigma, double x[3]) {
  ROWS_NOCONTRACT
  for (int c = 0; c < 3; ++c) x[c] = iv.p0[c] + sigma * (iv.m0[c] + sigma * (iv.c2[c] + sigma * iv.c3[c]));
}

// a point of the curve as a row of the kept-row layout: t and pos on the curve, columns 4 .. 19 linear in sigma
ROWS_HD inline void event_row(const Interval &iv, const double *r0, const double *r1, double sigma, double *out) {
  ROWS_NOCONTRACT
  out[0] = iv.t0 + sigma * iv.h;
  hermite(iv, sigma, out + 1);
  for (int c = 4; c < SRT_ROW; ++c) out[c] = r0[c] + sigma * (r1[c] - r0[c]);
}

// the ray of packed row j: the last r in [0, nrays) with offsets[r] <= j (empty rays have offsets[r] == offsets[r + 1] and
// are never the answer for a row that exists); -1 if offsets[0] > j
ROWS_HD inline long long ray_of_row(const long long *offsets, long long nrays, long long j) {
  long long lo = 0, hi = nrays;
  while (lo < hi) {
    const long long mid = lo + (hi - lo) / 2;
    if (offsets[mid] <= j) lo = mid + 1;
    else hi = mid;
  }
  return lo - 1;
}

// is (j, j + 1) an interval of one ray?  -> its ray, or -1
ROWS_HD inline long long interval_ray(const long long *offsets, long long nrays, long long j) {
  const long long r = ray_of_row(offsets, nrays, j);
  return (r < 0 || j + 1 >= offsets[r + 1]) ? -1 : r;
}

} // namespace rows
} // namespace srt
