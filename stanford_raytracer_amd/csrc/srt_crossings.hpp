// srt_crossings.hpp -- where and when a traced ray crosses a surface (include/srt.h, "surface crossings"): the surfaces' g(x),
// the bisection that locates a sign change of g on the cubic Hermite curve through two consecutive kept rows (srt_rows.hpp),
// and the two passes over packed rows.
//
// Two halves.  The POINT FUNCTIONS are __host__ __device__ and spell out every operation with contraction off (as
// srt_xform.hpp does), so that a host build (tests/native/crossings_host.cpp) and the device give the same bits wherever sqrt
// does.  The KERNELS are a count pass (one 16-bit surface mask per packed row: bit s = the interval that STARTS at this row holds
// an event of surface s) and a fill pass that reads only rows whose mask is not zero; a prefix sum of the masks' bit counts
// lies between them (srt_api_rows.hpp), which is what puts the events in (ray, interval, surface) order.
//
// Compiles for the device (hipcc) and for the host.
#pragma once
#include "srt_rows.hpp"

namespace srt {
namespace crossings {

// C as prepare() puts it into Surfaces::C, under the name callers of this header have always had for it
using rows::light_speed;

// the surfaces as the passes read them: a kind-1 p[0] is L * R_E, a kind-2 p[0] the sine of the latitude (both taken once, on
// the host), C the speed of light as the library's models compute it
struct Surfaces {
  int32_t n, reserved;
  double C;
  srt_surface s[SRT_MAXSURF];
};

// Host: the refusals of include/srt.h, by name.  0 = fine and *out is ready; otherwise `why` says what is wrong.
inline int prepare(int nsurf, const srt_surface *in, Surfaces *out, char *why, size_t whylen) {
  if (nsurf < 1 || nsurf > SRT_MAXSURF) {
    snprintf(why, whylen, "nsurf = %d is outside 1 .. %d (SRT_MAXSURF)", nsurf, SRT_MAXSURF);
    return -1;
  }
  if (!in) {
    snprintf(why, whylen, "null surfaces");
    return -1;
  }
  out->n = nsurf;
  out->reserved = 0;
  out->C = light_speed();
  for (int i = 0; i < SRT_MAXSURF; ++i) out->s[i] = srt_surface{0, 0, {1.0, 0.0, 0.0, 0.0}};
  for (int i = 0; i < nsurf; ++i) {
    const srt_surface &s = in[i];
    if (s.kind < 0 || s.kind > 3) {
      snprintf(why, whylen, "surface %d: unknown kind %d (0 sphere, 1 L-shell, 2 magnetic latitude, 3 plane)", i, (int)s.kind);
      return -1;
    }
    const int np = s.kind == 3 ? 4 : 1;
    for (int k = 0; k < np; ++k)
      if (!__builtin_isfinite(s.p[k])) {
        snprintf(why, whylen, "surface %d: parameter p[%d] is not finite", i, k);
        return -1;
      }
    srt_surface o = s;
    o.reserved = 0;
    if (s.kind == 0) {
      if (!(s.p[0] > 0.0)) {
        snprintf(why, whylen, "surface %d: sphere radius %g is not > 0", i, s.p[0]);
        return -1;
      }
    } else if (s.kind == 1) {
      if (!(s.p[0] > 0.0)) {
        snprintf(why, whylen, "surface %d: L = %g is not > 0", i, s.p[0]);
        return -1;
      }
      o.p[0] = s.p[0] * rows::EARTH_RADIUS;
    } else if (s.kind == 2) {
      if (!(fabs(s.p[0]) < 1.5707963267948966)) {
        snprintf(why, whylen, "surface %d: |latitude| = %g rad is not below pi/2", i, fabs(s.p[0]));
        return -1;
      }
      o.p[0] = sin(s.p[0]);
    } else {
      if (s.p[0] == 0.0 && s.p[1] == 0.0 && s.p[2] == 0.0) {
        snprintf(why, whylen, "surface %d: the plane's normal is zero", i);
        return -1;
      }
    }
    if (s.kind != 3) o.p[1] = o.p[2] = o.p[3] = 0.0;
    out->s[i] = o;
  }
  return 0;
}

// g(x) of a prepared surface, x in SM metres
ROWS_HD inline double surface_g(const srt_surface &s, const double x[3]) {
  ROWS_NOCONTRACT
  if (s.kind == 3) return s.p[0] * x[0] + s.p[1] * x[1] + s.p[2] * x[2] - s.p[3];
  const double rho2 = x[0] * x[0] + x[1] * x[1];
  const double r2 = rho2 + x[2] * x[2];
  const double r = sqrt(r2);
  if (s.kind == 0) return r - s.p[0];
  if (s.kind == 1) return r2 * r - s.p[0] * rho2; // |x|^3 - L R_E (x^2 + y^2): no division on the axis
  return x[2] - r * s.p[0];
}

// bit s: (g_i < 0) != (g_{i+1} < 0) for surface s -- a row exactly on the surface gives one event per pass, not two
ROWS_HD inline uint32_t interval_mask(const Surfaces &S, const double *r0, const double *r1) {
  if (!rows::interval_usable(r0, r1)) return 0u;
  uint32_t m = 0u;
  for (int s = 0; s < S.n; ++s) {
    const bool n0 = surface_g(S.s[s], r0 + 1) < 0.0, n1 = surface_g(S.s[s], r1 + 1) < 0.0;
    if (n0 != n1) m |= 1u << s;
  }
  return m;
}

// sigma*: BISECTIONS halvings of [0, 1], keeping the rows' end signs either side (neg0 = g_i < 0).  Returned is the end of the
// last bracket on which g >= 0, so that a row exactly on the surface is found at sigma = 1 or 0 exactly.
ROWS_HD inline double locate(const srt_surface &s, const rows::Interval &iv, bool neg0) {
  ROWS_NOCONTRACT
  double lo = 0.0, hi = 1.0;
  for (int it = 0; it < rows::BISECTIONS; ++it) {
    const double mid = 0.5 * (lo + hi);
    double x[3];
    rows::hermite(iv, mid, x);
    if ((surface_g(s, x) < 0.0) == neg0) lo = mid;
    else hi = mid;
  }
  return neg0 ? hi : lo;
}

// the mask of packed row j: of the interval (j, j + 1) when both rows belong to one ray.  The geometry is looked at first: most
// rows have no sign change, and only those that have one pay for the search in offsets.
ROWS_HD inline uint32_t row_mask(const Surfaces &S, long long nrays, const long long *offsets, long long total, const double *rows,
                                 long long j) {
  if (j + 1 >= total) return 0u;
  const uint32_t m = interval_mask(S, rows + j * SRT_ROW, rows + (j + 1) * SRT_ROW);
  if (!m) return 0u;
  if (rows::interval_ray(offsets, nrays, j) < 0) return 0u;
  return m;
}

// the events of packed row j, event number e0 onwards; events numbered >= capacity are left out
ROWS_HD inline void row_events(const Surfaces &S, long long nrays, const long long *offsets, const double *rows, long long j, uint32_t m,
                               long long e0, long long capacity, double *ev_rows, int32_t *ev_meta) {
  const long long r = rows::ray_of_row(offsets, nrays, j);
  if (r < 0) return;
  const double *r0 = rows + j * SRT_ROW, *r1 = r0 + SRT_ROW;
  rows::Interval iv;
  rows::interval_setup(r0, r1, S.C, iv);
  long long e = e0;
  for (int s = 0; s < S.n && e < capacity; ++s) {
    if (!(m >> s & 1u)) continue;
    const bool neg0 = surface_g(S.s[s], r0 + 1) < 0.0;
    const double sigma = locate(S.s[s], iv, neg0);
    rows::event_row(iv, r0, r1, sigma, ev_rows + e * SRT_ROW);
    int32_t *q = ev_meta + e * 4;
    q[0] = (int32_t)r;
    q[1] = s;
    q[2] = (int32_t)(j - offsets[r]);
    q[3] = neg0 ? 1 : -1;
    ++e;
  }
}

#if defined(__HIPCC__) && !defined(SRT_CROSSINGS_NO_KERNELS) // (a host-only build has no code object for kernels to live in)
// bit count of row i's mask; item `total` is 0, so that an exclusive sum over total + 1 items ends with the number of events
struct MaskCount {
  const uint16_t *mask;
  long long total;
  __host__ __device__ long long operator()(long long i) const { return i < total ? (long long)__builtin_popcount((unsigned)mask[i]) : 0ll; }
};

__global__ __launch_bounds__(256) void crossings_count_kernel(Surfaces S, long long nrays, const long long *__restrict__ offsets,
                                                              long long total, const double *__restrict__ rows,
                                                              uint16_t *__restrict__ mask) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < total; j += stride)
    mask[j] = (uint16_t)row_mask(S, nrays, offsets, total, rows, j);
}

__global__ __launch_bounds__(256) void crossings_fill_kernel(Surfaces S, long long nrays, const long long *__restrict__ offsets,
                                                             long long total, const double *__restrict__ rows,
                                                             const uint16_t *__restrict__ mask, const long long *__restrict__ evoff,
                                                             long long capacity, double *__restrict__ ev_rows,
                                                             int32_t *__restrict__ ev_meta) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < total; j += stride) {
    const uint32_t m = mask[j];
    if (!m) continue;
    const long long e0 = evoff[j];
    if (e0 >= capacity) continue;
    row_events(S, nrays, offsets, rows, j, m, e0, capacity, ev_rows, ev_meta);
  }
}
#endif

} // namespace crossings
} // namespace srt
