// srt_tubes.hpp -- ray tubes (include/srt.h, "ray tubes"): the cross-section of the tube that a ray and two neighbour rays span, at
// every kept row of the ray.  At the time of a centre row each neighbour is found among its own kept rows (a row hit exactly is
// taken as it stands, otherwise the point of the cubic Hermite curve of srt_rows.hpp between the two rows either side), and the
// section is the area vector of the triangle of the three points and its component along the centre row's group velocity.
//
// Two halves, as srt_crossings.hpp and srt_approaches.hpp have them.  The POINT FUNCTIONS are __host__ __device__ and spell out
// every operation with contraction off, so that a host build (tests/native/tubes_host.cpp) and the device give the same bits:
// only +, -, *, / and sqrt reach an output.  The KERNEL takes one lane per packed centre row.  Its cost is the two searches in the
// neighbours' times, column 0 of their rows at a 160-byte stride.  They are the definition's own binary search, step for step:
// the lanes of a wave are consecutive rows of one ray, so they share the first probes of a search (one address, one fetch) and
// part ways only in the last few.  A shortcut from a neighbouring lane's answer (a wave-wide bracket, a galloping start) gives the
// definition's answer only where the times increase, which the definition does not assume; none is taken.
//
// Compiles for the device (hipcc) and for the host.
#pragma once
#include "srt_rows.hpp"

namespace srt {
namespace tubes {

// the flags of include/srt.h
constexpr int OK = 0, NO_TUBE = 1, BAD_CENTRE = 2, NO_ROW = 3, UNUSABLE = 4, NO_VG = 5;

// Host: the refusals of include/srt.h, by name.  0 = fine; otherwise `why` says what is wrong.
inline int check_neighbours(long long nrays, const long long *nb, char *why, size_t whylen) {
  if (!nb) {
    snprintf(why, whylen, "null neighbours");
    return -1;
  }
  for (long long a = 0; a < nrays; ++a) {
    const long long b = nb[2 * a], c = nb[2 * a + 1];
    if (b == -1 && c == -1) continue;
    if (b == -1 || c == -1) {
      snprintf(why, whylen, "ray %lld: neighbours %lld, %lld: one of a pair is -1 (a ray without a tube has both)", a, b, c);
      return -1;
    }
    if (b < 0 || b >= nrays || c < 0 || c >= nrays) {
      snprintf(why, whylen, "ray %lld: neighbours %lld, %lld: an index outside 0 .. nrays - 1 = %lld", a, b, c, nrays - 1);
      return -1;
    }
    if (b == c || b == a || c == a) {
      snprintf(why, whylen, "ray %lld: neighbours %lld, %lld: a tube takes three different rays", a, b, c);
      return -1;
    }
  }
  return 0;
}

// the quiet NaN every output without a value receives (the same bits on host and device)
ROWS_HD inline double no_value() { return __builtin_nan(""); }

// the search of the definition in the times of n rows: the i = lo - 1 it ends with; -1: no row at or before t
ROWS_HD inline long long row_at_or_before(const double *r, long long n, double t) {
  long long lo = 0, hi = n;
  while (lo < hi) {
    const long long mid = lo + (hi - lo) / 2;
    if (r[mid * SRT_ROW] <= t) lo = mid + 1; // (a NaN compares false)
    else hi = mid;
  }
  return lo - 1;
}

// where a ray of n kept rows r is at time t -> OK and q, or NO_ROW, or UNUSABLE
ROWS_HD inline int neighbour_position(const double *r, long long n, double t, double C, double q[3]) {
  ROWS_NOCONTRACT
  const long long i = row_at_or_before(r, n, t);
  if (i < 0) return NO_ROW;
  const double *r0 = r + i * SRT_ROW;
  if (r0[0] == t) { // the row itself: no curve, no interval
    if (!(__builtin_isfinite(r0[1]) && __builtin_isfinite(r0[2]) && __builtin_isfinite(r0[3]))) return UNUSABLE;
    q[0] = r0[1], q[1] = r0[2], q[2] = r0[3];
    return OK;
  }
  if (i == n - 1) return NO_ROW;
  const double *r1 = r0 + SRT_ROW;
  if (!rows::interval_usable(r0, r1) || !(r1[0] > t)) return UNUSABLE;
  rows::Interval iv;
  rows::interval_setup(r0, r1, C, iv);
  const double sigma = (t - r0[0]) / (r1[0] - r0[0]);
  rows::hermite(iv, sigma, q);
  return OK;
}

// the section at a centre row from the two neighbour positions: out = (Sigma x, y, z, A_perp) -> OK or NO_VG
ROWS_HD inline int section_at(const double *centre, const double qb[3], const double qc[3], double out[4]) {
  ROWS_NOCONTRACT
  const double bx = qb[0] - centre[1], by = qb[1] - centre[2], bz = qb[2] - centre[3];
  const double cx = qc[0] - centre[1], cy = qc[1] - centre[2], cz = qc[2] - centre[3];
  out[0] = 0.5 * (by * cz - bz * cy);
  out[1] = 0.5 * (bz * cx - bx * cz);
  out[2] = 0.5 * (bx * cy - by * cx);
  const double vx = centre[7], vy = centre[8], vz = centre[9];
  const double norm = sqrt(vx * vx + vy * vy + vz * vz);
  if (!(__builtin_isfinite(vx) && __builtin_isfinite(vy) && __builtin_isfinite(vz)) || !(norm > 0.0) || !__builtin_isfinite(norm)) {
    out[3] = no_value();
    return NO_VG;
  }
  out[3] = (out[0] * vx + out[1] * vy + out[2] * vz) / norm;
  return OK;
}

// The whole of packed row j, a row of ray a: the flag, and out[4].  nb = neighbours[nrays][2].  A neighbour whose offsets do not
// lie within 0 .. total in order (which a sound packed set never has) is read as a ray without rows, never beyond the rows.
ROWS_HD inline int row_section(double C, const long long *offsets, long long total, const double *rows, const long long *nb,
                               long long a, long long j, double out[4]) {
  out[0] = out[1] = out[2] = out[3] = no_value();
  const long long b = nb[2 * a], c = nb[2 * a + 1];
  if (b < 0 || c < 0) return NO_TUBE;
  const double *centre = rows + j * SRT_ROW;
  const double t = centre[0];
  if (!(__builtin_isfinite(t) && __builtin_isfinite(centre[1]) && __builtin_isfinite(centre[2]) && __builtin_isfinite(centre[3])))
    return BAD_CENTRE;
  double q[2][3];
  for (int k = 0; k < 2; ++k) { // b before c
    const long long r = k == 0 ? b : c;
    long long o0 = offsets[r], o1 = offsets[r + 1];
    if (o0 < 0 || o1 > total || o1 < o0) o1 = o0 = 0;
    const int f = neighbour_position(rows + o0 * SRT_ROW, o1 - o0, t, C, q[k]);
    if (f != OK) return f;
  }
  double s[4];
  const int f = section_at(centre, q[0], q[1], s);
  out[0] = s[0], out[1] = s[1], out[2] = s[2], out[3] = s[3];
  return f;
}

#if defined(__HIPCC__) && !defined(SRT_TUBES_NO_KERNELS) // (a host-only build has no code object for kernels to live in)
constexpr int BLOCK = 256;

// One lane per packed row; a grid-stride loop over the rows.  section[total][4] and flag[total]; either may be null.
// (A template on its block size: the compiler emits templates behind the plain kernels, with the approaches' and the binning's, so
// this kernel's arrival moves no trace kernel within the code object.)
template <int THREADS>
__global__ __launch_bounds__(THREADS) void tubes_kernel(double C, long long nrays, const long long *__restrict__ offsets, long long total,
                                                        const double *__restrict__ rows, const long long *__restrict__ nb,
                                                        double *__restrict__ section, int32_t *__restrict__ flag) {
  for (long long j = (long long)blockIdx.x * THREADS + threadIdx.x; j < total; j += (long long)gridDim.x * THREADS) {
    const long long a = rows::ray_of_row(offsets, nrays, j);
    double out[4];
    int f = NO_TUBE;
    out[0] = out[1] = out[2] = out[3] = no_value();
    if (a >= 0) f = row_section(C, offsets, total, rows, nb, a, j, out); // (a < 0: offsets[0] > j, which a sound set never has)
    if (section) {
      double *s = section + 4 * j;
      s[0] = out[0], s[1] = out[1], s[2] = out[2], s[3] = out[3];
    }
    if (flag) flag[j] = f;
  }
}
#endif

} // namespace tubes
} // namespace srt
