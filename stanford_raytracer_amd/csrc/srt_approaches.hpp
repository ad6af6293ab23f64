// srt_approaches.hpp -- each ray's closest approach to observer points (include/srt.h, "closest approaches"): on the cubic
// Hermite curve through two consecutive kept rows (srt_rows.hpp), the test function f = (p - o) . p', the bisection that locates its
// change from < 0 to >= 0, the distance there, and the two passes over packed rows x observers.
//
// Two halves, as srt_crossings.hpp has them.  The POINT FUNCTIONS are __host__ __device__ and spell out every operation with
// contraction off, so that a host build (tests/native/approaches_host.cpp) and the device give the same bits: only +, -, * and
// sqrt reach an event.  The interval, the curve, the event's row and the search in offsets are srt_rows.hpp's.
// The KERNELS take one lane per packed row (the interval that starts there) and walk the observers, staged through LDS in tiles
// that every lane reads at the same address (a broadcast).  A pair is first held against the hull of the cubic's Bezier points
// -- about ten fp64 instructions -- and only a survivor pays for the end signs and the bisection.  A count pass writes one uint32
// per row, a prefix sum lies between (srt_api_rows.hpp), and a fill pass recounts the rows that have events and writes them at the
// scanned position: that is what puts the events in (ray, interval, observer) order.
//
// Compiles for the device (hipcc) and for the host.
#pragma once
#include "srt_crossings.hpp" // (crossings::light_speed, which callers of this header pass as C; the curve: srt_rows.hpp)

namespace srt {
namespace approaches {

// Host: the refusals of include/srt.h, by name.  0 = fine; otherwise `why` says what is wrong.
inline int check_observers(int nobs, const srt_observer *in, char *why, size_t whylen) {
  if (nobs < 1 || nobs > SRT_MAXOBS) {
    snprintf(why, whylen, "nobs = %d is outside 1 .. %d (SRT_MAXOBS)", nobs, SRT_MAXOBS);
    return -1;
  }
  if (!in) {
    snprintf(why, whylen, "null observers");
    return -1;
  }
  for (int i = 0; i < nobs; ++i) {
    for (int c = 0; c < 3; ++c)
      if (!__builtin_isfinite(in[i].x[c])) {
        snprintf(why, whylen, "observer %d: coordinate x[%d] is not finite", i, c);
        return -1;
      }
    if (!__builtin_isfinite(in[i].radius) || !(in[i].radius > 0.0)) {
      snprintf(why, whylen, "observer %d: radius %g is not finite and > 0", i, in[i].radius);
      return -1;
    }
  }
  return 0;
}

// usable for approaches: the condition of every packed-row consumer, and time runs forward
ROWS_HD inline bool interval_usable(const double *r0, const double *r1) { return rows::interval_usable(r0, r1) && r1[0] > r0[0]; }

// An interval as a pair that survives the hull test reads it: the curve and the far end as the rows give it
// (p1, m1 = C vg1 h).
struct Prepared {
  rows::Interval iv;
  double p1[3], m1[3];
};
ROWS_HD inline void prepare(const double *r0, const double *r1, double C, Prepared &P) {
  ROWS_NOCONTRACT
  rows::interval_setup(r0, r1, C, P.iv);
  for (int c = 0; c < 3; ++c) {
    P.p1[c] = r1[1 + c];
    P.m1[c] = C * r1[7 + c] * P.iv.h;
  }
}

// The ball that holds the curve, which is all the hull test reads (and all a lane keeps in registers while it walks the
// observers): centre c = (p0 + p1) / 2, `reach` = the largest distance of the Bezier points p0, p0 + m0 / 3, p1 - m1 / 3, p1
// from c (a cubic lies in their hull) plus 2^-40 (|c|_1 + itself), far more than the rounding of c, of the radius and of the
// curve's evaluation.  A reach that is not finite rejects nothing.
struct Ball {
  double c[3], reach;
};
ROWS_HD inline void ball_of(const double *r0, const double *r1, double C, Ball &B) {
  ROWS_NOCONTRACT
  const double h = r1[0] - r0[0];
  double q[4] = {0.0, 0.0, 0.0, 0.0}, mag = 0.0;
  for (int c = 0; c < 3; ++c) {
    const double m0 = C * r0[7 + c] * h, m1 = C * r1[7 + c] * h;
    B.c[c] = 0.5 * r0[1 + c] + 0.5 * r1[1 + c];
    mag = mag + fabs(B.c[c]);
    const double b0 = r0[1 + c] - B.c[c], b3 = r1[1 + c] - B.c[c];
    const double b1 = b0 + m0 * (1.0 / 3.0), b2 = b3 - m1 * (1.0 / 3.0);
    q[0] = q[0] + b0 * b0;
    q[1] = q[1] + b1 * b1;
    q[2] = q[2] + b2 * b2;
    q[3] = q[3] + b3 * b3;
  }
  double rho2 = q[0];
  for (int k = 1; k < 4; ++k) rho2 = (q[k] > rho2 || q[k] != q[k]) ? q[k] : rho2; // (a NaN stays)
  const double rho = sqrt(rho2);
  B.reach = rho + 0x1p-40 * (mag + rho);
}

// the conservative reject: |o - c| > (radius + reach)(1 + 2^-20) cannot hold an event.  Anything not finite compares false or
// rejects only what is truly far.
ROWS_HD inline bool too_far(const Ball &B, const srt_observer &o) {
  ROWS_NOCONTRACT
  const double dx = o.x[0] - B.c[0], dy = o.x[1] - B.c[1], dz = o.x[2] - B.c[2];
  const double d2 = dx * dx + dy * dy + dz * dz;
  const double thr = (o.radius + B.reach) * (1.0 + 0x1p-20);
  return d2 > thr * thr;
}

// f at an end, from the row itself: (p - o) . m
ROWS_HD inline double end_f(const double p[3], const double m[3], const srt_observer &o) {
  ROWS_NOCONTRACT
  return (p[0] - o.x[0]) * m[0] + (p[1] - o.x[1]) * m[1] + (p[2] - o.x[2]) * m[2];
}

// f(sigma) = (p(sigma) - o) . p'(sigma)
ROWS_HD inline double approach_f(const rows::Interval &iv, const srt_observer &o, double sigma) {
  ROWS_NOCONTRACT
  double f = 0.0;
  for (int c = 0; c < 3; ++c) {
    const double x = iv.p0[c] + sigma * (iv.m0[c] + sigma * (iv.c2[c] + sigma * iv.c3[c]));
    const double v = iv.m0[c] + sigma * (2.0 * iv.c2[c] + 3.0 * sigma * iv.c3[c]);
    const double t = (x - o.x[c]) * v;
    f = c == 0 ? t : f + t;
  }
  return f;
}

// does the interval hold an approach of o: f(0) < 0 and !(f(1) < 0)
ROWS_HD inline bool holds_approach(const Prepared &P, const srt_observer &o) {
  return end_f(P.iv.p0, P.iv.m0, o) < 0.0 && !(end_f(P.p1, P.m1, o) < 0.0);
}

// sigma*: the crossings' locate with neg0 = true, on f
ROWS_HD inline double locate(const rows::Interval &iv, const srt_observer &o) {
  ROWS_NOCONTRACT
  double lo = 0.0, hi = 1.0;
  for (int it = 0; it < rows::BISECTIONS; ++it) {
    const double mid = 0.5 * (lo + hi);
    if (approach_f(iv, o, mid) < 0.0) lo = mid;
    else hi = mid;
  }
  return hi;
}

// the distance at sigma
ROWS_HD inline double distance_at(const rows::Interval &iv, const srt_observer &o, double sigma) {
  ROWS_NOCONTRACT
  double x[3];
  rows::hermite(iv, sigma, x);
  const double dx = x[0] - o.x[0], dy = x[1] - o.x[1], dz = x[2] - o.x[2];
  return sqrt(dx * dx + dy * dy + dz * dz);
}

// The per-(interval, observer) decision behind the reject and the end signs: locate, measure, compare.
ROWS_HD inline bool approach_event(const Prepared &P, const srt_observer &o, double *sigma, double *dist) {
  *sigma = locate(P.iv, o);
  *dist = distance_at(P.iv, o, *sigma);
  return *dist <= o.radius;
}

ROWS_HD inline void write_event(const Prepared &P, const double *r0, const double *r1, double sigma, double dist, long long ray,
                                int obs, long long interval, long long e, double *ev_rows, int32_t *ev_meta, double *ev_dist) {
  rows::event_row(P.iv, r0, r1, sigma, ev_rows + e * SRT_ROW);
  int32_t *q = ev_meta + e * 4;
  q[0] = (int32_t)ray;
  q[1] = obs;
  q[2] = (int32_t)interval;
  q[3] = 0;
  ev_dist[e] = dist;
}

// The events of packed row j against observers obs[0 .. n), which carry the indices first, first + 1, ..: the walk both passes
// and the host build share.  `state` lives across the tiles of one row.  Counting: ev_rows == nullptr.  Filling: event number
// st.e onwards is written while it is below capacity, and the walk ends after `want` events.
struct RowState {
  long long ray, e; // ray: -2 not looked up yet
  uint32_t n;       // events so far
  bool live;
};
// one pair that the hull test let through; false: the walk of this row is over
ROWS_HD inline bool row_pair(double C, const double *r0, const double *r1, long long nrays, const long long *offsets,
                             long long j, const srt_observer &o, int index, RowState &st, uint32_t want, long long capacity,
                             double *ev_rows, int32_t *ev_meta, double *ev_dist) {
  Prepared P; // (made again for each of the few survivors, from rows the caches hold: the walk itself keeps only the ball)
  prepare(r0, r1, C, P);
  if (!holds_approach(P, o)) return true;
  if (st.ray == -2) { // only a row with a survivor pays for the search in offsets
    st.ray = rows::interval_ray(offsets, nrays, j);
    if (st.ray < 0) {
      st.live = false;
      return false;
    }
  }
  double sigma, dist;
  if (!approach_event(P, o, &sigma, &dist)) return true;
  if (ev_rows) {
    if (st.e < capacity) write_event(P, r0, r1, sigma, dist, st.ray, index, j - offsets[st.ray], st.e, ev_rows, ev_meta, ev_dist);
    ++st.e;
    if (++st.n == want || st.e >= capacity) {
      st.live = false;
      return false;
    }
  } else {
    ++st.n;
  }
  return true;
}
// The hull test runs over WALK observers at a time without a branch, so that their reads are in flight together; the few pairs
// it lets through are then taken in ascending order.
constexpr int WALK = 8;
ROWS_HD inline void row_walk(const Ball &B, double C, const double *r0, const double *r1, long long nrays, const long long *offsets,
                             long long j, const srt_observer *obs, int n, int first, RowState &st, uint32_t want, long long capacity,
                             double *ev_rows, int32_t *ev_meta, double *ev_dist) {
  int m = 0;
  for (; m + WALK <= n; m += WALK) {
    unsigned near = 0u;
#pragma unroll
    for (int u = 0; u < WALK; ++u) near |= too_far(B, obs[m + u]) ? 0u : 1u << u;
    while (near) {
      const int u = __builtin_ctz(near);
      near &= near - 1u;
      if (!row_pair(C, r0, r1, nrays, offsets, j, obs[m + u], first + m + u, st, want, capacity, ev_rows, ev_meta, ev_dist)) return;
    }
  }
  for (; m < n; ++m)
    if (!too_far(B, obs[m]) && !row_pair(C, r0, r1, nrays, offsets, j, obs[m], first + m, st, want, capacity, ev_rows, ev_meta, ev_dist))
      return;
}

#if defined(__HIPCC__) && !defined(SRT_APPROACHES_NO_KERNELS) // (a host-only build has no code object for kernels to live in)
constexpr int BLOCK = 256;
constexpr int TILE = 1024; // observers per LDS tile: 32 B each, 32 KiB
static_assert(sizeof(srt_observer) == 32, "an observer is 32 bytes");

// row i's count as the scan reads it; item `total` is 0, so that an exclusive sum over total + 1 items ends with the total
struct RowCount {
  const uint32_t *count;
  long long total;
  __host__ __device__ long long operator()(long long i) const { return i < total ? (long long)count[i] : 0ll; }
};

// FILL = false: count[j] = the number of events of the interval that starts at packed row j (0 for a ray's last row).
// FILL = true: rows with count[j] > 0 are walked again and their events written from evoff[j] on.
// One block takes BLOCK consecutive rows at a time and every tile of observers in turn; the loops and barriers are uniform.
template <bool FILL>
__global__ __launch_bounds__(BLOCK) void approaches_kernel(double C, int nobs, const srt_observer *__restrict__ obs, long long nrays,
                                                           const long long *__restrict__ offsets, long long total,
                                                           const double *__restrict__ rows, uint32_t *__restrict__ count,
                                                           const long long *__restrict__ evoff, long long capacity,
                                                           double *__restrict__ ev_rows, int32_t *__restrict__ ev_meta,
                                                           double *__restrict__ ev_dist) {
  __shared__ srt_observer tile[TILE];
  const long long nchunks = (total + BLOCK - 1) / BLOCK;
  for (long long chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const long long j = chunk * BLOCK + threadIdx.x;
    const double *r0 = rows + j * SRT_ROW, *r1 = r0 + SRT_ROW;
    RowState st;
    st.ray = -2, st.e = 0, st.n = 0;
    st.live = j + 1 < total && interval_usable(r0, r1);
    uint32_t want = 0;
    if (FILL) {
      if (st.live) want = count[j];
      st.live = want > 0;
      if (st.live) st.e = evoff[j];
      if (st.e >= capacity) st.live = false;
    }
    if (!__syncthreads_or(st.live ? 1 : 0)) { // (also the barrier between the last tile's readers and the next staging)
      if (!FILL && j < total) count[j] = 0u;
      continue;
    }
    Ball B;
    if (st.live) ball_of(r0, r1, C, B);
    for (int t0 = 0; t0 < nobs; t0 += TILE) {
      const int nt = nobs - t0 < TILE ? nobs - t0 : TILE;
      if (t0 > 0) __syncthreads();
      {
        const double *src = (const double *)(obs + t0);
        double *dst = (double *)tile;
        for (int i = threadIdx.x; i < nt * 4; i += BLOCK) dst[i] = src[i];
      }
      __syncthreads();
      if (st.live) row_walk(B, C, r0, r1, nrays, offsets, j, tile, nt, t0, st, want, capacity, FILL ? ev_rows : nullptr, ev_meta, ev_dist);
    }
    if (!FILL && j < total) count[j] = st.n;
  }
}
#endif

} // namespace approaches
} // namespace srt
