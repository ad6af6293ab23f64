// Host build of the closest-approach finder -- stanford_raytracer_amd/csrc/srt_approaches.hpp's hull reject, its test function f,
// its bisection, the per-pair decision and the walk of a row over the observers, the very source the device compiles -- for the
// CPU tests (tests/test_approaches_host.py).  Compiled as HIP for the host alone, contraction off.  What is restated here because
// it lives in the kernels and in srt_api_rows.hpp: the loop over the rows in place of the two launches, the whole observer array in
// place of the LDS tiles, and the running sum in place of the device scan.
//
// As a program: approaches_host < input, where input is "nobs nrays capacity", nobs lines "x y z radius", nrays + 1 offsets, then
// the rows (20 numbers each); prints the total, then one line per kept event: ray observer interval 0, the distance and the row.
#include <cstdio>
#include <vector>

#define SRT_CROSSINGS_NO_KERNELS
#define SRT_APPROACHES_NO_KERNELS
#include "../../stanford_raytracer_amd/csrc/srt_approaches.hpp"

namespace ap = srt::approaches;

// -> 0, or -1 with `why` filled (refused observers); *count = all events, the first min(count, capacity) are written.
extern "C" int aph_approaches(int nobs, const srt_observer *observers, long long nrays, const long long *offsets, const double *rows,
                              long long capacity, double *ev_rows, int *ev_meta, double *ev_dist, long long *count, char *why,
                              int whylen) {
  if (ap::check_observers(nobs, observers, why, (size_t)whylen)) return -1;
  const double C = srt::crossings::light_speed();
  const long long total = offsets[nrays];
  long long e = 0;
  for (long long j = 0; j + 1 < total; ++j) {
    const double *r0 = rows + j * SRT_ROW, *r1 = r0 + SRT_ROW;
    if (!ap::interval_usable(r0, r1)) continue;
    ap::Ball B;
    ap::ball_of(r0, r1, C, B);
    // the count pass of the row, then the fill pass of a row that has events, as the device has them
    ap::RowState st;
    st.ray = -2, st.e = 0, st.n = 0, st.live = true;
    ap::row_walk(B, C, r0, r1, nrays, offsets, j, observers, nobs, 0, st, 0u, 0, nullptr, nullptr, nullptr);
    const unsigned want = st.n;
    if (want && e < capacity) {
      st.ray = -2, st.e = e, st.n = 0, st.live = true;
      ap::row_walk(B, C, r0, r1, nrays, offsets, j, observers, nobs, 0, st, want, capacity, ev_rows, ev_meta, ev_dist);
    }
    e += want;
  }
  *count = e;
  return 0;
}

// the definition without the reject: the number of events, for the tests that the reject changes nothing
extern "C" long long aph_count_without_reject(int nobs, const srt_observer *observers, long long nrays, const long long *offsets,
                                              const double *rows) {
  const double C = srt::crossings::light_speed();
  long long n = 0;
  for (long long r = 0; r < nrays; ++r)
    for (long long j = offsets[r]; j + 1 < offsets[r + 1]; ++j) {
      const double *r0 = rows + j * SRT_ROW, *r1 = r0 + SRT_ROW;
      if (!ap::interval_usable(r0, r1)) continue;
      ap::Prepared P;
      ap::prepare(r0, r1, C, P);
      for (int m = 0; m < nobs; ++m) {
        double sigma, dist;
        if (ap::holds_approach(P, observers[m]) && ap::approach_event(P, observers[m], &sigma, &dist)) ++n;
      }
    }
  return n;
}

// how many pairs of usable intervals the hull test lets through (so that a test can see that it rejects at all)
extern "C" long long aph_survivors(int nobs, const srt_observer *observers, long long nrays, const long long *offsets, const double *rows) {
  const double C = srt::crossings::light_speed();
  long long n = 0;
  for (long long r = 0; r < nrays; ++r)
    for (long long j = offsets[r]; j + 1 < offsets[r + 1]; ++j) {
      const double *r0 = rows + j * SRT_ROW, *r1 = r0 + SRT_ROW;
      if (!ap::interval_usable(r0, r1)) continue;
      ap::Ball B;
      ap::ball_of(r0, r1, C, B);
      for (int m = 0; m < nobs; ++m) n += ap::too_far(B, observers[m]) ? 0 : 1;
    }
  return n;
}

int main() {
  int nobs = 0;
  long long nrays = 0, capacity = 0;
  if (scanf("%d %lld %lld", &nobs, &nrays, &capacity) != 3 || nobs < 0 || nobs > SRT_MAXOBS || nrays < 0 || capacity < 0) return 2;
  std::vector<srt_observer> obs((size_t)nobs + 1);
  for (int m = 0; m < nobs; ++m)
    if (scanf("%lf %lf %lf %lf", &obs[m].x[0], &obs[m].x[1], &obs[m].x[2], &obs[m].radius) != 4) return 2;
  std::vector<long long> offsets((size_t)nrays + 1);
  for (auto &o : offsets)
    if (scanf("%lld", &o) != 1) return 2;
  for (long long r = 0; r < nrays; ++r)
    if (offsets[r + 1] < offsets[r] || offsets[0] != 0) return 2;
  const long long total = offsets[nrays];
  std::vector<double> rows((size_t)total * SRT_ROW + 1);
  for (long long i = 0; i < total * SRT_ROW; ++i)
    if (scanf("%lf", &rows[i]) != 1) return 2;
  std::vector<double> ev((size_t)capacity * SRT_ROW + 1), dist((size_t)capacity + 1);
  std::vector<int> meta((size_t)capacity * 4 + 1);
  long long count = 0;
  char why[200];
  if (aph_approaches(nobs, obs.data(), nrays, offsets.data(), rows.data(), capacity, ev.data(), meta.data(), dist.data(), &count, why,
                     sizeof why)) {
    fprintf(stderr, "%s\n", why);
    return 1;
  }
  printf("%lld\n", count);
  for (long long e = 0; e < count && e < capacity; ++e) {
    printf("%d %d %d %d %.17g", meta[4 * e], meta[4 * e + 1], meta[4 * e + 2], meta[4 * e + 3], dist[e]);
    for (int c = 0; c < SRT_ROW; ++c) printf(" %.17g", ev[(size_t)e * SRT_ROW + c]);
    printf("\n");
  }
  return 0;
}
