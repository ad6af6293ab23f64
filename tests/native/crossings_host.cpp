// Host build of the surface-crossing finder -- stanford_raytracer_amd/csrc/srt_crossings.hpp's g, its Hermite curve in the Delta
// form, its bisection, the mask of a packed row and the events of a row, the very source the device compiles -- for the CPU tests
// (tests/test_crossings_host.py).  Compiled as HIP for the host alone, contraction off.  What is restated here because it lives
// in srt_api_rows.hpp: the loop over the rows in place of the two launches, and the running sum in place of the device scan.
//
// As a program: crossings_host < input, where input is "nsurf nrays capacity", nsurf lines "kind p0 p1 p2 p3", nrays + 1 offsets,
// then the rows (20 numbers each); prints the total, then one line per kept event: ray surface interval direction and the row.
#include <cstdio>
#include <vector>

#define SRT_CROSSINGS_NO_KERNELS
#include "../../stanford_raytracer_amd/csrc/srt_crossings.hpp"

namespace cx = srt::crossings;

// -> 0, or -1 with `why` filled (a refused surface); *count = all events, the first min(count, capacity) are written
extern "C" int cxh_crossings(int nsurf, const srt_surface *surfaces, long long nrays, const long long *offsets, const double *rows,
                             long long capacity, double *ev_rows, int *ev_meta, long long *count, char *why, int whylen) {
  cx::Surfaces S;
  if (cx::prepare(nsurf, surfaces, &S, why, (size_t)whylen)) return -1;
  const long long total = offsets[nrays];
  long long e = 0;
  for (long long j = 0; j < total; ++j) {
    const uint32_t m = cx::row_mask(S, nrays, offsets, total, rows, j);
    if (!m) continue;
    if (e < capacity) cx::row_events(S, nrays, offsets, rows, j, m, e, capacity, ev_rows, ev_meta);
    e += __builtin_popcount(m);
  }
  *count = e;
  return 0;
}

extern "C" double cxh_light_speed() { return cx::light_speed(); }

int main() {
  int nsurf = 0;
  long long nrays = 0, capacity = 0;
  if (scanf("%d %lld %lld", &nsurf, &nrays, &capacity) != 3 || nsurf < 0 || nsurf > 64 || nrays < 0 || capacity < 0) return 2;
  std::vector<srt_surface> surf((size_t)nsurf + 1);
  for (int s = 0; s < nsurf; ++s) {
    double kind;
    if (scanf("%lf %lf %lf %lf %lf", &kind, &surf[s].p[0], &surf[s].p[1], &surf[s].p[2], &surf[s].p[3]) != 5) return 2;
    surf[s].kind = (int32_t)kind;
    surf[s].reserved = 0;
  }
  std::vector<long long> offsets((size_t)nrays + 1);
  for (auto &o : offsets)
    if (scanf("%lld", &o) != 1) return 2;
  for (long long r = 0; r < nrays; ++r)
    if (offsets[r + 1] < offsets[r] || offsets[0] != 0) return 2;
  const long long total = offsets[nrays];
  std::vector<double> rows((size_t)total * SRT_ROW + 1);
  for (long long i = 0; i < total * SRT_ROW; ++i)
    if (scanf("%lf", &rows[i]) != 1) return 2;
  std::vector<double> ev((size_t)capacity * SRT_ROW + 1);
  std::vector<int> meta((size_t)capacity * 4 + 1);
  long long count = 0;
  char why[200];
  if (cxh_crossings(nsurf, surf.data(), nrays, offsets.data(), rows.data(), capacity, ev.data(), meta.data(), &count, why, sizeof why)) {
    fprintf(stderr, "%s\n", why);
    return 1;
  }
  printf("%lld\n", count);
  for (long long e = 0; e < count && e < capacity; ++e) {
    printf("%d %d %d %d", meta[4 * e], meta[4 * e + 1], meta[4 * e + 2], meta[4 * e + 3]);
    for (int c = 0; c < SRT_ROW; ++c) printf(" %.17g", ev[(size_t)e * SRT_ROW + c]);
    printf("\n");
  }
  return 0;
}
