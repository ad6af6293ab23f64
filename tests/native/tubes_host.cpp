// Host build of the ray-tube sections -- stanford_raytracer_amd/csrc/srt_tubes.hpp's search in a neighbour's times, the neighbour's
// position, the section and the whole of a packed row, the very source the device compiles -- for the CPU tests
// (tests/test_tubes_host.py).  Compiled as HIP for the host alone, contraction off.  What is restated here because it lives in the
// kernel and in srt_api_rows.hpp: the loop over the packed rows in place of the launch.
//
// As a program: tubes_host < input, where input is "nrays", nrays lines "b c", nrays + 1 offsets, then the rows (20 numbers each);
// prints one line per packed row: the flag and the four values of the section.
#include <cstdio>
#include <vector>

#define SRT_TUBES_NO_KERNELS
#include "../../stanford_raytracer_amd/csrc/srt_tubes.hpp"

namespace tb = srt::tubes;

// -> 0, or -1 with `why` filled (refused neighbours); section[total][4] and flag[total], either may be null
extern "C" int tbh_tubes(long long nrays, const long long *neighbours, const long long *offsets, const double *rows, double *section,
                         int *flag, char *why, int whylen) {
  if (tb::check_neighbours(nrays, neighbours, why, (size_t)whylen)) return -1;
  const double C = srt::rows::light_speed();
  const long long total = offsets[nrays];
  for (long long j = 0; j < total; ++j) {
    const long long a = srt::rows::ray_of_row(offsets, nrays, j);
    double out[4] = {tb::no_value(), tb::no_value(), tb::no_value(), tb::no_value()};
    const int f = a >= 0 ? tb::row_section(C, offsets, total, rows, neighbours, a, j, out) : tb::NO_TUBE;
    if (section)
      for (int c = 0; c < 4; ++c) section[4 * j + c] = out[c];
    if (flag) flag[j] = f;
  }
  return 0;
}

// the search alone: the i the definition ends with among n rows
extern "C" long long tbh_row_at_or_before(const double *rows, long long n, double t) { return tb::row_at_or_before(rows, n, t); }

int main() {
  long long nrays = 0;
  if (scanf("%lld", &nrays) != 1 || nrays < 0) return 2;
  std::vector<long long> nb((size_t)nrays * 2 + 2), offsets((size_t)nrays + 1);
  for (long long i = 0; i < 2 * nrays; ++i)
    if (scanf("%lld", &nb[i]) != 1) return 2;
  for (auto &o : offsets)
    if (scanf("%lld", &o) != 1) return 2;
  for (long long r = 0; r < nrays; ++r)
    if (offsets[r + 1] < offsets[r] || offsets[0] != 0) return 2;
  const long long total = offsets[nrays];
  std::vector<double> rows((size_t)total * SRT_ROW + 1), section((size_t)total * 4 + 1);
  std::vector<int> flag((size_t)total + 1);
  for (long long i = 0; i < total * SRT_ROW; ++i) {
    char tok[64];
    if (scanf("%63s", tok) != 1 || sscanf(tok, "%lf", &rows[i]) != 1) return 2; // (nan and inf are read as well)
  }
  char why[200];
  if (tbh_tubes(nrays, nb.data(), offsets.data(), rows.data(), section.data(), flag.data(), why, sizeof why)) {
    fprintf(stderr, "%s\n", why);
    return 1;
  }
  for (long long j = 0; j < total; ++j)
    printf("%d %.17g %.17g %.17g %.17g\n", flag[j], section[4 * j], section[4 * j + 1], section[4 * j + 2], section[4 * j + 3]);
  return 0;
}
