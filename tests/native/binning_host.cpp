// Host build of the ray binning -- stanford_raytracer_amd/csrc/srt_binning.hpp's coordinate functions, its edge search, its
// samples, weights and deposits and the whole routine of a packed row, the very source the device compiles -- for the CPU tests
// (tests/test_binning_host.py).  Compiled as HIP for the host alone, contraction off.  What is restated here because it lives in
// the kernel and in srt_api_rows.hpp: the loop over the rows in place of the launch, and plain adds in place of the atomics.
#include <cstdio>
#include <vector>

#define SRT_BINNING_NO_KERNELS
#include "../../stanford_raytracer_amd/csrc/srt_binning.hpp"

namespace bn = srt::binning;

struct AccHost {
  long long *ticks, *hits;
  void operator()(long long cell, unsigned long long t, unsigned long long h) const {
    if (ticks) ticks[cell] = (long long)((unsigned long long)ticks[cell] + t);
    if (hits) hits[cell] = (long long)((unsigned long long)hits[cell] + h);
  }
};

// -> 0, or -1 with `why` filled (a refused grid).  ACCUMULATES into ticks[ncells], hits[ncells] (either may be null) and
// counters[4], as the device call does.
extern "C" int bnh_bin(const srt_bin_params *params, long long nrays, const long long *offsets, const double *rows,
                       const double *rowweight, const double *rayweight, long long *ticks, long long *hits, long long *counters,
                       char *why, int whylen) {
  bn::Grid G;
  std::vector<double> edges(3 * (bn::MAXN + 1));
  if (bn::prepare(params, &G, edges.data(), why, (size_t)whylen)) return -1;
  const long long total = offsets[nrays];
  AccHost acc{ticks, hits};
  unsigned long long c[4] = {0, 0, 0, 0};
  for (long long j = 0; j < total; ++j) bn::bin_row(G, edges.data(), nrays, offsets, total, rows, rowweight, rayweight, j, acc, c);
  for (int k = 0; k < 4; ++k) counters[k] += (long long)c[k];
  return 0;
}

extern "C" long long bnh_cells(const srt_bin_params *params, char *why, int whylen) {
  bn::Grid G;
  std::vector<double> edges(3 * (bn::MAXN + 1));
  if (bn::prepare(params, &G, edges.data(), why, (size_t)whylen)) return -1;
  return G.ncells;
}

extern "C" double bnh_coordinate(int kind, const double *x) { return bn::coordinate(kind, x); }
extern "C" int bnh_find_cell(const double *edges, int n, double c) { return bn::find_cell(edges, n, c); }
