// Host build of srt_t04.hpp that records the (x, y) of every t_pow call, for tests/fastmath_cases.py::t04_pow_pairs: the
// header's host branch calls ::pow, which is renamed here for the length of the include -- the header itself is untouched.
#include <math.h>

static double *g_pairs = nullptr;
static long g_cap = 0, g_n = 0;
static inline double t04_logged_pow(double x, double y) {
  if (g_n < g_cap) {
    g_pairs[2 * g_n] = x;
    g_pairs[2 * g_n + 1] = y;
  }
  ++g_n;
  return pow(x, y);
}
#define pow t04_logged_pow
#include "../../stanford_raytracer_amd/csrc/srt_t04.hpp"
#undef pow

// in[14] as t04h_components; appends to pairs[2 * cap]; returns the number of calls made so far (may exceed cap)
extern "C" long t04p_components(const double *in, double *pairs, long cap, long start) {
  g_pairs = pairs;
  g_cap = cap;
  g_n = start;
  const srt::t04::Components c = srt::t04::external_field(srt::t04::T04D_T04_S_A, in[0], in[1], in[2], in[3], in[4], in[5], in[6], in[7],
                                                          in[8], in[9], in[10], in[11], in[12], in[13]);
  (void)c;
  return g_n;
}
