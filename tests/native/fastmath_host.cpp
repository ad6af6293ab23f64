// Host emulation of stanford_raytracer_amd/csrc/srt_fastmath.hpp for tests/test_fastmath_host.py: the unmodified header,
// compiled by g++ with tests/native/hip_stub first on the include path (exact 1/b and 1/sqrt(x) in place of the hardware's
// seeds).  Same op codes as the device probe (fastmath_ops.hpp).
#include "../../stanford_raytracer_amd/csrc/srt_fastmath.hpp"
#include "fastmath_ops.hpp"

extern "C" int fmh_eval(int op, long n, const double *a, const double *b, double *o0, double *o1) {
  if (op < 0 || op >= FMO_COUNT || n < 0) return -1;
  for (long i = 0; i < n; ++i) fm_op(op, a[i], b[i], o0[i], o1[i]);
  return 0;
}
