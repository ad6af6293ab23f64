// Device probe of the device-only elementary functions (srt_fastmath.hpp) and of the device build of the T04 EXTERN modules
// (srt_t04.hpp), for tests/test_gpu_fastmath.py.  A library of its own (libsrt_fastmath_probe.so, built by build.py next
// to libsrt_hip.so, which neither links nor knows it).  Plain C entry points on HOST arrays: each allocates, copies, launches,
// copies back and frees by itself and returns 0, or the negated hipError_t of the first HIP call that failed (-1000 for bad
// arguments), so the caller needs numpy and ctypes only and can stop at the first error.
#include <hip/hip_runtime.h>

#include "../../stanford_raytracer_amd/csrc/srt_fastmath.hpp"
#include "../../stanford_raytracer_amd/csrc/srt_t04.hpp"

#define FMO_HD __device__
#include "fastmath_ops.hpp"

namespace {

__global__ void __launch_bounds__(256) fmp_eval_kernel(int op, long n, const double *a, const double *b, double *o0, double *o1) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double r0, r1;
  fm_op(op, a[i], b[i], r0, r1);
  o0[i] = r0;
  o1[i] = r1;
}

// one lane per row: in[14] = PDYN, DST, BYIMF, BZIMF, W1..W6, PS, X, Y, Z; out[33] = the 11 modules of Components, x y z each
// (the order of tests/native/t04_host.cpp::t04h_components)
__global__ void __launch_bounds__(64) fmp_t04_kernel(long n, const double *in, double *out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double *r = in + 14 * i;
  const srt::t04::Components c = srt::t04::external_field(srt::t04::T04D_T04_S_A, r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8],
                                                          r[9], r[10], r[11], r[12], r[13]);
  const srt::t04::V3 v[11] = {c.cf, c.t1, c.t2, c.src, c.prc, c.r11, c.r12, c.r21, c.r22, c.himf, c.total};
  double *o = out + 33 * i;
  for (int k = 0; k < 11; ++k) {
    o[3 * k] = v[k].x;
    o[3 * k + 1] = v[k].y;
    o[3 * k + 2] = v[k].z;
  }
}

struct DevBuf { // frees on every exit path
  void *p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
};

#define FMP_CHECK(call)                      \
  do {                                       \
    const hipError_t e_ = (call);            \
    if (e_ != hipSuccess) {                  \
      (void)hipGetLastError();               \
      return e_ > 0 ? -(int)e_ : -1000;      \
    }                                        \
  } while (0)

} // namespace

extern "C" int fmp_op_count(void) { return FMO_COUNT; }

extern "C" int fmp_eval(int op, long n, const double *a, const double *b, double *o0, double *o1) {
  if (op < 0 || op >= FMO_COUNT || n <= 0 || n > (1L << 27) || !a || !b || !o0 || !o1) return -1000;
  const size_t bytes = (size_t)n * sizeof(double);
  DevBuf da, db, d0, d1;
  FMP_CHECK(hipMalloc(&da.p, bytes));
  FMP_CHECK(hipMalloc(&db.p, bytes));
  FMP_CHECK(hipMalloc(&d0.p, bytes));
  FMP_CHECK(hipMalloc(&d1.p, bytes));
  FMP_CHECK(hipMemcpy(da.p, a, bytes, hipMemcpyHostToDevice));
  FMP_CHECK(hipMemcpy(db.p, b, bytes, hipMemcpyHostToDevice));
  const unsigned blocks = (unsigned)((n + 255) / 256);
  fmp_eval_kernel<<<blocks, 256>>>(op, n, (const double *)da.p, (const double *)db.p, (double *)d0.p, (double *)d1.p);
  FMP_CHECK(hipGetLastError());
  FMP_CHECK(hipDeviceSynchronize());
  FMP_CHECK(hipMemcpy(o0, d0.p, bytes, hipMemcpyDeviceToHost));
  FMP_CHECK(hipMemcpy(o1, d1.p, bytes, hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int fmp_t04_components(long n, const double *in, double *out) {
  if (n <= 0 || n > (1L << 20) || !in || !out) return -1000;
  DevBuf di, dout;
  FMP_CHECK(hipMalloc(&di.p, (size_t)n * 14 * sizeof(double)));
  FMP_CHECK(hipMalloc(&dout.p, (size_t)n * 33 * sizeof(double)));
  FMP_CHECK(hipMemcpy(di.p, in, (size_t)n * 14 * sizeof(double), hipMemcpyHostToDevice));
  const unsigned blocks = (unsigned)((n + 63) / 64);
  fmp_t04_kernel<<<blocks, 64>>>(n, (const double *)di.p, (double *)dout.p);
  FMP_CHECK(hipGetLastError());
  FMP_CHECK(hipDeviceSynchronize());
  FMP_CHECK(hipMemcpy(out, dout.p, (size_t)n * 33 * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}
