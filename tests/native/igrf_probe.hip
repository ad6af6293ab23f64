// Device probe of the IGRF synthesis igrf_core<NP> (stanford_raytracer_amd/csrc/srt_device.hpp), for tests/test_igrf_edges.py.
// Part of the probe library (libsrt_fastmath_probe.so, built by build.py; libsrt_hip.so neither links nor knows it).  One
// plain C entry point on HOST arrays in the style of fastmath_probe.hip: it allocates, copies, launches, copies back, frees,
// and returns 0, or the negated hipError_t of the first HIP call that failed (-1000 for bad arguments).
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../stanford_raytracer_amd/csrc/srt_device.hpp"

namespace {

// One stencil of NP points per lane, 64 lanes per block = one wave.  EVERY lane of every block runs the synthesis (its
// terms are read across the wave with v_readlane): the index is clamped as in the layered kernels, so the lanes past n repeat
// stencil n - 1, and only the store is guarded.
template <int NP>
__global__ void __launch_bounds__(64) igp_kernel(const srt::FieldConst *f, long n, const float *pos, float *out) {
  const long i = (long)blockIdx.x * 64 + threadIdx.x;
  const long j = i < n ? i : n - 1;
  float xg[NP], yg[NP], zg[NP], hx[NP], hy[NP], hz[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    xg[p] = pos[(j * NP + p) * 3];
    yg[p] = pos[(j * NP + p) * 3 + 1];
    zg[p] = pos[(j * NP + p) * 3 + 2];
  }
  srt::igrf_core<NP>(*f, xg, yg, zg, hx, hy, hz);
  if (i < n) {
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      out[(j * NP + p) * 3] = hx[p];
      out[(j * NP + p) * 3 + 1] = hy[p];
      out[(j * NP + p) * 3 + 2] = hz[p];
    }
  }
}

struct DevBuf { // frees on every exit path
  void *p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
};

#define IGP_CHECK(call)                      \
  do {                                       \
    const hipError_t e_ = (call);            \
    if (e_ != hipSuccess) {                  \
      (void)hipGetLastError();               \
      return e_ > 0 ? -(int)e_ : -1000;      \
    }                                        \
  } while (0)

} // namespace

// G, H, REC in geopack's index n(n-1)/2 + m, A row-major (GEO -> GSW); np = 1, 7 or 8 points per stencil;
// pos[n][np][3] GSW positions in Earth radii -> out[n][np][3] nT
extern "C" int igp_igrf(const float *G, const float *H, const float *REC, const float *A, int np, long n, const float *pos,
                        float *out) {
  if (!G || !H || !REC || !A || !pos || !out || n <= 0 || n > (1L << 20) || (np != 1 && np != 7 && np != 8)) return -1000;
  srt::FieldConst fc;
  memset(&fc, 0, sizeof fc);
  srt::igrf_pack_terms(G, H, REC, fc);
  for (int k = 0; k < 9; ++k) fc.A[k] = A[k];
  fc.use_igrf = 1;
  const size_t bytes = (size_t)n * np * 3 * sizeof(float);
  DevBuf df, dp, dout;
  IGP_CHECK(hipMalloc(&df.p, sizeof fc));
  IGP_CHECK(hipMalloc(&dp.p, bytes));
  IGP_CHECK(hipMalloc(&dout.p, bytes));
  IGP_CHECK(hipMemcpy(df.p, &fc, sizeof fc, hipMemcpyHostToDevice));
  IGP_CHECK(hipMemcpy(dp.p, pos, bytes, hipMemcpyHostToDevice));
  IGP_CHECK(hipMemset(dout.p, 0xff, bytes));
  const unsigned blocks = (unsigned)((n + 63) / 64);
  const srt::FieldConst *f = (const srt::FieldConst *)df.p;
  if (np == 1) igp_kernel<1><<<blocks, 64>>>(f, n, (const float *)dp.p, (float *)dout.p);
  else if (np == 7) igp_kernel<7><<<blocks, 64>>>(f, n, (const float *)dp.p, (float *)dout.p);
  else igp_kernel<8><<<blocks, 64>>>(f, n, (const float *)dp.p, (float *)dout.p);
  IGP_CHECK(hipGetLastError());
  IGP_CHECK(hipDeviceSynchronize());
  IGP_CHECK(hipMemcpy(out, dout.p, bytes, hipMemcpyDeviceToHost));
  return 0;
}
