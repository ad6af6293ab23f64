// Device probe of the interp model's stencil lookup in both layouts (InterpModel, srt_models.hpp; InterpNodesModel,
// srt_interp_nodes.hpp), for tests/test_gpu_interp_nodes.py: the stencil path without the integrator around it.  Part of the
// probe library (libsrt_fastmath_probe.so, built by build.py; libsrt_hip.so neither links nor knows it).  One plain C entry
// point on HOST arrays in the style of igrf_probe.hip; the two models are handles of the library in the same process, given
// by the device addresses of their structs (srt_model_device_struct).  Returns 0, or the negated hipError_t of the first
// HIP call that failed (-1000 for bad arguments).
#include <hip/hip_runtime.h>

#include "../../stanford_raytracer_amd/csrc/srt_interp_nodes.hpp"

namespace {

// One stencil per lane, 64 lanes per block = one wave; every lane of every block takes part in the (cooperative) lookups, the
// lanes past n repeat stencil n - 1, and only the stores are guarded.  out[3][n][8][4]: density_stencil<1> of the expanded
// layout, of the node table, and the node table's per-point form at the same eight points.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1))) void inp_kernel(const srt::InterpModel *em,
                                                                                          const srt::InterpNodesModel *nm, long n,
                                                                                          const double *c, const double *d,
                                                                                          const double *e, double *out) {
  __shared__ __attribute__((aligned(16))) double tile[srt::TILE_DOUBLES];
  srt::tile_reset(*em, tile);
  const long i = (long)blockIdx.x * 64 + threadIdx.x;
  const long j = i < n ? i : n - 1;
  const double cc[3] = {c[3 * j], c[3 * j + 1], c[3 * j + 2]}, dd[3] = {d[3 * j], d[3 * j + 1], d[3 * j + 2]};
  const double ee[3] = {e[3 * j], e[3 * j + 1], e[3 * j + 2]};
  double A[8][4], B[8][4], P[8][4];
  em->density_stencil<1>(cc, dd, ee, A, tile);
  nm->density_stencil<1>(cc, dd, ee, B, tile);
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    double q[3] = {cc[0], cc[1], cc[2]};
    if (p >= 1 && p <= 6) {
      const int a = (p - 1) >> 1;
      q[a] = ((p - 1) & 1) ? cc[a] - dd[a] : cc[a] + dd[a];
    } else if (p == 7) {
      q[0] = ee[0], q[1] = ee[1], q[2] = ee[2];
    }
    nm->point_direct_exp(q[0], q[1], q[2], P[p]);
  }
  if (i < n) {
#pragma unroll
    for (int p = 0; p < 8; ++p)
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        out[((0 * n + j) * 8 + p) * 4 + s] = A[p][s];
        out[((1 * n + j) * 8 + p) * 4 + s] = B[p][s];
        out[((2 * n + j) * 8 + p) * 4 + s] = P[p][s];
      }
  }
}

struct DevBuf { // frees on every exit path
  void *p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
};

#define INP_CHECK(call)                 \
  do {                                  \
    const hipError_t e_ = (call);       \
    if (e_ != hipSuccess) {             \
      (void)hipGetLastError();          \
      return e_ > 0 ? -(int)e_ : -1000; \
    }                                   \
  } while (0)

} // namespace

// expanded, nodes: device addresses of an InterpModel and an InterpNodesModel of the same grid; c, d, e[n][3]: centres, offsets
// and free points -> out[3][n][8][4]
extern "C" int inp_stencils(const void *expanded, const void *nodes, long n, const double *c, const double *d, const double *e,
                            double *out) {
  if (!expanded || !nodes || !c || !d || !e || !out || n <= 0 || n > (1L << 20)) return -1000;
  const size_t in_bytes = (size_t)n * 3 * sizeof(double), out_bytes = (size_t)n * 3 * 8 * 4 * sizeof(double);
  DevBuf dc, dd, de, dout;
  INP_CHECK(hipMalloc(&dc.p, in_bytes));
  INP_CHECK(hipMalloc(&dd.p, in_bytes));
  INP_CHECK(hipMalloc(&de.p, in_bytes));
  INP_CHECK(hipMalloc(&dout.p, out_bytes));
  INP_CHECK(hipMemcpy(dc.p, c, in_bytes, hipMemcpyHostToDevice));
  INP_CHECK(hipMemcpy(dd.p, d, in_bytes, hipMemcpyHostToDevice));
  INP_CHECK(hipMemcpy(de.p, e, in_bytes, hipMemcpyHostToDevice));
  INP_CHECK(hipMemset(dout.p, 0xff, out_bytes));
  const unsigned blocks = (unsigned)((n + 63) / 64);
  inp_kernel<<<blocks, 64>>>((const srt::InterpModel *)expanded, (const srt::InterpNodesModel *)nodes, n, (const double *)dc.p,
                             (const double *)dd.p, (const double *)de.p, (double *)dout.p);
  INP_CHECK(hipGetLastError());
  INP_CHECK(hipDeviceSynchronize());
  INP_CHECK(hipMemcpy(out, dout.p, out_bytes, hipMemcpyDeviceToHost));
  return 0;
}
