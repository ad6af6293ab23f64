// srt_api_grid.hpp -- modelnum 3 and the regular grids around it: the finite-difference and coefficient kernels with their
// constant tables, the two table layouts and the choice between them, the interp constructors (from arrays, from another model,
// from a grid file), the grid sampler behind srt_build_grid, and dumpmodel.
// A part of srt_api.hip (srt_api_core.hpp).
#pragma once
#include "srt_api_core.hpp"
#include "srt_api_model.hpp"
#include "srt_host.hpp"
#include "srt_kernels.hpp"
#include "srt_interp_nodes.hpp"
#include "srt_xform.hpp"

// ---- interp: finite-difference derivatives + coefficient expansion on the device --------------------
struct GridDims {
  int nspec, nx, ny, nz;
};
__device__ __forceinline__ size_t gidx(const GridDims &g, int s, int i, int j, int k) {
  return (((size_t)k * g.ny + j) * g.nx + i) * g.nspec + s;
}
// tricubic_compute_finite_difference_derivatives, one axis (libtricubic.f95:736-790)
__global__ void fd_axis_kernel(GridDims g, const double *src, double *dst, int axis, double h) {
  size_t total = (size_t)g.nspec * g.nx * g.ny * g.nz;
  for (size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (size_t)gridDim.x * blockDim.x) {
    int s = (int)(id % g.nspec);
    size_t r = id / g.nspec;
    int i = (int)(r % g.nx);
    r /= g.nx;
    int j = (int)(r % g.ny);
    int k = (int)(r / g.ny);
    int c[3] = {i, j, k};
    int n[3] = {g.nx, g.ny, g.nz};
    int lo[3] = {i, j, k}, hi[3] = {i, j, k};
    int a = c[axis], na = n[axis];
    double v;
    if (a == 0) {
      hi[axis] = 1;
      v = (src[gidx(g, s, hi[0], hi[1], hi[2])] - src[gidx(g, s, lo[0], lo[1], lo[2])]) / h;
    } else if (a == na - 1) {
      lo[axis] = na - 2;
      v = (src[gidx(g, s, hi[0], hi[1], hi[2])] - src[gidx(g, s, lo[0], lo[1], lo[2])]) / h;
    } else {
      lo[axis] = a - 1;
      hi[axis] = a + 1;
      v = (src[gidx(g, s, hi[0], hi[1], hi[2])] - src[gidx(g, s, lo[0], lo[1], lo[2])]) / 2.0 / h;
    }
    dst[id] = v;
  }
}

struct ArrPtrs {
  const double *a[8];
};
__constant__ short c_tri_ptr[65];
__constant__ signed char c_tri_col[TRI_NNZ];
__constant__ signed char c_tri_val[TRI_NNZ];

// tricubic_get_coeff for every cell (libtricubic.f95:638-656,715-720) with the corner gathering,
// clamping and sticky derivative-zeroing flags of tricubic_interpolate_at (:859-921; SURVEY A-7).
// One 64-thread block per (cell, species): thread t first gathers constraint b[t] (t = 8*family +
// corner), then computes coefficient row t of the sparse 64x64 product.
__global__ __launch_bounds__(64) void build_coeffs_kernel(GridDims g, ArrPtrs arrs, double dx, double dy, double dz,
                                                          double *coef, long long npairs) {
  __shared__ double b[64];
  const int t = threadIdx.x;
  const int q = t >> 3, l = t & 7;
  for (long long pair = blockIdx.x; pair < npairs; pair += gridDim.x) {
    long long cell = pair / g.nspec;
    int s = (int)(pair % g.nspec);
    int ci = (int)(cell % (g.nx + 1));
    long long r = cell / (g.nx + 1);
    int cj = (int)(r % (g.ny + 1));
    int ck = (int)(r / (g.ny + 1));
    int it = ci + (l & 1), jt = cj + ((l >> 1) & 1), kt = ck + (l >> 2); // 1-based corner indices
    it = it < 1 ? 1 : (it > g.nx ? g.nx : it);
    jt = jt < 1 ? 1 : (jt > g.ny ? g.ny : jt);
    kt = kt < 1 ? 1 : (kt > g.nz ? g.nz : kt);
    // flags are set by the first clamped corner and never reset inside the corner loop
    bool fi = (ci == 0) || (ci == g.nx && l >= 1);
    bool fj = (cj == 0) || (cj == g.ny && l >= 2);
    bool fk = (ck == 0) || (ck == g.nz && l >= 4);
    double v = arrs.a[q][gidx(g, s, it - 1, jt - 1, kt - 1)];
    bool zero = false;
    switch (q) {
    case 1: v = v * dx; zero = fi; break;
    case 2: v = v * dy; zero = fj; break;
    case 3: v = v * dz; zero = fk; break;
    case 4: v = v * dx * dy; zero = fi || fj; break;
    case 5: v = v * dx * dz; zero = fi || fk; break;
    case 6: v = v * dy * dz; zero = fj || fk; break;
    case 7: v = v * dx * dy * dz; zero = fi || fj || fk; break;
    default: break;
    }
    __syncthreads();
    b[t] = zero ? 0.0 : v;
    __syncthreads();
    double acc = 0.0;
    for (int e = c_tri_ptr[t]; e < c_tri_ptr[t + 1]; ++e) acc = tri_term(acc, c_tri_val[e], b[(int)c_tri_col[e]]);
    coef[(size_t)pair * 64 + t] = acc;
  }
}

// The node table of the second layout (srt_interp_nodes.hpp): nodes[node][species][8] = the eight constraint families of
// build_coeffs_kernel, scaled by the spacings with its left-to-right products, so the stored bits are the bits it forms.
// One thread per (node, species); the arrays and the table are indexed alike (gidx).
__global__ void build_nodes_kernel(ArrPtrs arrs, double dx, double dy, double dz, double *nodes, size_t n) {
  for (size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x; id < n; id += (size_t)gridDim.x * blockDim.x) {
    double v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = arrs.a[q][id];
    v[1] = v[1] * dx;
    v[2] = v[2] * dy;
    v[3] = v[3] * dz;
    v[4] = v[4] * dx * dy;
    v[5] = v[5] * dx * dz;
    v[6] = v[6] * dy * dz;
    v[7] = v[7] * dx * dy * dz;
#pragma unroll
    for (int q = 0; q < 8; ++q) nodes[id * 8 + q] = v[q];
  }
}

// ---- the two layouts of modelnum 3: sizes, and the choice SRT_INTERP_AUTO makes (pure host code) ----
static bool layout_known(int layout) { return layout == SRT_INTERP_EXPANDED || layout == SRT_INTERP_NODES || layout == SRT_INTERP_AUTO; }
static int layout_unknown(const char *who, int layout) {
  return srt_set_error(SRT_EINVAL, "%s: unknown layout %d (SRT_INTERP_EXPANDED 0, SRT_INTERP_NODES 1, SRT_INTERP_AUTO 2)", who, layout);
}
extern "C" int srt_interp_layout_bytes(int nspec, int nx, int ny, int nz, int layout, int64_t *table, int64_t *peak) {
  if (layout != SRT_INTERP_EXPANDED && layout != SRT_INTERP_NODES)
    return srt_set_error(SRT_EINVAL, "srt_interp_layout_bytes: layout %d is neither SRT_INTERP_EXPANDED nor SRT_INTERP_NODES", layout);
  if (nspec < 1 || nspec > SRT_MAXSPEC || nx < 2 || ny < 2 || nz < 2) return srt_set_error(SRT_EINVAL, "srt_interp_layout_bytes: bad grid");
  const int64_t n = (int64_t)nx * ny * nz * nspec; // values per grid array
  const int64_t t = layout == SRT_INTERP_EXPANDED ? (int64_t)(nx + 1) * (ny + 1) * (nz + 1) * nspec * 64 * 8 : n * 64;
  if (table) *table = t;
  if (peak) *peak = t + 8 * n * 8; // creation holds the eight grid arrays and the table at the same time
  return SRT_OK;
}
extern "C" int srt_interp_layout_choose(int nspec, int nx, int ny, int nz, int64_t free_bytes) {
  int64_t t, pk;
  int rc = srt_interp_layout_bytes(nspec, nx, ny, nz, SRT_INTERP_EXPANDED, &t, &pk);
  if (rc) return rc;
  if (pk <= free_bytes) return SRT_INTERP_EXPANDED;
  if ((rc = srt_interp_layout_bytes(nspec, nx, ny, nz, SRT_INTERP_NODES, &t, &pk))) return rc;
  if (pk <= free_bytes) return SRT_INTERP_NODES;
  return srt_set_error(SRT_ENOMEM, "interp model %dx%dx%d, %d species: the node table needs %lld bytes at creation, %lld are free", nx,
                       ny, nz, nspec, (long long)pk, (long long)free_bytes);
}
// SRT_INTERP_AUTO -> the layout that fits the current device's free memory (or an error); the others pass through
static int resolve_layout(int nspec, int nx, int ny, int nz, int layout, int *out) {
  *out = layout;
  if (layout != SRT_INTERP_AUTO) return SRT_OK;
  size_t fr = 0, tot = 0;
  HIP_OK(hipMemGetInfo(&fr, &tot));
  const int c = srt_interp_layout_choose(nspec, nx, ny, nz, (int64_t)fr);
  if (c < 0) return c;
  *out = c;
  return SRT_OK;
}

// FD derivatives (unless given) + coefficient expansion (or the node table: `layout`, SRT_INTERP_EXPANDED or _NODES) + model
// object, from the 8 arrays already on the device.  Only the table's kernel and what the model struct holds branch by layout:
// the axes, the owner (ModelPtr) and the tail (model_hand_over, srt_api_model.hpp) are common.
// arr[0] = F; arr[1..7] = derivative blocks (contents ignored when !have_derivs).  The arrays are freed here, before the model
// is made.
static int interp_from_device_arrays(int nspec, int nx, int ny, int nz, const double bounds[6], const double *qs,
                                     const double *ms, DevBuf<double> (&arr)[8], bool have_derivs, int yearday, int msec,
                                     srt_model **out, int layout = SRT_INTERP_EXPANDED) {
  const size_t nnode = (size_t)nx * ny * nz, n = nnode * nspec;
  const size_t ncell = (size_t)(nx + 1) * (ny + 1) * (nz + 1);
  GridDims g{nspec, nx, ny, nz};
  // interp_dens_model_adapter.f95:87-89
  double dx = (bounds[1] - bounds[0]) / (nx - 1.0);
  double dy = (bounds[3] - bounds[2]) / (ny - 1.0);
  double dz = (bounds[5] - bounds[4]) / (nz - 1.0);
  DevBuf<double> coef;
  hipError_t e = hipSuccess;
  if (!have_derivs) {
    for (int a = 1; a < 8 && e == hipSuccess; ++a) e = hipMemset(arr[a].p, 0, n * sizeof(double));
    const int blocks = stride_blocks(n);
    auto fd = [&](int src, int dst, int axis, double h) {
      hipLaunchKernelGGL(fd_axis_kernel, dim3(blocks), dim3(256), 0, 0, g, (const double *)arr[src].p, arr[dst].p, axis, h);
    };
    // order and guards of libtricubic.f95:736-790
    if (nx > 2) fd(0, 1, 0, dx);
    if (ny > 2) fd(0, 2, 1, dy);
    if (nz > 2) fd(0, 3, 2, dz);
    if (nx > 2 && ny > 2) fd(2, 4, 0, dx);
    if (nx > 2 && nz > 2) fd(3, 5, 0, dx);
    if (ny > 2 && nz > 2) fd(3, 6, 1, dy);
    if (nx > 2 && ny > 2 && nz > 2) fd(6, 7, 0, dx);
  }
  const bool as_nodes = layout == SRT_INTERP_NODES;
  if (e == hipSuccess) e = coef.alloc(as_nodes ? n * 8 : ncell * nspec * 64);
  if (e != hipSuccess)
    return srt_set_error(e == hipErrorOutOfMemory ? SRT_ENOMEM : SRT_EDEVICE, "interp model setup: %s", hipGetErrorString(e));
  ArrPtrs ap;
  for (int a = 0; a < 8; ++a) ap.a[a] = arr[a].p;
  if (as_nodes) {
    hipLaunchKernelGGL(build_nodes_kernel, dim3(stride_blocks(n)), dim3(256), 0, 0, ap, dx, dy, dz, coef.p, n);
  } else {
    (void)hipMemcpyToSymbol(HIP_SYMBOL(c_tri_ptr), TRI_PTR, sizeof TRI_PTR);
    (void)hipMemcpyToSymbol(HIP_SYMBOL(c_tri_col), TRI_COL, sizeof TRI_COL);
    (void)hipMemcpyToSymbol(HIP_SYMBOL(c_tri_val), TRI_VAL, sizeof TRI_VAL);
    long long npairs = (long long)ncell * nspec;
    int blocks = (int)(npairs < 262144 ? npairs : 262144);
    hipLaunchKernelGGL(build_coeffs_kernel, dim3(blocks), dim3(64), 0, 0, g, ap, dx, dy, dz, coef.p, npairs);
  }
  e = hipDeviceSynchronize();
  for (auto &b : arr) b.release();
  if (e != hipSuccess) return srt_set_error(SRT_EDEVICE, "%s build failed: %s", as_nodes ? "node table" : "coefficient", hipGetErrorString(e));
  // the model object: the table, and the axes in InterpModel's form on both layouts (the launch-cell ray order,
  // srt_trace_batch_device, takes its keys from them)
  ModelPtr m = new_model(as_nodes ? KIND_INTERP_NODES : KIND_INTERP, nspec);
  m->d_coef.swap(coef);
  m->device_bytes = (int64_t)(m->d_coef.cap * sizeof(double));
  InterpModel &im = m->as<InterpModel>();
  im.coef = as_nodes ? nullptr : m->d_coef.p;
  im.nspec = nspec;
  im.ax = Axis{bounds[0], dx, 1.0 / dx, nx};
  im.ay = Axis{bounds[2], dy, 1.0 / dy, ny};
  im.az = Axis{bounds[4], dz, 1.0 / dz, nz};
  if (as_nodes) {
    InterpNodesModel &nm = m->as<InterpNodesModel>();
    nm.nodes = m->d_coef.p;
    nm.nspec = nspec;
    nm.ax = im.ax, nm.ay = im.ay, nm.az = im.az;
  }
  fill_common(m->cm, nspec, qs, ms, yearday, msec);
  return model_hand_over(m, out, [&](srt_model *p) -> int { // (the node-table layout keeps the axes on the device as well)
    if (!as_nodes) return SRT_OK;
    if (p->d_axes.alloc(1) != hipSuccess) return srt_set_error(SRT_ENOMEM, "hipMalloc failed");
    if (hipMemcpy(p->d_axes.p, &im, sizeof im, hipMemcpyHostToDevice) != hipSuccess) return srt_set_error(SRT_EDEVICE, "upload of the axes failed");
    return SRT_OK;
  });
}

static int alloc_grid_arrays(size_t n, DevBuf<double> (&arr)[8]) {
  for (auto &b : arr)
    if (b.alloc(n) != hipSuccess)
      return srt_set_error(SRT_ENOMEM, "hipMalloc of grid arrays failed (%zu bytes each)", n * sizeof(double));
  return SRT_OK;
}

static int create_interp(int nspec, int nx, int ny, int nz, const double bounds[6], const double *qs, const double *ms,
                         const double *F, const double *const *derivs, int yearday, int msec, int layout, srt_model **out) {
  if (!bounds || !qs || !ms || !F || !out) return srt_set_error(SRT_EINVAL, "null argument");
  if (nspec < 1 || nspec > SRT_MAXSPEC)
    return srt_set_error(SRT_EINVAL, "nspec=%d unsupported (1..%d species: SRT_MAXSPEC, include/srt.h)", nspec, SRT_MAXSPEC);
  if (nx < 2 || ny < 2 || nz < 2) return srt_set_error(SRT_EINVAL, "grid must have >= 2 nodes per axis");
  DeviceScope srt_iscope_;
  int rc = srt_iscope_.enter_default();
  if (rc) return rc;
  const size_t n = (size_t)nx * ny * nz * nspec;
  if ((size_t)(nx + 1) * (ny + 1) * (nz + 1) >= (size_t)1 << 31) return srt_set_error(SRT_EINVAL, "grid too large");
  if ((rc = resolve_layout(nspec, nx, ny, nz, layout, &layout))) return rc;
  DevBuf<double> arr[8];
  rc = alloc_grid_arrays(n, arr);
  if (rc) return rc;
  hipError_t e = hipMemcpy(arr[0].p, F, n * sizeof(double), hipMemcpyHostToDevice);
  if (derivs)
    for (int a = 1; a < 8 && e == hipSuccess; ++a)
      e = hipMemcpy(arr[a].p, derivs[a - 1], n * sizeof(double), hipMemcpyHostToDevice);
  if (e != hipSuccess) return srt_set_error(SRT_EDEVICE, "grid upload: %s", hipGetErrorString(e));
  return interp_from_device_arrays(nspec, nx, ny, nz, bounds, qs, ms, arr, derivs != nullptr, yearday, msec, out, layout);
}
extern "C" int srt_model_create_interp(int nspec, int nx, int ny, int nz, const double bounds[6],
                                       const double *qs, const double *ms, const double *F,
                                       const double *const *derivs, int yearday, int msec, srt_model **out) {
  return create_interp(nspec, nx, ny, nz, bounds, qs, ms, F, derivs, yearday, msec, SRT_INTERP_EXPANDED, out);
}
extern "C" int srt_model_create_interp_layout(int nspec, int nx, int ny, int nz, const double bounds[6], const double *qs,
                                              const double *ms, const double *F, const double *const *derivs, int yearday,
                                              int msec, int layout, srt_model **out) {
  if (!layout_known(layout)) return layout_unknown("srt_model_create_interp_layout", layout);
  return create_interp(nspec, nx, ny, nz, bounds, qs, ms, F, derivs, yearday, msec, layout, out);
}

// ---- the step before the path: sample a model on a regular grid, in log space, on the device ----
// gcpm_dens_model_buildgrid.f95:160-300 with any in-scope model in place of GCPM: node coordinates
// (/ (ind) /)*del + min (:163-179), f = log(Ns) (:212-214), and, for compder = 1, the seven explicit
// finite-difference blocks with d = 1e-3*|pos| (:197-201, :219-296) in the reference's own order of operations.
struct SampleArgs {
  double min[3], del[3];
  double *a[8];
  long long nnode;
  int compder;
};
template <class M, bool USE_LDS>
__global__ __launch_bounds__(64) void sample_grid_kernel(const M *__restrict__ mp, GridDims g, SampleArgs A) {
  const M &m = *mp;
  __shared__ __attribute__((aligned(16))) double tile[USE_LDS ? TILE_DOUBLES : 2];
  const long long id = (long long)blockIdx.x * WAVE + threadIdx.x;
  const bool live = id < A.nnode;
  const long long node = live ? id : A.nnode - 1; // every lane takes part in the (cooperative) lookups
  const int i = (int)(node % g.nx), j = (int)((node / g.nx) % g.ny), k = (int)(node / ((long long)g.nx * g.ny));
  double pos[3];
  {
#pragma clang fp contract(off)
    double px = (double)i * A.del[0], py = (double)j * A.del[1], pz = (double)k * A.del[2];
    pos[0] = px + A.min[0];
    pos[1] = py + A.min[1];
    pos[2] = pz + A.min[2];
  }
  double d = 1.0e-3 * sqrt(pos[0] * pos[0] + pos[1] * pos[1] + pos[2] * pos[2]);
  if (d == 0.0) d = 1.0e-3;
  auto lnN = [&](double sx, double sy, double sz, double (&L)[4]) { // log(Ns) at (pos + sx*dx) + sy*dy) + sz*dz
    double p[1][3] = {{(pos[0] + sx * d) + 0.0, (pos[1] + 0.0) + sy * d, ((pos[2] + 0.0) + 0.0) + sz * d}};
    double Ns[1][4];
    m.template density<1>(p, Ns, tile);
#pragma unroll
    for (int s = 0; s < 4; ++s) L[s] = log(Ns[0][s]);
  };
  auto put = [&](int blk, const double (&v)[4]) {
    if (live)
      for (int s = 0; s < g.nspec; ++s) A.a[blk][(size_t)node * g.nspec + s] = v[s];
  };
  double f[4], t[4], u[4];
  lnN(0, 0, 0, f);
  put(0, f);
  if (!A.compder) return;
  // first derivatives: tmp = log(N+) ; tmp = tmp - log(N-) ; tmp = tmp/d/2
  for (int ax = 0; ax < 3; ++ax) {
    lnN(ax == 0, ax == 1, ax == 2, t);
    lnN(-(ax == 0), -(ax == 1), -(ax == 2), u);
#pragma unroll
    for (int s = 0; s < 4; ++s) t[s] = (t[s] - u[s]) / d / 2.0;
    put(1 + ax, t);
  }
  // mixed second derivatives: (+,+) - (-,+) - (+,-) + (-,-) ; /d/d/4        pairs (x,y) (x,z) (y,z)
  for (int pr = 0; pr < 3; ++pr) {
    const int a0 = pr == 2 ? 1 : 0, a1 = pr == 0 ? 1 : 2;
    double sg[3];
    auto at = [&](double s0, double s1, double (&L)[4]) {
      sg[0] = sg[1] = sg[2] = 0.0;
      sg[a0] = s0;
      sg[a1] = s1;
      lnN(sg[0], sg[1], sg[2], L);
    };
    at(1, 1, t);
    at(-1, 1, u);
#pragma unroll
    for (int s = 0; s < 4; ++s) t[s] = t[s] - u[s];
    at(1, -1, u);
#pragma unroll
    for (int s = 0; s < 4; ++s) t[s] = t[s] - u[s];
    at(-1, -1, u);
#pragma unroll
    for (int s = 0; s < 4; ++s) t[s] = (t[s] + u[s]) / d / d / 4.0;
    put(4 + pr, t);
  }
  // third derivative: +++ -(-++) -(+-+) +(--+) -(++-) +(-+-) +(+--) -(---) ; /d/d/d/8
  {
    const double sx[8] = {1, -1, 1, -1, 1, -1, 1, -1}, sy[8] = {1, 1, -1, -1, 1, 1, -1, -1}, sz[8] = {1, 1, 1, 1, -1, -1, -1, -1};
    const double sign[8] = {1, -1, -1, 1, -1, 1, 1, -1};
    lnN(sx[0], sy[0], sz[0], t);
    for (int q = 1; q < 8; ++q) {
      lnN(sx[q], sy[q], sz[q], u);
#pragma unroll
      for (int s = 0; s < 4; ++s) t[s] = sign[q] > 0 ? t[s] + u[s] : t[s] - u[s];
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) t[s] = t[s] / d / d / d / 8.0;
    put(7, t);
  }
}

// fills arr[0] (and arr[1..7] when compder) on the device
static int sample_model_on_grid(srt_model *src, int compder, int nx, int ny, int nz, const double bounds[6],
                                DevBuf<double> (&arr)[8]) {
  GridDims g{src->nspec, nx, ny, nz};
  SampleArgs A;
  // gcpm_dens_model_buildgrid.f95:161-163
  A.del[0] = (bounds[1] - bounds[0]) / (nx - 1.0);
  A.del[1] = (bounds[3] - bounds[2]) / (ny - 1.0);
  A.del[2] = (bounds[5] - bounds[4]) / (nz - 1.0);
  A.min[0] = bounds[0];
  A.min[1] = bounds[2];
  A.min[2] = bounds[4];
  for (int a = 0; a < 8; ++a) A.a[a] = arr[a].p;
  A.nnode = (long long)nx * ny * nz;
  A.compder = compder;
  const int rc = with_model(src, [&](auto tag) -> int {
    using T = decltype(tag);
    launch_wave_blocks(sample_grid_kernel<typename T::Model, T::lds>, A.nnode, 0, src->on_device<typename T::Model>(), g, A);
    return SRT_OK;
  });
  if (rc) return rc;
  hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) return srt_set_error(SRT_EDEVICE, "grid sampling failed: %s", hipGetErrorString(e));
  return SRT_OK;
}

static int check_grid_request(srt_model *src, int nx, int ny, int nz, const double bounds[6]) {
  if (!src || !bounds) return srt_set_error(SRT_EINVAL, "null argument");
  if (nx < 2 || ny < 2 || nz < 2) return srt_set_error(SRT_EINVAL, "grid must have >= 2 nodes per axis");
  if ((size_t)(nx + 1) * (ny + 1) * (nz + 1) >= (size_t)1 << 31) return srt_set_error(SRT_EINVAL, "grid too large");
  if (!(bounds[1] > bounds[0]) || !(bounds[3] > bounds[2]) || !(bounds[5] > bounds[4])) return srt_set_error(SRT_EINVAL, "empty bounds");
  return SRT_OK;
}

extern "C" int srt_build_grid(srt_model *src, int compder, int nx, int ny, int nz, const double bounds[6], double *F,
                              double *derivs) {
  int rc = check_grid_request(src, nx, ny, nz, bounds);
  if (rc) return rc;
  SRT_MODEL_SCOPE;
  if ((rc = ensure_model(src))) return rc;
  if (!F || (compder && !derivs)) return srt_set_error(SRT_EINVAL, "null output");
  const size_t n = (size_t)nx * ny * nz * src->nspec;
  DevBuf<double> arr[8];
  if ((rc = alloc_grid_arrays(n, arr)) || (rc = sample_model_on_grid(src, compder ? 1 : 0, nx, ny, nz, bounds, arr))) return rc;
  hipError_t e = hipMemcpy(F, arr[0].p, n * sizeof(double), hipMemcpyDeviceToHost);
  if (compder)
    for (int a = 1; a < 8 && e == hipSuccess; ++a)
      e = hipMemcpy(derivs + (size_t)(a - 1) * n, arr[a].p, n * sizeof(double), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return srt_set_error(SRT_EDEVICE, "grid download: %s", hipGetErrorString(e));
  return SRT_OK;
}

// ---- dumpmodel.f95: funcPlasmaParams of any model on a regular grid, in SM or MAG coordinates ----
// Three launches on one stream: the nodes' coordinates (dumpmodel.f95:219-237, and SM_TO_MAG_D for mag_coords = 1,
// :1140-1143), then the UNCHANGED params_kernel on them, then the 19 values of a node packed into the file's 4 nspec + 3.  The
// dump of a node is therefore what srt_plasma_params gives at the node's coordinates, bit for bit, by construction: the
// lookups are the same instruction stream on the same inputs (a kernel that formed the coordinates around the lookup would
// leave the compiler free to fuse other products, HISTORY.md section 22).
struct DumpArgs {
  double min[3], del[3];
  int n[3];
  int mag;
  xform::Chain chain;
};
// x[count][3] = the coordinates of nodes first .. first + count - 1 (linear index = the file's order: x fastest, then y, z)
__global__ __launch_bounds__(256) void dump_points_kernel(DumpArgs A, long long first, long long count, double *__restrict__ x) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count) return;
  const long long node = first + t;
  const int idx[3] = {(int)(node % A.n[0]), (int)((node / A.n[0]) % A.n[1]), (int)(node / ((long long)A.n[0] * A.n[1]))};
  double pos[3];
  {
#pragma clang fp contract(off)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double p = (double)idx[c] * A.del[c]; // (/ (ind) /)*del + min: a product, then a sum
      pos[c] = A.n[c] == 1 ? A.min[c] : p + A.min[c]; // one node: x = (/ minx /), del (a quotient by zero) is never read
    }
  }
  double q[3] = {pos[0], pos[1], pos[2]};
  if (A.mag) xform::apply(A.chain, pos, q);
  x[3 * t] = q[0];
  x[3 * t + 1] = q[1];
  x[3 * t + 2] = q[2];
}
// f[count][4 nspec + 3] = (qs, Ns, ms, nus, B0) from params_kernel's p[count][19] = qs(4) Ns(4) ms(4) nus(4) B0(3): the unused
// species slot of a three-species model is dropped.  One thread per output value: a block writes one contiguous run.
__global__ __launch_bounds__(256) void dump_pack_kernel(long long count, int nspec, const double *__restrict__ p, double *__restrict__ f) {
  const int per = 4 * nspec + 3;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count * per) return;
  const long long node = t / per;
  const int c = (int)(t - node * per);
  const int src = c < 4 * nspec ? 4 * (c / nspec) + c % nspec : 16 + (c - 4 * nspec);
  f[t] = p[19 * node + src];
}

extern "C" int srt_dump_model(srt_model *m, int nx, int ny, int nz, const double bounds[6], int mag_coords, double *f) {
  // every refusal by name comes before the device is touched
  if (!bounds || !f) return srt_set_error(SRT_EINVAL, "srt_dump_model: null argument");
  if (nx < 1 || ny < 1 || nz < 1) return srt_set_error(SRT_EINVAL, "srt_dump_model: nx, ny, nz = %d, %d, %d: every axis needs at least 1 node", nx, ny, nz);
  const int n3[3] = {nx, ny, nz};
  for (int c = 0; c < 3; ++c)
    if (n3[c] > 1 && !(bounds[2 * c + 1] > bounds[2 * c]))
      return srt_set_error(SRT_EINVAL, "srt_dump_model: empty bounds on the %c axis (%d nodes need max > min)", "xyz"[c], n3[c]);
  const long long nxy = (long long)nx * ny, nnode = nxy <= 2147483647ll ? nxy * nz : -1; // (either product fits 63 bits)
  if (nnode < 0 || nnode > 2147483647ll)
    return srt_set_error(SRT_EINVAL, "srt_dump_model: %d x %d x %d is more than 2^31 - 1 nodes", nx, ny, nz);
  if (mag_coords != 0 && mag_coords != 1) return srt_set_error(SRT_EINVAL, "srt_dump_model: mag_coords = %d is neither 0 (SM) nor 1 (MAG)", mag_coords);
  if (!m) return srt_set_error(SRT_EINVAL, "srt_dump_model: null model");
  SRT_MODEL_SCOPE;
  int rc = ensure_model(m);
  if (rc) return rc;
  DumpArgs A;
  memset(&A, 0, sizeof A);
  for (int c = 0; c < 3; ++c) {
    A.n[c] = n3[c];
    A.min[c] = bounds[2 * c];
    A.del[c] = n3[c] > 1 ? (bounds[2 * c + 1] - bounds[2 * c]) / (n3[c] - 1.0) : 0.0; // dumpmodel.f95:220-222
  }
  A.mag = mag_coords;
  if (mag_coords) A.chain = xform::chain(m->cm.fld.yearday, m->cm.fld.msec, false);
  const int per = 4 * m->nspec + 3;
  // the output is whole on the device; the coordinates and params_kernel's 19 values per node exist for one piece at a time
  const long long PIECE = 1ll << 20;
  const long long piece = nnode < PIECE ? nnode : PIECE;
  DevBuf<double> dx, dp19, df;
  if (df.alloc((size_t)nnode * per) != hipSuccess || dx.alloc((size_t)3 * piece) != hipSuccess || dp19.alloc((size_t)19 * piece) != hipSuccess) {
    (void)hipGetLastError();
    return srt_set_error(SRT_ENOMEM, "srt_dump_model: %lld nodes of %d values do not fit on the device", nnode, per);
  }
  srt_model::LaunchTimes &lt = m->hist[m->next_hist];
  HIP_OK(hipEventRecord(lt.ev0, 0));
  for (long long first = 0; first < nnode; first += piece) {
    const long long count = nnode - first < piece ? nnode - first : piece;
    hipLaunchKernelGGL(dump_points_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, 0, A, first, count, dx.p);
    rc = with_model(m, [&](auto tag) -> int {
      using T = decltype(tag);
      launch_wave_blocks(params_kernel<typename T::Model, T::lds>, count, 0, m->on_device<typename T::Model>(), m->d_common.p, count,
                         (const double *)dx.p, dp19.p);
      return SRT_OK;
    });
    if (rc) return rc;
    hipLaunchKernelGGL(dump_pack_kernel, dim3((unsigned)((count * per + 255) / 256)), dim3(256), 0, 0, count, m->nspec,
                       (const double *)dp19.p, df.p + (size_t)first * per);
  }
  HIP_OK(hipGetLastError());
  HIP_OK(hipEventRecord(lt.ev1, 0));
  lt.used = true;
  m->last_hist = m->next_hist;
  m->next_hist = (m->next_hist + 1) % srt_model::NHIST;
  HIP_OK(hipMemcpy(f, df.p, (size_t)nnode * per * sizeof(double), hipMemcpyDeviceToHost));
  return SRT_OK;
}

static int create_interp_from_model(srt_model *src, int compder, int nx, int ny, int nz, const double bounds[6], int yearday,
                                    int msec, int layout, srt_model **out) {
  int rc = check_grid_request(src, nx, ny, nz, bounds);
  if (rc) return rc;
  if (!out) return srt_set_error(SRT_EINVAL, "null argument");
  SRT_MODEL_SCOPE; // the new model is built beside its source, on the source's device
  if ((rc = ensure_model(src))) return rc;
  const size_t n = (size_t)nx * ny * nz * src->nspec;
  if ((rc = resolve_layout(src->nspec, nx, ny, nz, layout, &layout))) return rc;
  DevBuf<double> arr[8];
  if ((rc = alloc_grid_arrays(n, arr)) || (rc = sample_model_on_grid(src, compder ? 1 : 0, nx, ny, nz, bounds, arr))) return rc;
  return interp_from_device_arrays(src->nspec, nx, ny, nz, bounds, src->cm.sp.q, src->cm.sp.m, arr, compder != 0,
                                   yearday, msec, out, layout);
}
extern "C" int srt_model_create_interp_from_model(srt_model *src, int compder, int nx, int ny, int nz,
                                                  const double bounds[6], int yearday, int msec, srt_model **out) {
  return create_interp_from_model(src, compder, nx, ny, nz, bounds, yearday, msec, SRT_INTERP_EXPANDED, out);
}
extern "C" int srt_model_create_interp_from_model_layout(srt_model *src, int compder, int nx, int ny, int nz,
                                                         const double bounds[6], int yearday, int msec, int layout,
                                                         srt_model **out) {
  if (!layout_known(layout)) return layout_unknown("srt_model_create_interp_from_model_layout", layout);
  return create_interp_from_model(src, compder, nx, ny, nz, bounds, yearday, msec, layout, out);
}

static int create_interp_file(const char *gridfile, int yearday, int msec, int layout, srt_model **out) {
  if (!gridfile || !out) return srt_set_error(SRT_EINVAL, "null argument");
  srt_host::GridFile gf;
  std::string err;
  if (!srt_host::read_grid_file(gridfile, gf, err)) return srt_set_error(SRT_EIO, "%s: %s", gridfile, err.c_str());
  const double *dptr[7];
  for (int a = 0; a < 7; ++a) dptr[a] = gf.have_derivs ? gf.derivs[a].data() : nullptr;
  return create_interp(gf.nspec, gf.nx, gf.ny, gf.nz, gf.bounds, gf.qs, gf.ms, gf.F.data(), gf.have_derivs ? dptr : nullptr, yearday,
                       msec, layout, out);
}
extern "C" int srt_model_create_interp_file(const char *gridfile, int yearday, int msec, srt_model **out) {
  return create_interp_file(gridfile, yearday, msec, SRT_INTERP_EXPANDED, out);
}
extern "C" int srt_model_create_interp_file_layout(const char *gridfile, int yearday, int msec, int layout, srt_model **out) {
  if (!layout_known(layout)) return layout_unknown("srt_model_create_interp_file_layout", layout);
  return create_interp_file(gridfile, yearday, msec, layout, out);
}
