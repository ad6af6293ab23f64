// Host build of the node-table lookup of modelnum 3 -- stanford_raytracer_amd/csrc/srt_interp_nodes.hpp's gather with its clamp
// and sticky flags, its 64 unrolled coefficient rows and InterpModel::eval, the very source the device compiles -- for the CPU
// tests (tests/test_interp_nodes_host.py), checked against the oracle.  Compiled as HIP for the host alone.  What is restated
// here because it is device-only or lives in srt_api_grid.hpp: the finite-difference passes (fd_axis_kernel and their order), the
// fill of the node table (build_nodes_kernel) and the cell search (Axis::locate: the count of nodes <= x and the local
// coordinate), each plainly.
//
// As a program: interp_nodes_host < input, where input is "nspec nx ny nz have_derivs npoints", six bounds, the values of F (and
// of the seven derivative blocks) in the grid file's order, then the points; prints ln N_s of every point, one line each.
#include <cstdio>
#include <vector>

#include "../../stanford_raytracer_amd/csrc/srt_interp_nodes.hpp"

namespace {

struct Dims {
  int nspec, nx, ny, nz;
};
size_t gidx(const Dims &g, int s, int i, int j, int k) { return (((size_t)k * g.ny + j) * g.nx + i) * g.nspec + s; }

// tricubic_compute_finite_difference_derivatives, one axis (libtricubic.f95:736-790)
void fd_axis(const Dims &g, const double *src, double *dst, int axis, double h) {
  const int n[3] = {g.nx, g.ny, g.nz};
  for (int k = 0; k < g.nz; ++k)
    for (int j = 0; j < g.ny; ++j)
      for (int i = 0; i < g.nx; ++i)
        for (int s = 0; s < g.nspec; ++s) {
          int lo[3] = {i, j, k}, hi[3] = {i, j, k};
          const int a = lo[axis], na = n[axis];
          double v;
          if (a == 0) {
            hi[axis] = 1;
            v = (src[gidx(g, s, hi[0], hi[1], hi[2])] - src[gidx(g, s, lo[0], lo[1], lo[2])]) / h;
          } else if (a == na - 1) {
            lo[axis] = na - 2;
            v = (src[gidx(g, s, hi[0], hi[1], hi[2])] - src[gidx(g, s, lo[0], lo[1], lo[2])]) / h;
          } else {
            lo[axis] = a - 1, hi[axis] = a + 1;
            v = (src[gidx(g, s, hi[0], hi[1], hi[2])] - src[gidx(g, s, lo[0], lo[1], lo[2])]) / 2.0 / h;
          }
          dst[gidx(g, s, i, j, k)] = v;
        }
}

// number of nodes <= x (a NaN: 0) and the local coordinate, with the nodes real(i)*del + min rounded product first
int locate(double x, double mn, double del, int n, double &xl) {
  auto node = [&](int i) {
    volatile double prod = (double)i * del; // (rounded on its own: not fused into the sum)
    return prod + mn;
  };
  int g = 0;
  while (g < n && node(g) <= x) ++g;
  xl = (g >= 1 && g < n) ? (x - node(g - 1)) / del : 0.0;
  return g;
}

} // namespace

// F[nz][ny][nx][nspec]; derivs = NULL (finite differences) or the seven blocks concatenated; x[n][3] -> lnN[n][4] (species
// the grid does not have: 0).  Returns 0.
extern "C" int inh_lnN(int nspec, int nx, int ny, int nz, const double *bounds, const double *F, const double *derivs, long n,
                       const double *x, double *lnN) {
  const Dims g{nspec, nx, ny, nz};
  const size_t nv = (size_t)nx * ny * nz * nspec;
  const double dx = (bounds[1] - bounds[0]) / (nx - 1.0), dy = (bounds[3] - bounds[2]) / (ny - 1.0),
               dz = (bounds[5] - bounds[4]) / (nz - 1.0);
  std::vector<std::vector<double>> arr(8, std::vector<double>(nv, 0.0));
  arr[0].assign(F, F + nv);
  if (derivs) {
    for (int a = 1; a < 8; ++a) arr[a].assign(derivs + (size_t)(a - 1) * nv, derivs + (size_t)a * nv);
  } else { // order and guards of libtricubic.f95:736-790
    auto fd = [&](int src, int dst, int axis, double h) { fd_axis(g, arr[src].data(), arr[dst].data(), axis, h); };
    if (nx > 2) fd(0, 1, 0, dx);
    if (ny > 2) fd(0, 2, 1, dy);
    if (nz > 2) fd(0, 3, 2, dz);
    if (nx > 2 && ny > 2) fd(2, 4, 0, dx);
    if (nx > 2 && nz > 2) fd(3, 5, 0, dx);
    if (ny > 2 && nz > 2) fd(3, 6, 1, dy);
    if (nx > 2 && ny > 2 && nz > 2) fd(6, 7, 0, dx);
  }
  // the node table: the eight families scaled with build_coeffs_kernel's left-to-right products
  std::vector<double> nodes(nv * 8);
  for (size_t id = 0; id < nv; ++id) {
    double *v = &nodes[id * 8];
    v[0] = arr[0][id];
    v[1] = arr[1][id] * dx;
    v[2] = arr[2][id] * dy;
    v[3] = arr[3][id] * dz;
    v[4] = arr[4][id] * dx * dy;
    v[5] = arr[5][id] * dx * dz;
    v[6] = arr[6][id] * dy * dz;
    v[7] = arr[7][id] * dx * dy * dz;
  }
  for (long p = 0; p < n; ++p) {
    double xl, yl, zl;
    const int ci = locate(x[3 * p], bounds[0], dx, nx, xl), cj = locate(x[3 * p + 1], bounds[2], dy, ny, yl),
              ck = locate(x[3 * p + 2], bounds[4], dz, nz, zl);
    for (int s = 0; s < 4; ++s)
      lnN[4 * p + s] = s < nspec ? srt::InterpNodesModel::lnN_in_cell(nodes.data(), nx, ny, nz, nspec, s, ci, cj, ck, xl, yl, zl) : 0.0;
  }
  return 0;
}

int main() {
  int nspec, nx, ny, nz, have, np;
  if (scanf("%d %d %d %d %d %d", &nspec, &nx, &ny, &nz, &have, &np) != 6 || nspec < 1 || nspec > 4 || nx < 2 || ny < 2 || nz < 2 || np < 0)
    return 2;
  double b[6];
  for (double &v : b)
    if (scanf("%lf", &v) != 1) return 2;
  const size_t nv = (size_t)nx * ny * nz * nspec;
  std::vector<double> F(nv), D(have ? 7 * nv : 0), x(3 * (size_t)np), out(4 * (size_t)np);
  for (double &v : F)
    if (scanf("%lf", &v) != 1) return 2;
  for (double &v : D)
    if (scanf("%lf", &v) != 1) return 2;
  for (double &v : x)
    if (scanf("%lf", &v) != 1) return 2;
  inh_lnN(nspec, nx, ny, nz, b, F.data(), have ? D.data() : nullptr, np, x.data(), out.data());
  for (int p = 0; p < np; ++p) printf("%.17g %.17g %.17g %.17g\n", out[4 * p], out[4 * p + 1], out[4 * p + 2], out[4 * p + 3]);
  return 0;
}
