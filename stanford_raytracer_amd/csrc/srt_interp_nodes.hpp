// srt_interp_nodes.hpp -- modelnum = 3 in its second layout: a node table, the 64 coefficients of a cell built at each lookup.
//
// HBM layout:  nodes[k][j][i][species][8]  doubles -- per (node, species) the eight constraint families of
// build_coeffs_kernel (srt_api_grid.hpp) in its order, already scaled by the spacings with that kernel's left-to-right products:
//     f, f_x dx, f_y dy, f_z dz, f_xy dx dy, f_xz dx dz, f_yz dy dz, f_xyz dx dy dz
// One record is 64 B, a node 256 B at four species, corners i and i + 1 are adjacent: a lookup reads four runs of 512 B.
// nx ny nz nspec 64 bytes: an eighth of the expanded table coef[cell][species][64] (InterpModel, srt_models.hpp).
//
// A lookup: the cell search of InterpModel (Axis::locate / in_cell), the cell's 8 corners x 8 families gathered per species
// with tricubic_interpolate_at's clamp of the corner indices and its sticky zeroing flags (libtricubic.f95:859-921; they
// matter only in cells 0 and n of an axis: the interior is a wave-uniform fast path), the 64 coefficient rows formed as
// build_coeffs_kernel forms them -- tri_term, the one expression both use, over the same entries in the same order, here
// fully unrolled with the 1000 matrix entries as compile-time constants -- and InterpModel's own evaluation (plane_stencil,
// plane_points, eval) and exponential on them.  The coefficients are the expanded table's bit for bit, and so is everything
// evaluated from them.
//
// Where things live: a lane's 64 gathered values of one species in registers (128), the coefficients a plane of 16 at a time
// (32 more); nothing in LDS, no ring, no residency: every lookup gathers again.
#pragma once
#include "srt_models.hpp"
#include "tricubic_matrix.h"

namespace srt {

// One term of a coefficient row: acc + val b, as one fused multiply-add.  build_coeffs_kernel and the node-table lookup both
// form their rows with this function.  The fma is spelled out so that it does not rest on the compiler's contraction: the build
// kernel's run-time loop always fuses, while in the unrolled rows a product that two rows share (the same val b[col]) may be
// computed once and added unfused, an ulp away from the table's coefficient.  (Operands in this order: the build kernel keeps
// the instruction stream it had with the contracted expression.)
SRT_HD __forceinline__ double tri_term(double acc, signed char val, double b) { return fma(b, (double)val, acc); }

// entries E .. END-1 of the sparse matrix, in order, onto acc
template <int E, int END>
SRT_HD __forceinline__ double tri_row_from(double acc, const double (&b)[64]) {
  if constexpr (E < END) {
    constexpr int col = TRI_COL[E];
    constexpr signed char val = TRI_VAL[E];
    return tri_row_from<E + 1, END>(tri_term(acc, val, b[col]), b);
  } else {
    return acc;
  }
}
// coefficient row T of tricubic_get_coeff: sum over TRI_PTR[T] .. TRI_PTR[T+1]-1 of val b[col], from 0.0, in that order
template <int T>
SRT_HD __forceinline__ double tri_row(const double (&b)[64]) {
  return tri_row_from<TRI_PTR[T], TRI_PTR[T + 1]>(0.0, b);
}

struct InterpNodesModel {
  const double *nodes; // [nz][ny][nx][nspec][8]
  Axis ax, ay, az;
  int nspec;

  // b[8 family + corner] of cell (ci, cj, ck) (each 0 .. n: the number of nodes <= the coordinate) and species s: the gather
  // of build_coeffs_kernel.  EDGE = false is for cells 1 .. n-1 of every axis, where no corner is clamped and no flag set.
  template <bool EDGE>
  SRT_HD __forceinline__ static void gather(const double *nodes, int nx, int ny, int nz, int nspec, int s, int ci, int cj, int ck,
                                            double (&b)[64]) {
#pragma unroll
    for (int l = 0; l < 8; ++l) {
      int it = ci + (l & 1), jt = cj + ((l >> 1) & 1), kt = ck + (l >> 2); // 1-based corner indices
      bool fi = false, fj = false, fk = false;
      if (EDGE) {
        it = it < 1 ? 1 : (it > nx ? nx : it);
        jt = jt < 1 ? 1 : (jt > ny ? ny : jt);
        kt = kt < 1 ? 1 : (kt > nz ? nz : kt);
        // flags are set by the first clamped corner and never reset inside the corner loop
        fi = (ci == 0) || (ci == nx && l >= 1);
        fj = (cj == 0) || (cj == ny && l >= 2);
        fk = (ck == 0) || (ck == nz && l >= 4);
      }
      const size_t node = ((size_t)(kt - 1) * (size_t)ny + (size_t)(jt - 1)) * (size_t)nx + (size_t)(it - 1);
      const d2_t *r = reinterpret_cast<const d2_t *>(nodes + (node * (size_t)nspec + (size_t)s) * 8);
      const d2_t r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3];
      b[l] = r0.x;
      b[8 + l] = fi ? 0.0 : r0.y;
      b[16 + l] = fj ? 0.0 : r1.x;
      b[24 + l] = fk ? 0.0 : r1.y;
      b[32 + l] = (fi || fj) ? 0.0 : r2.x;
      b[40 + l] = (fi || fk) ? 0.0 : r2.y;
      b[48 + l] = (fj || fk) ? 0.0 : r3.x;
      b[56 + l] = (fi || fj || fk) ? 0.0 : r3.y;
    }
  }
  // coefficients a(16 K .. 16 K + 15), as plane_stencil / plane_points take them: c[2j], c[2j+1] = a(0..3 + 4j + 16K)
  template <int K>
  SRT_HD __forceinline__ static void plane_coefs(const double (&b)[64], d2_t (&c)[8]) {
    c[0].x = tri_row<16 * K + 0>(b), c[0].y = tri_row<16 * K + 1>(b);
    c[1].x = tri_row<16 * K + 2>(b), c[1].y = tri_row<16 * K + 3>(b);
    c[2].x = tri_row<16 * K + 4>(b), c[2].y = tri_row<16 * K + 5>(b);
    c[3].x = tri_row<16 * K + 6>(b), c[3].y = tri_row<16 * K + 7>(b);
    c[4].x = tri_row<16 * K + 8>(b), c[4].y = tri_row<16 * K + 9>(b);
    c[5].x = tri_row<16 * K + 10>(b), c[5].y = tri_row<16 * K + 11>(b);
    c[6].x = tri_row<16 * K + 12>(b), c[6].y = tri_row<16 * K + 13>(b);
    c[7].x = tri_row<16 * K + 14>(b), c[7].y = tri_row<16 * K + 15>(b);
  }
  // ln N_s at local coordinates (xl, yl, zl) of cell (ci, cj, ck): gather, all 64 rows, InterpModel::eval
  SRT_HD __forceinline__ static double lnN_in_cell(const double *nodes, int nx, int ny, int nz, int nspec, int s, int ci, int cj,
                                                   int ck, double xl, double yl, double zl) {
    double b[64];
    gather<true>(nodes, nx, ny, nz, nspec, s, ci, cj, ck, b);
    d2_t a[32];
    {
      d2_t c[8];
      plane_coefs<0>(b, c);
#pragma unroll
      for (int q = 0; q < 8; ++q) a[q] = c[q];
      plane_coefs<1>(b, c);
#pragma unroll
      for (int q = 0; q < 8; ++q) a[8 + q] = c[q];
      plane_coefs<2>(b, c);
#pragma unroll
      for (int q = 0; q < 8; ++q) a[16 + q] = c[q];
      plane_coefs<3>(b, c);
#pragma unroll
      for (int q = 0; q < 8; ++q) a[24 + q] = c[q];
    }
    double x1[1] = {xl}, y1[1] = {yl}, z1[1] = {zl}, o1[1];
    InterpModel::eval<1>([&](int q) { return make_double2(a[q].x, a[q].y); }, x1, y1, z1, o1);
    return o1[0];
  }

  // one point on its own (lane-divergent): InterpModel::point_direct's two forms
  template <bool EXP>
  __device__ __forceinline__ void point_direct_body(double x, double y, double z, double out[4]) const {
    double xl, yl, zl;
    const int ci = ax.locate(x, xl), cj = ay.locate(y, yl), ck = az.locate(z, zl);
    double o[4] = {EXP ? 0.0 : out[0], EXP ? 0.0 : out[1], EXP ? 0.0 : out[2], EXP ? 0.0 : out[3]};
#pragma unroll 1
    for (int s = 0; s < nspec; ++s) {
      const double v = lnN_in_cell(nodes, ax.n, ay.n, az.n, nspec, s, ci, cj, ck, xl, yl, zl);
      const double e = EXP ? exp(v) : v; // Ns = exp(Ns) (interp_dens_model_adapter.f95:206)
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = (k == s) ? e : o[k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = o[k];
  }
  __device__ __noinline__ void point_direct(double x, double y, double z, double lnN[4]) const { point_direct_body<false>(x, y, z, lnN); }
  __device__ __noinline__ void point_direct_exp(double x, double y, double z, double N[4]) const { point_direct_body<true>(x, y, z, N); }

  // is any lane's cell one in which a corner is clamped (cells 0 and n of an axis)?  wave-uniform
  __device__ __forceinline__ static bool any_edge(const Axis &lx, const Axis &ly, const Axis &lz, int ci, int cj, int ck) {
    return __any((ci < 1) | (ci >= lx.n) | (cj < 1) | (cj >= ly.n) | (ck < 1) | (ck >= lz.n)) != 0;
  }

  // InterpModel::density_stencil on the node table: the coefficients of the centre's cell once per species, all 7 + NE points
  // that lie in that cell from them, a point in another cell through the per-point form.
  //
  // The empty asm with a memory clobber at the end is there for the kernels around the lookup, not for the lookup: the expanded
  // lookup has such clobbers (its LDS reads), so the caller's loads of the field constants are issued again behind it, and the
  // compiler orders the operands of n . B in dispersion_F (n[0] B[0] + n[1] B[1]: which product is fused into the sum) by where
  // those loads stand.  Without the clobber here the evalrhs site of the dipole trace kernels fused the other product in five
  // of those sums, dF/dk moved in the last bit, and fixed-step rows of the two layouts parted at rounding level from row 1 on
  // (HISTORY section 22).  With it every sum of two products has the same operand order in both layouts' kernels.
  template <int NE>
  __device__ __forceinline__ void density_stencil(const double c[3], const double d[3], const double *extra,
                                                  double (&Ns)[7 + NE][4], double *, bool = true) const {
    double X[3], Y[3], Z[3], E[3] = {0.0, 0.0, 0.0};
    const Axis lx = ax, ly = ay, lz = az;
    const double rx = fdiv_recip(lx.del), ry = fdiv_recip(ly.del), rz = fdiv_recip(lz.del);
    double xlo, ylo, zlo; // node(cell - 1) per axis
    const int ci = lx.locate(c[0], X[0], rx, xlo), cj = ly.locate(c[1], Y[0], ry, ylo), ck = lz.locate(c[2], Z[0], rz, zlo);
    // The offsets and the free point pass through an empty asm, as in InterpModel::density_stencil (which has them there for
    // its schedule): the caller forms an offset as a product (del |x|), and a sum c + d the compiler can see through could be
    // contracted with it into one fma, which rounds once where the expanded lookup's opaque sum rounds twice.
    double dd[3] = {d[0], d[1], d[2]}, ee[3] = {NE ? extra[0] : 0.0, NE ? extra[1] : 0.0, NE ? extra[2] : 0.0};
#pragma unroll
    for (int a_ = 0; a_ < 3; ++a_) {
      asm volatile("" : "+v"(dd[a_]));
      if (NE) asm volatile("" : "+v"(ee[a_]));
    }
    const double xhi = lx.node(ci), yhi = ly.node(cj), zhi = lz.node(ck);
    const bool same = lx.in_cell(c[0] + dd[0], ci, xlo, xhi, rx, X[1]) & lx.in_cell(c[0] - dd[0], ci, xlo, xhi, rx, X[2]) &
                      ly.in_cell(c[1] + dd[1], cj, ylo, yhi, ry, Y[1]) & ly.in_cell(c[1] - dd[1], cj, ylo, yhi, ry, Y[2]) &
                      lz.in_cell(c[2] + dd[2], ck, zlo, zhi, rz, Z[1]) & lz.in_cell(c[2] - dd[2], ck, zlo, zhi, rz, Z[2]);
    bool extra_same = true;
    if (NE) {
      extra_same = lx.in_cell(ee[0], ci, xlo, xhi, rx, E[0]) & ly.in_cell(ee[1], cj, ylo, yhi, ry, E[1]) &
                   lz.in_cell(ee[2], ck, zlo, zhi, rz, E[2]);
    }
    const bool edge = any_edge(lx, ly, lz, ci, cj, ck);
    const double *tab = nodes;
    const int ns = nspec;
    double acc[7 + NE][4];
#pragma unroll
    for (int i = 0; i < 7 + NE; ++i)
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[i][k] = 0.0;
    // species nspec-1 down to 0, each put in front and the others moved up one place: every species ends in its own place,
    // places beyond nspec keep their 0.0
#pragma unroll 1
    for (int s = ns - 1; s >= 0; --s) {
      double b[64];
      if (edge) gather<true>(tab, lx.n, ly.n, lz.n, ns, s, ci, cj, ck, b);
      else gather<false>(tab, lx.n, ly.n, lz.n, ns, s, ci, cj, ck, b);
      double vz[7 + NE];
      d2_t cf[8];
      plane_coefs<3>(b, cf);
      InterpModel::plane_stencil<NE, true>(cf, X, Y, Z, E, vz);
      plane_coefs<2>(b, cf);
      InterpModel::plane_stencil<NE>(cf, X, Y, Z, E, vz);
      plane_coefs<1>(b, cf);
      InterpModel::plane_stencil<NE>(cf, X, Y, Z, E, vz);
      plane_coefs<0>(b, cf);
      InterpModel::plane_stencil<NE>(cf, X, Y, Z, E, vz);
#pragma unroll
      for (int i = 0; i < 7 + NE; ++i) {
        const double e = exp(vz[i]); // Ns = exp(Ns) (:206)
        acc[i][3] = acc[i][2], acc[i][2] = acc[i][1], acc[i][1] = acc[i][0], acc[i][0] = e;
      }
    }
    // rare: a stencil point or the free point lies in another cell
    const unsigned away = (same ? 0u : 1u) | (extra_same ? 0u : 2u);
    if (__any(away != 0u)) {
      if (away & 1u) {
#pragma unroll
        for (int ax_ = 0; ax_ < 3; ++ax_)
#pragma unroll
          for (int sg = 0; sg < 2; ++sg) {
            double pt[3] = {c[0], c[1], c[2]}, t[4];
            pt[ax_] = sg ? c[ax_] - d[ax_] : c[ax_] + d[ax_];
            point_direct_exp(pt[0], pt[1], pt[2], t);
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[1 + 2 * ax_ + sg][k] = t[k];
          }
      }
      if (NE && (away & 2u)) {
        double t[4];
        point_direct_exp(extra[0], extra[1], extra[2], t);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[7 + NE - 1][k] = t[k];
      }
    }
    asm volatile("" ::: "memory"); // (see above the function)
#pragma unroll
    for (int i = 0; i < 7 + NE; ++i)
#pragma unroll
      for (int k = 0; k < 4; ++k) Ns[i][k] = acc[i][k];
  }

  // NP unrelated points (layered kernels, the builders): InterpModel::density on the node table
  template <int NP>
  __device__ __forceinline__ void density(const double (&p)[NP][3], double (&Ns)[NP][4], double *) const {
    // cell of point 0; the other points normally share it
    double xl[NP], yl[NP], zl[NP];
    const int ci = ax.locate(p[0][0], xl[0]);
    const int cj = ay.locate(p[0][1], yl[0]);
    const int ck = az.locate(p[0][2], zl[0]);
    unsigned strag = 0; // bit i: point i lies in another cell
#pragma unroll
    for (int i = 1; i < NP; ++i) {
      int c1 = ax.locate(p[i][0], xl[i]);
      int c2 = ay.locate(p[i][1], yl[i]);
      int c3 = az.locate(p[i][2], zl[i]);
      if (c1 != ci || c2 != cj || c3 != ck) strag |= 1u << i;
    }
    const bool edge = any_edge(ax, ay, az, ci, cj, ck);
    double acc[NP][4];
#pragma unroll
    for (int i = 0; i < NP; ++i)
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[i][k] = 0.0;
#pragma unroll 1
    for (int s = 0; s < nspec; ++s) {
      double b[64];
      if (edge) gather<true>(nodes, ax.n, ay.n, az.n, nspec, s, ci, cj, ck, b);
      else gather<false>(nodes, ax.n, ay.n, az.n, nspec, s, ci, cj, ck, b);
      double vz[NP];
#pragma unroll
      for (int i = 0; i < NP; ++i) vz[i] = 0.0;
      d2_t cf[8];
      plane_coefs<3>(b, cf);
      InterpModel::plane_points<NP>(cf, xl, yl, zl, vz);
      plane_coefs<2>(b, cf);
      InterpModel::plane_points<NP>(cf, xl, yl, zl, vz);
      plane_coefs<1>(b, cf);
      InterpModel::plane_points<NP>(cf, xl, yl, zl, vz);
      plane_coefs<0>(b, cf);
      InterpModel::plane_points<NP>(cf, xl, yl, zl, vz);
#pragma unroll
      for (int i = 0; i < NP; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[i][k] = (k == s) ? vz[i] : acc[i][k];
    }
    if (__any(strag != 0)) {
#pragma unroll
      for (int i = 1; i < NP; ++i)
        if (strag & (1u << i)) {
          double t[4] = {0.0, 0.0, 0.0, 0.0};
          point_direct(p[i][0], p[i][1], p[i][2], t);
#pragma unroll
          for (int k = 0; k < 4; ++k) acc[i][k] = t[k];
        }
    }
    asm volatile("" ::: "memory"); // (as density_stencil)
#pragma unroll
    for (int i = 0; i < NP; ++i)
#pragma unroll
      for (int s = 0; s < 4; ++s) Ns[i][s] = (s < nspec) ? exp(acc[i][s]) : 0.0; // Ns = exp(Ns) (:206)
  }
};

} // namespace srt
