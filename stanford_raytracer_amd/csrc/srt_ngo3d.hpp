// srt_ngo3d.hpp -- modelnum = 5: the 3-D Ngo model (ngo_3d_dens_model_adapter.f95:120-177 + ngo_3d_dens_model.f95, which is
// ngo_dens_model.f95 with d-prefixed intrinsic names and a `save`).
//
// Modelnum 1's diffusive-equilibrium plasmasphere with the plasmapause moved, per evaluated point, to where bulge
// (pp_profile_d.f95:52-131) puts it for the point's MLT and the run's Kp: the adapter calls pp_profile(r/r0, amlt, kp, a8), uses
// nothing of it but a8, and sets the density module's lk = a8 - ddk before it calls dens.  dens reads lk in two places, the knee
// (deltal = l - lk) and the sinusoidal perturbation of the ducts (delk, critl); NgoModel's bodies take it as an argument there.
// The file's own lk serves only readinput's normalisation of ane0, once at setup (NgoModel::ane0 holds the result).
//
// The head of a point: its longitude as cartesian_to_spherical gives it (atan2(y, x), as srt_simple3d.hpp restates it), amlt =
// mod(24 p(2) / (2 pi) + 12, 24) or the state's MLT when fixed_MLT = 1, then s3d::bulge -- the Fortran's order of operations, its
// default-real literals, products not fused into sums.  ONE body for both MLT modes: with fixed_MLT = 1 the value is the same
// for every point and is computed for every point all the same, so that a point's bits do not depend on the mode.
// L, lam, z(1), z(2) and latitu are those of modelnum 1's adapter (NgoModel::dens_point).
//
// Compiles for the device and, less the cross-lane stencil service, for the host (tests/native/ngo3d_host.cpp).
#pragma once
#include "srt_models.hpp"
#include "srt_simple3d.hpp"

namespace srt {

struct Ngo3dModel {
  NgoModel ngo; // readinput's state, ane0 normalised with the file's lk
  double kp, mlt;
  int fixed_mlt;

  // lk of the point (x, y, .): a8(amlt, kp) - ddk (:127-132, :154-160)
  SRT_HD __forceinline__ double lk_at(double x, double y) const {
    S3D_NOCONTRACT
    const double p2 = atan2(y, x);
    const double amlt = (fixed_mlt == 1) ? mlt : fmod(24.0 * p2 / (2.0 * s3d::S_PI) + 12.0, 24.0);
    double a8, a9;
    s3d::bulge(amlt, kp, a8, a9);
    return a8 - ngo.ddk;
  }

  // noinline: ONE compiled body, so that a point gets the same arithmetic whichever path (and lane) evaluates it
  SRT_HD __noinline__ void dens_point(double x, double y, double z, double Ns[4]) const {
    double rho2 = x * x + y * y;
    double r2 = rho2 + z * z;
    double r = sqrt(r2);
    ngo.dens_core_at<true>(ngo.r0 * r / R_E, rho2 / r2, z, lk_at(x, y), Ns);
  }

  template <int NP>
  __device__ __forceinline__ void density(const double (&p)[NP][3], double (&Ns)[NP][4], double *) const {
#pragma unroll
    for (int i = 0; i < NP; ++i) dens_point(p[i][0], p[i][1], p[i][2], Ns[i]);
  }
  // NgoModel::dens_pair with the two points' heads next to each other in front of it: two independent chains all the way
  __device__ __noinline__ NgoModel::Dens2 dens_pair(double ax, double ay, double az, double bx, double by, double bz) const {
    NgoModel::Dens2 r;
    const double rhoa = ax * ax + ay * ay, ra2 = rhoa + az * az, ra = sqrt(ra2);
    const double rhob = bx * bx + by * by, rb2 = rhob + bz * bz, rb = sqrt(rb2);
    const double z1[2] = {ngo.r0 * ra / R_E, ngo.r0 * rb / R_E}, s2[2] = {rhoa / ra2, rhob / rb2}, lat[2] = {az, bz};
    const double lk2[2] = {lk_at(ax, ay), lk_at(bx, by)};
    double N[2][4];
    ngo.dens_core2<true>(z1, s2, lat, lk2, N);
#pragma unroll
    for (int s = 0; s < 4; ++s) r.a[s] = N[0][s], r.b[s] = N[1][s];
    return r;
  }
  // the stencil service of modelnum 1, tail mode included: the same function of the same arguments on another lane
  template <int NE>
  __device__ __forceinline__ void density_stencil(const double c[3], const double d[3], const double *extra,
                                                  double (&Ns)[7 + NE][4], double *, bool need = true) const {
    NgoModel::stencil_of<NE>(*this, c, d, extra, Ns, need);
  }
};

} // namespace srt
