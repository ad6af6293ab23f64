// srt_xform.hpp -- xform_double's frame rotations SM <-> MAG (SM_TO_MAG.f95, MAG_TO_SM.f95) and what they call:
// t4_d, t3_d, t2_d, t1_d, t5_d (T1.f95 .. T5.f95), t0_d (T0.f95), get_q_c_d (Get_q_c.f95), pol_to_cart_d and the three plane
// rotations rotate_{x,y,z}_d (Rotate_x.f95 .. Rotate_z.f95).
//
// Two halves.  The ANGLES depend on the date only and are host work, once per date, in double (angles, chain); the dipole tilt
// of the adapters (srt_host::dipole_tilt) is the `mu` of the same chain and is taken from here.  The ROTATIONS are per point:
// seven plane rotations one after the other in the Fortran's order, each with the Fortran's operations -- two products and
// one sum per changed component, products not fused into the sums -- from sines and cosines the host has computed, so that the
// host and the device give the same bits.  The chain is never collapsed into one 3 x 3 matrix: that would be other roundings.
//
// Compiles for the device (hipcc) and for the host (srt_host.cpp, plain C++).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define XF_HD __host__ __device__
#else
#define XF_HD
#endif
#if defined(__clang__)
#define XF_NOCONTRACT _Pragma("clang fp contract(off)")
#else
#define XF_NOCONTRACT // (g++: built with -ffp-contract=off)
#endif

namespace srt {
namespace xform {

// ROTATE_X_d / ROTATE_Y_d / ROTATE_Z_d with c = COS(ANGLE), s = SIN(ANGLE); in and out may not alias
XF_HD inline void rotate_x(double c, double s, const double in[3], double out[3]) {
  XF_NOCONTRACT
  out[0] = in[0];
  out[1] = in[1] * c + in[2] * s;
  out[2] = in[2] * c - in[1] * s;
}
XF_HD inline void rotate_y(double c, double s, const double in[3], double out[3]) {
  XF_NOCONTRACT
  out[0] = in[0] * c + in[2] * s;
  out[1] = in[1];
  out[2] = in[2] * c - in[0] * s;
}
XF_HD inline void rotate_z(double c, double s, const double in[3], double out[3]) {
  XF_NOCONTRACT
  out[0] = in[0] * c + in[1] * s;
  out[1] = in[1] * c - in[0] * s;
  out[2] = in[2];
}

// one plane rotation of a chain: about axis 0 / 1 / 2 = x / y / z by the angle whose cosine and sine are c, s
struct Rotation {
  int axis;
  double c, s;
};
// sm_to_mag_d or mag_to_sm_d for one date: the seven rotations in the order the Fortran applies them
struct Chain {
  static constexpr int N = 7;
  Rotation r[N];
};
XF_HD inline void apply(const Chain &ch, const double in[3], double out[3]) {
  double a[3] = {in[0], in[1], in[2]}, b[3];
  for (int k = 0; k < Chain::N; ++k) {
    const Rotation &r = ch.r[k];
    if (r.axis == 0) rotate_x(r.c, r.s, a, b);
    else if (r.axis == 1) rotate_y(r.c, r.s, a, b);
    else rotate_z(r.c, r.s, a, b);
    a[0] = b[0];
    a[1] = b[1];
    a[2] = b[2];
  }
  out[0] = a[0];
  out[1] = a[1];
  out[2] = a[2];
}

// ---- host, once per date -------------------------------------------------------------------------------------------
// the angles of T1 .. T5 for itime = (yearday, msec)
struct Angles {
  double theta;         // T1: Greenwich mean sidereal time
  double epsilon;       // T2: obliquity of the ecliptic
  double lamdas;        // T2: ecliptic longitude of the Sun
  double psi;           // T3: GSE -> GSM, from the dipole axis q_c in GSE
  double mu;            // T4: the dipole tilt, GSM -> SM
  double phi, lamda;    // T5: geographic latitude and longitude of the dipole pole
};
inline Angles angles(int yearday, int msec) {
  XF_NOCONTRACT
  const double degrad = 3.141592653589793238462643 / 180.0;
  Angles a;
  const int iyr = yearday / 1000, iday = yearday - iyr * 1000;
  const double ut = msec / 3600000.0, fracday = ut / 24.0;
  const double rmjd = 45.0 + (double)(iyr - 1859) * 365.0 + ((double)((iyr - 1861) / 4) + 1.0) + (double)iday - 1.0 + fracday;
  // T5.f95 and Get_q_c.f95: the pole
  const double factor = (rmjd - 46066.0) / 365.25;
  a.phi = (78.8 + 4.283e-2 * factor) * degrad;
  a.lamda = (289.1 - 1.413e-2 * factor) * degrad;
  // T0.f95, T1.f95, T2.f95
  const double t0 = (rmjd - 51544.5) / 36525.0;
  a.theta = (100.461 + 36000.770 * t0 + 15.04107 * ut) * degrad;
  a.epsilon = (23.439 - 0.013 * t0) * degrad;
  const double m = (357.528 + 35999.05 * t0 + 0.04107 * ut) * degrad;
  const double cg = 280.46 + 36000.772 * t0 + 0.04107 * ut;
  a.lamdas = (cg + (1.915 - 0.0048 * t0) * sin(m) + 0.02 * sin(2.0 * m)) * degrad;
  // get_q_c_d: pol_to_cart_d(phi, lamda, 1) -> t1_d inverse -> t2_d
  const double coslat = cos(a.phi);
  const double qg[3] = {1.0 * coslat * cos(a.lamda), 1.0 * coslat * sin(a.lamda), 1.0 * sin(a.phi)};
  double tmp[3], tmp2[3], qc[3];
  rotate_z(cos(-a.theta), sin(-a.theta), qg, tmp);
  rotate_x(cos(a.epsilon), sin(a.epsilon), tmp, tmp2);
  rotate_z(cos(a.lamdas), sin(a.lamdas), tmp2, qc);
  // T3.f95, T4.f95
  const double pid2 = 3.141592653589793238462643 / 2.0;
  a.psi = qc[2] == 0.0 ? -copysign(pid2, qc[1]) : -atan(qc[1] / qc[2]);
  a.mu = -atan(qc[0] / sqrt(qc[1] * qc[1] + qc[2] * qc[2]));
  return a;
}
// SM_TO_MAG.f95: t4(-1) t3(-1) t2(-1) t1(+1) t5(+1);  MAG_TO_SM.f95: t5(-1) t1(-1) t2(+1) t3(+1) t4(+1).  The Fortran hands
// iverse * angle to the rotation, which takes COS and SIN of that product: so does this.
inline Chain chain(int yearday, int msec, bool inverse) {
  const Angles a = angles(yearday, msec);
  const double pid2 = 3.141592653589793238462643 / 2.0;
  const double tilt = a.phi - pid2;
  Chain ch;
  auto rot = [](int axis, double angle) { return Rotation{axis, cos(angle), sin(angle)}; };
  if (!inverse) {
    ch.r[0] = rot(1, -a.mu);      // t4_d, iverse = -1: rotate_y(-mu)
    ch.r[1] = rot(0, -a.psi);     // t3_d, -1: rotate_x(-psi)
    ch.r[2] = rot(2, -a.lamdas);  // t2_d, -1: rotate_z(-lamdas), rotate_x(-epsilon)
    ch.r[3] = rot(0, -a.epsilon);
    ch.r[4] = rot(2, a.theta);    // t1_d, +1: rotate_z(theta)
    ch.r[5] = rot(2, a.lamda);    // t5_d, +1: rotate_z(lamda), rotate_y(phi - pi/2)
    ch.r[6] = rot(1, tilt);
  } else {
    ch.r[0] = rot(1, -tilt);      // t5_d, -1: rotate_y(-(phi - pi/2)), rotate_z(-lamda)
    ch.r[1] = rot(2, -a.lamda);
    ch.r[2] = rot(2, -a.theta);   // t1_d, -1
    ch.r[3] = rot(0, a.epsilon);  // t2_d, +1: rotate_x(epsilon), rotate_z(lamdas)
    ch.r[4] = rot(2, a.lamdas);
    ch.r[5] = rot(0, a.psi);      // t3_d, +1
    ch.r[6] = rot(1, a.mu);       // t4_d, +1
  }
  return ch;
}

} // namespace xform
} // namespace srt
