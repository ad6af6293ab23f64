// srt_at64thch.hpp -- modelnum = 7: the AT64ThCh diffusive-equilibrium plasmasphere (AT64ThCh_adapter.f95:155-275).
//
// A restatement from the formulas, in double as written, operation for operation.  Above 400 km the electron density is scaled
// by zbrat = |B(point)| / |B(foot)|, where the foot is the end of the field line that geopack's TRACE_08 follows from the point
// through T04_s + IGRF down to the sphere r = (R_E + 400 km) / R_E (srt_fieldline.hpp): one trace per evaluated point.  Both
// magnitudes and their quotient are default REAL (fp32), as in the Fortran.
//
// Defined behaviour where the adapter has none (include/srt.h says the same to the caller):
//  1. :204 hands parmod, a DOUBLE array, to TRACE_08, whose PARMOD(10) is REAL: its T04_s reads the first 40 bytes of five
//     doubles as ten floats.  Here the trace sees real(parmod), as the adapter's own T04_s call (:281) does.
//  2. psi (:92) is a local that nothing sets and that only that last T04_s call reads; the reference's toolchain zeroes locals:
//     FieldConst::psi = 0 for this model (host).  RHAND_08 inside the trace reads geopack's own PSI from COMMON /GEOPACK1/
//     (RECALC_08's tilt angle): that one is `psi` below, a constant of the model.
//  3. A trace that has not ended after 500 points (the adapter's arrays; TRACE_08's own check is commented out) gives NaN
//     densities: a traced ray then ends with SRT_STOP_NUMERIC.
// The trace always uses T04_s and IGRF, whatever use_igrf / use_tsyganenko say: those choose bmag's base field (and B0).
// A point at or below 400 km takes zbrat = 1 without a trace; a line that leaves through the outer boundary has no foot on the
// sphere, and IGRF_GSM is evaluated wherever the trace stopped, as the Fortran does.
//
// On the device the points of a stencil are traced one after the other through ONE out-of-line body (foot_device): tracing
// them side by side (two points per packed IGRF instruction) was not built and not measured.
// Compiles for the device and, as HIP for the host alone, for the CPU tests (tests/native/at64thch_host.cpp).
#pragma once
#include "srt_device.hpp"
#include "srt_fieldline.hpp"

namespace srt {
namespace at64 {

constexpr double OH_HEIGHT = 400.0e3; // OH_transition_height (:162)

// IGRF_GSM at one point as a plain loop over the table (the host's branch; the device's igrf_core<1> is the same operations in
// the same order on terms read across the wave)
FL_HD static inline void igrf_point(const FieldConst &f, float xg, float yg, float zg, float &hx, float &hy, float &hz) {
  FL_NOCONTRACT
  const float a11 = f.A[0], a12 = f.A[1], a13 = f.A[2], a21 = f.A[3], a22 = f.A[4], a23 = f.A[5], a31 = f.A[6], a32 = f.A[7], a33 = f.A[8];
  const float xgeo = a11 * xg + a21 * yg + a31 * zg;
  const float ygeo = a12 * xg + a22 * yg + a32 * zg;
  const float zgeo = a13 * xg + a23 * yg + a33 * zg;
  const float rho2 = xgeo * xgeo + ygeo * ygeo;
  const float r = sqrtf(rho2 + zgeo * zgeo);
  const float c = zgeo / r;
  const float rho = sqrtf(rho2);
  const float s = rho / r;
  const bool pole = s < 1.e-5f;
  const float cf = pole ? 1.f : xgeo / rho;
  const float sf = pole ? 0.f : ygeo / rho;
  const float pp = 1.f / r;
  const int irp3 = (r + 2.f >= 1.f) ? (int)(r + 2.f) : 1; // (a NaN radius: 1, as the device's conversion gives)
  int nm = 3 + 30 / irp3;
  if (nm > 13) nm = 13;
  const int k = nm + 1;
  float p = 1.f, d = 0.f, bbr = 0.f, bbt = 0.f, bbf = 0.f, x = 0.f, y = 1.f, am = pp * pp;
  for (int m = 1; m <= k; ++m) {
    if (m > 1) {
      const float w = x;
      x = w * cf + y * sf;
      y = y * cf - w * sf;
    }
    float q = p, z = d, bi = 0.f, p2 = 0.f, d2 = 0.f, an = am;
    const int base = igrf_off(m) - m;
    for (int n = m; n <= k; ++n) {
      const float e = f.Gv[base + n], hh = f.Hv[base + n], xk = f.Rv[base + n];
      const float fn = (float)n;
      const float w = e * y + hh * x;
      bbr = bbr + (an * fn) * w * q;
      bbt = bbt - an * w * z;
      if (m != 1) bi = bi + an * (e * x - hh * y) * (pole ? z : q);
      const float dp = c * z - s * q - xk * d2;
      const float pm = c * q - xk * p2;
      d2 = z;
      p2 = q;
      z = dp;
      q = pm;
      an = an * pp;
    }
    d = s * d + c * p;
    p = s * p;
    if (m != 1) bbf = bbf + bi * (float)(m - 1);
    am = am * pp;
  }
  float bf;
  if (pole) bf = c < 0.f ? -bbf : bbf;
  else bf = bbf / s;
  const float he = bbr * s + bbt * c;
  const float hxgeo = he * cf - bf * sf, hygeo = he * sf + bf * cf, hzgeo = bbr * c - bbt * s;
  hx = a11 * hxgeo + a12 * hygeo + a13 * hzgeo;
  hy = a21 * hxgeo + a22 * hygeo + a23 * hzgeo;
  hz = a31 * hxgeo + a32 * hygeo + a33 * hzgeo;
}

#if defined(__HIPCC__)
// IGRF_GSM at one point per lane.  WAVE-UNIFORM CONTROL FLOW ONLY (igrf_core).  One compiled body.
__device__ __noinline__ void igrf1_device(const FieldConst &f, float xg, float yg, float zg, float &hx, float &hy, float &hz) {
  const float x1[1] = {xg}, y1[1] = {yg}, z1[1] = {zg};
  float a[1], b[1], c[1];
  igrf_core<1>(f, x1, y1, z1, a, b, c);
  hx = a[0];
  hy = b[0];
  hz = c[0];
}
// RHAND_08's field: T04_s(real(parmod), geopack's PSI) + IGRF_GSM.  One compiled body for the tracer's six call sites.
__device__ __noinline__ void trace_field_device(const FieldConst &f, float psi, float x, float y, float z, float &bx, float &by, float &bz) {
#pragma clang fp contract(off)
  float tx, ty, tz, hx, hy, hz;
  t04::t04_s(f.parmod, psi, x, y, z, tx, ty, tz);
  igrf1_device(f, x, y, z, hx, hy, hz);
  bx = tx + hx;
  by = ty + hy;
  bz = tz + hz;
}
struct WaveField {
  const FieldConst *f;
  float psi;
  __device__ __forceinline__ void operator()(float x, float y, float z, float &bx, float &by, float &bz) const {
    trace_field_device(*f, psi, x, y, z, bx, by, bz);
  }
};
// TRACE_08 for one point per lane: the one out-of-line body of the tracer.  WAVE-UNIFORM CONTROL FLOW ONLY.
__device__ __noinline__ fl::Foot foot_device(const FieldConst &f, float psi, fl::TraceConst c, float x, float y, float z, bool live) {
  const WaveField field{&f, psi};
  return fl::trace(field, c, x, y, z, live);
}
#endif
struct HostField {
  const FieldConst *f;
  float psi;
  FL_HD void operator()(float x, float y, float z, float &bx, float &by, float &bz) const {
    FL_NOCONTRACT
    float tx, ty, tz, hx, hy, hz;
    t04::t04_s(f->parmod, psi, x, y, z, tx, ty, tz);
    igrf_point(*f, x, y, z, hx, hy, hz);
    bx = tx + hx;
    by = ty + hy;
    bz = tz + hz;
  }
};

// the adapter's trace constants (:191-196): DIR 1, DSMAX 1, ERR 1e-4, RLIM 60, R0 = real((R_E + 400 km) / R_E)
FL_HD static inline fl::TraceConst trace_const() {
  fl::TraceConst c;
  c.dir = 1.f;
  c.dsmax = 1.f;
  c.err = 0.0001f;
  c.rlim = 60.f;
  c.r0 = (float)((OH_HEIGHT + R_E) / R_E);
  c.lmax = fl::LMAX;
  return c;
}

// :155-168 and :217-274 given zbrat: densities in m^-3 (electrons, O+, H+)
FL_HD static inline void plasma_density(int gcpm_kp, double x, double y, double z, double zbrat, double Ns[3]) {
  FL_NOCONTRACT
  const double radial_dist = sqrt(x * x + y * y + z * z);
  const double h = radial_dist - R_E;
  const double r0 = R_E + OH_HEIGHT;
  const double R = radial_dist / r0;
  const double lat_angle = asin(z / radial_dist);
  const double cos_lat = cos(lat_angle);
  const double L = (radial_dist / R_E) / (cos_lat * cos_lat);
  const double temp_gradient = 800.0, OH_transition_temp = 750.0;
  const double a = temp_gradient * (r0 / 1.0e6) / OH_transition_temp - 1.0;
  const double tt = (R * (1.0 + a) - a) / R;
  const double zg = (r0 / 1.0e6) / a * log(tt);
  const double peak_height = 300.0e3;
  const double Rp = (R_E + peak_height) / r0;
  const double c_p = 1.0 / ((Rp * (1.0 + a) - a) * Rp);
  const double neutral_temp = 1000.0;
  const double gh = 9.80665;
  const double mpg = 1.6726219e-27 * gh;
  const double H0 = 1.380658e-23 * neutral_temp / (16.0 * mpg) / 1.0e6;
  const double zz = zg + (c_p * H0 * exp(((peak_height - h) / 1.0e6) / H0));
  const double T = OH_transition_temp * tt;
  const double H1 = 1.380658e-23 * OH_transition_temp / mpg / 1.0e6;
  const double H3 = 1.380658e-23 * OH_transition_temp / (16.0 * mpg) / 1.0e6;
  const double etrans_dens = 2.0e11;
  const double n10 = 0.5 * etrans_dens, n30 = 0.5 * etrans_dens;
  const double ne_tmp = sqrt((etrans_dens * OH_transition_temp) * zbrat *
                             ((n10 * OH_transition_temp) * exp(-1.0 * zz / H1) + (n30 * OH_transition_temp) * exp(-1.0 * zz / H3))) / T;
  const double R13 = (n10 / n30) * exp(zz * ((H1 - H3) / (H1 * H3)));
  const double SN = 124.0 * pow(3.0 / L, 4.0) * 1.0e6;
  const double Lpp = 5.6 - (0.46 * (double)gcpm_kp);
  const double Lw = 0.14;
  const double tran = 0.5 * tanh(3.4534 * (L - Lpp) / Lw) + 0.5;
  const double ne = (1.0 - tran) * ne_tmp + tran * SN;
  Ns[0] = ne;
  Ns[1] = ne / (1.0 + R13);
  Ns[2] = ne / (1.0 + (1.0 / R13));
}

} // namespace at64

struct At64ThChModel {
  // the handle's field constants, which the trace ALWAYS uses (coefficient table, GEO->GSM matrix, parmod) and which say
  // what bmag's base field is (use_igrf): the device's copy on the device.  Kept by reference: what the model adds to them
  // lives here, so that FieldConst -- and with it every other kernel -- stays as it is.
  const FieldConst *fld;
  float psi; // geopack's PSI (RECALC_08's dipole tilt, COMMON /GEOPACK1/ word 16) for the trace's T04_s
  int gcpm_kp;

  struct Dens {
    double n[3];
  };
  // zbrat at a point: 1 at or below 400 km, else real(bmag / b_oh).  WAVE-UNIFORM CONTROL FLOW ONLY on the device.
  FL_HD double zbrat_at(double x, double y, double z) const {
    FL_NOCONTRACT
    const FieldConst &f = *fld;
    // SM_TO_GSM_d, then real(x_gsm / R_E)
    const float xg = (float)((x * f.cm - z * f.sm) / R_E);
    const float yg = (float)(y / R_E);
    const float zg = (float)((z * f.cm + x * f.sm) / R_E);
    float bx, by, bz;
    if (f.use_igrf) { // wave-uniform
#if defined(__HIP_DEVICE_COMPILE__)
      at64::igrf1_device(f, xg, yg, zg, bx, by, bz);
#else
      at64::igrf_point(f, xg, yg, zg, bx, by, bz);
#endif
    } else { // the dipole in SM, rotated to GSM, in nT as REAL (trig-free form as in bfield_igrf)
      const double rho2 = x * x + y * y, r2 = rho2 + z * z, r = sqrt(r2);
      const double k = f.bo_re3 / (r2 * r2 * r);
      const double dx = -3.0 * k * x * z, dy = -3.0 * k * y * z, dz = k * (rho2 - 2.0 * z * z);
      bx = (float)(1.0e9 * (dx * f.cm - dz * f.sm));
      by = (float)(1.0e9 * dy);
      bz = (float)(1.0e9 * (dz * f.cm + dx * f.sm));
    }
    const float bmag = sqrtf(bx * bx + by * by + bz * bz);
    const double h = sqrt(x * x + y * y + z * z) - R_E;
    const bool live = h > 400e3;
    const fl::TraceConst c = at64::trace_const();
    float ox, oy, oz;
#if defined(__HIP_DEVICE_COMPILE__)
    const fl::Foot ft = at64::foot_device(f, psi, c, xg, yg, zg, live);
    at64::igrf1_device(f, ft.x, ft.y, ft.z, ox, oy, oz);
#else
    const at64::HostField field{&f, psi};
    const fl::Foot ft = fl::trace(field, c, xg, yg, zg, live);
    at64::igrf_point(f, ft.x, ft.y, ft.z, ox, oy, oz);
#endif
    const float b_oh = sqrtf(ox * ox + oy * oy + oz * oz);
    return live ? (double)(float)((double)bmag / (double)b_oh) : 1.0;
  }
  // noinline: ONE compiled body, so that a point gets the same bits on whichever path or lane evaluates it
#if defined(__HIPCC__)
  FL_HD __noinline__
#else
  __attribute__((noinline))
#endif
  Dens dens_point(double x, double y, double z) const {
    Dens d;
    at64::plasma_density(gcpm_kp, x, y, z, zbrat_at(x, y, z), d.n);
    return d;
  }

#if defined(__HIPCC__)
  template <int NP>
  __device__ __forceinline__ void density(const double (&p)[NP][3], double (&Ns)[NP][4], double *) const {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const Dens d = dens_point(p[i][0], p[i][1], p[i][2]);
#pragma unroll
      for (int s = 0; s < 3; ++s) Ns[i][s] = d.n[s];
      Ns[i][3] = 0.0;
    }
  }
  // Stencil of one right-hand side: Ns[0] centre, Ns[1+2a] = c + d_a e_a, Ns[2+2a] = c - d_a e_a, Ns[7] = extra.  Every lane
  // of the wave evaluates every point, whether it carries a ray or not (the trace is wave-uniform).
  template <int NE>
  __device__ __forceinline__ void density_stencil(const double c0[3], const double d[3], const double *extra, double (&Ns)[7 + NE][4],
                                                  double *, bool = true) const {
#pragma unroll
    for (int i = 0; i < 7 + NE; ++i) {
      double q[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        double v = c0[a];
        if (i == 1 + 2 * a) v = c0[a] + d[a];
        if (i == 2 + 2 * a) v = c0[a] - d[a];
        if (NE && i == 7) v = extra[a];
        q[a] = v;
      }
      const Dens r = dens_point(q[0], q[1], q[2]);
#pragma unroll
      for (int s = 0; s < 3; ++s) Ns[i][s] = r.n[s];
      Ns[i][3] = 0.0;
    }
  }
#endif
};

} // namespace srt
