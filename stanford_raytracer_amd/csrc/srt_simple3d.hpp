// srt_simple3d.hpp -- modelnum = 6: the closed-form "simplified GCPM" (simple_3d_model_adapter.f95:701-818 and what it
// calls: cartesian_to_spherical, pp_profile / bulge (pp_profile_d.f95), ne_ps, ne_trough, switch (switch_d.f95),
// check_crossing, main_ps_density, find_intersection_iono_ps, ne_iono, and the He+ / O+ / H+ split).
//
// A restatement from the formulas, operation for operation: the Fortran's order of evaluation is kept, its default-real
// literals are (double)...f (SURVEY A-6), products are not fused into sums (fp contract off in every function).
//
// Defined behaviour for the adapter's three locals that nothing sets (the reference's toolchain zeroes them, SURVEY A-1):
//   rz12 in ne_ps (:106) = 0; diff in find_intersection_iono_ps (:585) = 0 on the first trip of the altitude search, which
//   therefore never flips its step (2000 km -> 3000 km); switch_cap in funcPlasmaParams (:790) = 0, so aHeH is not reduced.
// With do_cap = 0 the results of ne_cap, poleward_edge, tranlow and tranhigh are dead: none of it is here, nor the PN table.
//
// Exact restructuring, no approximation: everything that depends on the point only through its MLT -- bulge's a8,
// the trough density at geosynchronous orbit, check_crossing's zl -- is evaluated once per point where the Fortran
// evaluates it in funcPlasmaParams, again in main_ps_density and again in every trip of the altitude search; likewise the
// latitude-only part of ne_iono and the date-only part of ne_ps.  Same functions of the same arguments: the same values.
// The values the Fortran computes and never uses (h in ne_ps, the result of pp_profile(r/REkm), ne_cap) are left out.
//
// check_crossing's "Failed to find knee" stop becomes a NaN density (the trace kernel then ends the ray with
// SRT_STOP_NUMERIC, as for the other process-killing paths of the reference).
//
// Compiles for the device (hipcc) and for the host (tests/native/simple3d_host.cpp builds it with g++).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define S3D_HD __host__ __device__
#define S3D_NOINLINE __noinline__
#else
#define S3D_HD
#define S3D_NOINLINE __attribute__((noinline))
#endif
#if defined(__clang__)
#define S3D_NOCONTRACT _Pragma("clang fp contract(off)")
#else
#define S3D_NOCONTRACT // (g++: built with -ffp-contract=off)
#endif
// a default-real literal of the Fortran, as the double it is promoted to
#define S3D_R(lit_) ((double)lit_##f)

namespace srt {
namespace s3d {

constexpr double S_PI = 3.141592653589793238462643; // constants.f95
constexpr double S_RE = 6371.2e3;
constexpr double S_REKM = S_RE * 1e-3;
constexpr double S_R2D = 180.0 / S_PI;
constexpr double RZ12 = 0.0;  // ne_ps's unset local (see above)
constexpr double F107 = 70.0; // :89
constexpr double IONO_MERGE_RADIUS = 10000.0; // :86

// x**y.  On the device one out-of-line copy: the library's pow is several hundred instructions at every call site.
#if defined(__HIP_DEVICE_COMPILE__)
S3D_HD __noinline__ static double s_pow(double x, double y) { return ::pow(x, y); }
#else
S3D_HD static inline double s_pow(double x, double y) { return ::pow(x, y); }
#endif

// switch (switch_d.f95): tanh transition from 0 to 1 around a, width da; 3.4534 is a default-real literal
S3D_HD static inline double s_switch(double x, double a, double da) {
  S3D_NOCONTRACT
  const double c = S3D_R(3.4534) / da;
  return tanh(c * (x - a)) / 2.0 + 0.5;
}

// x**n for an integer n >= 0 by repeated squaring (ne_iono's lat**(11-i))
S3D_HD static inline double s_powi(double a, int b) {
  S3D_NOCONTRACT
  double r = (b & 1) ? a : 1.0;
  while ((b >>= 1) != 0) {
    a *= a;
    if (b & 1) r *= a;
  }
  return r;
}

// What a point's density needs of its MLT, Kp and the date alone.
struct MltTerms {
  double a8, a9;  // bulge: plasmapause location and slope
  double geosync; // ne_trough's geosync_trough
  double season;  // ne_ps: 0.15 (cos 2f - 0.5 cos 4f) + (0.00127 rz12 - 0.0635)
  double zl;      // check_crossing
};

// bulge (pp_profile_d.f95:52-131)
S3D_HD static inline void bulge(double amlt, double akp, double &a8, double &a9) {
  S3D_NOCONTRACT
  const double ahour_rad = S3D_R(0.26179939), ahrrad = S3D_R(2.6179939e-1); // the two data statements
  const double centroid = 47.0 / (akp + S3D_R(3.9)) + S3D_R(11.3);
  double x = amlt - centroid;
  if (x < -12.0) x = x + 24.0;
  if (x > 12.0) x = x - 24.0;
  const double absx = fabs(x) * ahrrad;
  const double along = amlt * ahour_rad + S3D_R(1.5707963);
  const double salong = sin(along);
  const double b1 = S3D_R(0.043) * salong - S3D_R(0.4589);
  const double b2 = -(S3D_R(0.361) * salong) + S3D_R(5.7464);
  a8 = (b1 * akp + b2) * (1.0 + exp(-(1.5 * absx * absx) + S3D_R(0.08) * absx - S3D_R(0.7)));
  const double b3 = -(S3D_R(0.0243) * salong) + S3D_R(0.2464);
  const double b4 = -(S3D_R(0.3137) * salong) - S3D_R(5.2214);
  const double b5 = S3D_R(3.5817) * salong + S3D_R(48.8114);
  a9 = b3 * akp * akp + b4 * akp + b5;
}

// pp_profile (pp_profile_d.f95:27-49) with bulge's a8, a9 handed in
S3D_HD static inline double pp_profile(double al, double a8, double a9) {
  S3D_NOCONTRACT
  const double f = 2.0 * (a9 - 1.0) * log10(al / a8);
  const double factor = (27.75 < f) ? 27.75 : f; // min(27.75, .)
  return s_pow(1.0 + s_pow(10.0, factor), -(a9 / (a9 - 1.0)));
}

// ne_ps (:102-122) given the date term
S3D_HD static inline double ne_ps(double L, double season) {
  S3D_NOCONTRACT
  const double a6 = -S3D_R(0.79), a7 = S3D_R(5.208);
  const double x234 = season * exp(-((L - 2.0) / 1.5));
  return s_pow(10.0, a6 * L + a7 + x234);
}
S3D_HD static inline double ne_ps_season(double doy) {
  S3D_NOCONTRACT
  const double doy_factor = S_PI * (doy + 9.0) / 365.0;
  return 0.15 * (cos(2.0 * doy_factor) - 0.5 * cos(4.0 * doy_factor)) + (0.00127 * RZ12 - 0.0635);
}

// ne_trough (:125-202): the trough density at geosynchronous orbit (a function of MLT and Kp) ...
S3D_HD static inline double trough_geosync(double amlt, double akp) {
  S3D_NOCONTRACT
  const double phitp = S3D_R(0.145) * (akp * akp) - S3D_R(2.63) * akp + S3D_R(21.86);
  const double antp = (phitp - 3.5) * S3D_R(0.56);
  const double t0 = 26.0 - phitp, t1 = antp / S3D_R(0.83);
  const double damping_time = (t0 < t1) ? t0 : t1;
  const double damping = -1.0 * antp / damping_time;
  const double down_time = phitp + damping_time;
  const double del = 3.5 - (down_time - 24.0);
  double center = 3.5 - del / 2.0;
  if (center < 0.0) center = 24.0 + center;
  double diff = amlt - center;
  if (diff < -12.0) diff = 24.0 + diff;
  if (diff > 12.0) diff = diff - 24.0;
  const double aminden = S3D_R(0.18);
  const double width = 2.0 * del;
  const double denmin = aminden + diff * diff / (del * width);
  const double dengrow = S3D_R(0.56) * (amlt - 3.5) + aminden;
  const double sdel = S3D_R(0.4), shift = 0.5;
  const double switch1 = s_switch(amlt, 3.5 + shift, sdel);
  const double switch2 = s_switch(amlt, phitp, 0.5);
  if (amlt < 8.0) {
    const double dendamp = antp + damping * (amlt + 24.0 - phitp);
    const double switch0 = s_switch(amlt, down_time - 24.0 - shift, sdel);
    return denmin * switch0 * (1.0 - switch1) + dendamp * (1.0 - switch0) + dengrow * switch1 * (1.0 - switch2);
  }
  const double dendamp = antp + damping * (amlt - phitp);
  const double switch3 = s_switch(amlt, down_time - shift, sdel);
  return denmin * switch3 + dengrow * switch1 * (1.0 - switch2) + dendamp * switch2 * (1.0 - switch3);
}
// ... scaled to L with a power law of -4.5
S3D_HD static inline double ne_trough(double L, double geosync) {
  S3D_NOCONTRACT
  return geosync * s_pow(L, -4.5) / 2.0514092e-4;
}

// check_crossing (:206-244): where plasmasphere x plasmapause profile crosses the trough, by a halving search from a8.
// NaN when the Fortran stops ("Failed to find knee").
S3D_HD static inline double check_crossing(const MltTerms &t) {
  S3D_NOCONTRACT
  double stepl = 0.5, zl = t.a8, diff;
  int icount = -1; // the evaluation at a8 itself, then the Fortran's loop (its icount starts at 0)
  for (;;) {
    const double b = pp_profile(zl, t.a8, t.a9);
    const double a = ne_ps(zl, t.season);
    const double c = ne_trough(zl, t.geosync);
    diff = a * b - c;
    if (++icount > 100) return NAN;
    if (!(fabs(stepl) > 0.05)) return zl;
    if ((diff < 0.0 && stepl > 0.0) || (diff > 0.0 && stepl < 0.0)) stepl = -stepl / 2.0;
    zl = zl + stepl;
  }
}

S3D_HD static inline MltTerms mlt_terms(double amlt, double akp, double doy) {
  MltTerms t;
  bulge(amlt, akp, t.a8, t.a9);
  t.geosync = trough_geosync(amlt, akp);
  t.season = ne_ps_season(doy);
  t.zl = check_crossing(t);
  return t;
}

// main_ps_density (:529-565) with do_trough = 1, do_cap = 0
S3D_HD static inline double main_ps_density(double L, const MltTerms &t) {
  S3D_NOCONTRACT
  const double ne_eq_ps = ne_ps(L, t.season);
  const double ne_eq_trough = ne_trough(L, t.geosync);
  const double sw = s_switch(L, t.zl, 0.6);
  return ne_eq_ps * (1.0 - sw) + sw * ne_eq_trough;
}

// ne_iono (:289-359): what depends on latitude and MLT only ...
struct IonoTerms {
  double dens_day, dens_nite, grad_day, grad_nite, s;
};
S3D_HD static inline double iono_gauss(const double *c, double lat) {
  S3D_NOCONTRACT
  const double q1 = (lat - c[1]) / c[2], q2 = (lat - c[4]) / c[5];
  return c[0] * exp(-(q1 * q1)) + c[3] * exp(-(q2 * q2)) + c[6] + c[7] * lat + c[8] * (lat * lat);
}
S3D_HD static inline IonoTerms iono_terms(double lat, double mlt) {
  S3D_NOCONTRACT
  const double dens_coef_day[9] = {S3D_R(9.23183e+03), -S3D_R(2.23382e+01), S3D_R(1.49365e+01), S3D_R(1.70763e+04), S3D_R(2.63301e+01),
                                   S3D_R(3.75599e+01), S3D_R(9.15522e+03), -S3D_R(3.31022e+01), -S3D_R(6.13435e-01)};
  const double grad_coef_day[11] = {S3D_R(2.31678e-22),  S3D_R(1.17475e-20),  -S3D_R(5.20743e-18), -S3D_R(1.98686e-16),
                                    S3D_R(4.44845e-14),  S3D_R(1.19067e-12),  -S3D_R(1.85079e-10), -S3D_R(3.38517e-09),
                                    S3D_R(3.84124e-07),  S3D_R(3.35202e-06),  -S3D_R(1.84164e-03)};
  const double dens_coef_nite[9] = {S3D_R(6.99184e+03), -S3D_R(3.11663e+00), S3D_R(1.30464e+01), S3D_R(8.58528e+03), S3D_R(2.19513e+01),
                                    S3D_R(1.56983e+01), S3D_R(2.89385e+03), -S3D_R(1.87291e+01), S3D_R(3.21094e-01)};
  const double grad_coef_nite[11] = {S3D_R(2.39859e-23),  -S3D_R(1.28908e-20), -S3D_R(1.77123e-20), S3D_R(2.32415e-16),
                                     -S3D_R(4.42548e-15), -S3D_R(1.46548e-12), S3D_R(2.84474e-11),  S3D_R(3.59593e-09),
                                     -S3D_R(2.62414e-08), -S3D_R(2.70750e-06), -S3D_R(1.63765e-03)};
  IonoTerms t;
  t.dens_day = iono_gauss(dens_coef_day, lat);
  t.dens_nite = iono_gauss(dens_coef_nite, lat);
  t.grad_day = 0.0;
  t.grad_nite = 0.0;
  for (int i = 1; i <= 11; ++i) {
    const double p = s_powi(lat, 11 - i);
    t.grad_day = t.grad_day + grad_coef_day[i - 1] * p;
    t.grad_nite = t.grad_nite + grad_coef_nite[i - 1] * p;
  }
  const double mltslope = 0.1, m24 = fmod(mlt, 24.0);
  const double s1 = 1.0 / (1.0 + exp((m24 - 18.0) / mltslope));
  const double s2 = 1.0 / (1.0 + exp((m24 - 6.0) / mltslope));
  t.s = s1 - s2;
  return t;
}
// ... extrapolated in log space from 1500 km to the altitude, day and night faded
S3D_HD static inline double ne_iono(const IonoTerms &t, double alt) {
  S3D_NOCONTRACT
  const double dd = t.dens_day * s_pow(10.0, t.grad_day * (alt - 1500.0));
  const double dn = t.dens_nite * s_pow(10.0, t.grad_nite * (alt - 1500.0));
  return t.s * dd + (1.0 - t.s) * dn;
}

// find_intersection_iono_ps (:569-606): the altitude where ionosphere and plasmasphere densities meet.  diff is 0 on the
// first trip (see the top of the file).
S3D_HD static inline double find_intersection_iono_ps(double cos2lam, const MltTerms &mt, const IonoTerms &it) {
  S3D_NOCONTRACT
  double stepl = 1000.0, alt_guess = 2000.0, diff = 0.0;
  while (fabs(stepl) > 100.0 && alt_guess < 10000.0) {
    if ((diff < 0.0 && stepl > 0.0) || (diff > 0.0 && stepl < 0.0)) stepl = -stepl / 2.0;
    alt_guess = alt_guess + stepl;
    const double L_cur = (alt_guess + S_REKM) / (S_REKM * cos2lam);
    const double ps = main_ps_density(L_cur, mt);
    const double iono = ne_iono(it, alt_guess);
    diff = iono - ps;
  }
  return alt_guess;
}

// The per-model constants (simpleStateData less the field tail, which lives in Common like every model's)
struct Simple3dConst {
  double kp;
  int year, doy; // itime(1) / 1000 and the rest
  int fixed_mlt;
  double mlt;
};

// funcPlasmaParams :701-818, densities in m^-3 (electrons, H+, He+, O+)
S3D_HD static inline void plasma_density(const Simple3dConst &c, double x, double y, double z, double Ns[4]) {
  S3D_NOCONTRACT
  // cartesian_to_spherical (util.f95:109-122)
  const double p1 = sqrt(x * x + y * y + z * z);
  const double p2 = atan2(y, x);
  const double p3 = (p1 != 0.0) ? acos(z / p1) : 0.0;
  const double akp = c.kp;
  const double amlt = (c.fixed_mlt == 1) ? c.mlt : fmod(24.0 * p2 / (2.0 * S_PI) + 12.0, 24.0);
  const double lamr = S_PI / 2.0 - p3;
  const double lam = lamr * S_R2D;
  const double cl = cos(lamr), cos2lam = cl * cl;
  const double L = p1 / (S_RE * cos2lam);
  const double r = S_REKM * L * cos2lam;
  const MltTerms mt = mlt_terms(amlt, akp, (double)c.doy);
  const IonoTerms it = iono_terms(lam, amlt);
  double ne_eq_ps = main_ps_density(L, mt);
  const double iono_merge_altitude = find_intersection_iono_ps(cos2lam, mt, it);
  const double ne_eq_iono = ne_iono(it, r - S_REKM);
  const double switch_iono2ps = 1.0 - s_switch(r - S_REKM, iono_merge_altitude - IONO_MERGE_RADIUS / 2.0, IONO_MERGE_RADIUS);
  ne_eq_ps = ne_eq_iono * switch_iono2ps + (1.0 - switch_iono2ps) * ne_eq_ps;
  const double ce = ne_eq_ps;
  // He+ to H+ ratio, relative O+ density (:787-803); switch_cap = 0
  const double switch_cap = 0.0;
  double aHeH = s_pow(10.0, -S3D_R(1.541) - S3D_R(0.176) * r / S_REKM + S3D_R(8.557e-3) * F107 - S3D_R(1.458e-5) * F107 * F107);
  aHeH = aHeH * (1.0 - switch_cap);
  const double aheight = r - S_REKM;
  const double q = 1.0 + aheight * aheight / 281250.0;
  const double alphaO = S3D_R(0.995) / (q * q * q) + S3D_R(0.005);
  double alphaHe = 0.0;
  if (aHeH != 0.0) {
    const double alphaHeP = (1.0 - alphaO) / (1.0 + 1.0 / aHeH);
    const double v = alphaHeP * (1.0 - exp(-(aheight / 600.0)));
    alphaHe = (v < 0.0) ? 0.0 : v; // max(0.0, .); a NaN stays one
  }
  const double che = alphaHe * ce;
  const double co = alphaO * ce;
  const double ch = ce - che - co;
  Ns[0] = 1.0e6 * ce;
  Ns[1] = 1.0e6 * ch;
  Ns[2] = 1.0e6 * che;
  Ns[3] = 1.0e6 * co;
}

} // namespace s3d

struct Simple3dModel {
  s3d::Simple3dConst c;

  struct Dens {
    double n[4];
  };
  // noinline: ONE compiled body, so that a point gets the same bits on whichever path or lane evaluates it
  S3D_HD S3D_NOINLINE Dens dens_point(double x, double y, double z) const {
    Dens d;
    s3d::plasma_density(c, x, y, z, d.n);
    return d;
  }

#if defined(__HIPCC__)
  template <int NP>
  __device__ __forceinline__ void density(const double (&p)[NP][3], double (&Ns)[NP][4], double *) const {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const Dens d = dens_point(p[i][0], p[i][1], p[i][2]);
#pragma unroll
      for (int s = 0; s < 4; ++s) Ns[i][s] = d.n[s];
    }
  }
  // Stencil of one right-hand side: Ns[0] centre, Ns[1+2a] = c + d_a e_a, Ns[2+2a] = c - d_a e_a, Ns[7] = extra.
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
      for (int s = 0; s < 4; ++s) Ns[i][s] = r.n[s];
    }
  }
#endif
};

} // namespace srt
