// srt_ngo_setup.hpp -- readinput of the Ngo density modules (ngo_dens_model.f95:29-160; ngo_3d_dens_model.f95 has the same) on
// the host: a parsed card file into the struct the device reads.  Shared by the library (srt_api_model.hpp, which evaluates the
// normalisation's one density on the device) and the host build of the density path (tests/native/ngo3d_host.cpp).
#pragma once
#include "srt_host.hpp"
#include "srt_models.hpp"
#include <cmath>
#include <cstring>

namespace srt {

// everything but the normalisation: g.ane0 is the file's value still
inline void ngo_fill(const srt_host::NgoConfig &cfg, NgoModel &g) {
  memset(&g, 0, sizeof g);
  g.r0 = 6370.0;
  g.pi32 = (double)3.141592653589793f; // default-real literal, ngo_dens_model.f95:36 (SURVEY A-6)
  g.num = cfg.num;
  g.kducts = cfg.kducts;
  g.kinit = 2;
  g.therm = cfg.therm;
  g.rbase = cfg.rbase;
  g.ane0 = cfg.ane0;
  for (int i = 0; i < 5; ++i) g.alpha0[i] = cfg.alpha0[i];
  g.rzero = cfg.rzero;
  g.scbot = cfg.scbot;
  g.lk = cfg.lk;
  g.expk = cfg.expk;
  g.ddk = cfg.ddk;
  g.rconsn = cfg.rconsn;
  g.scr = cfg.scr;
  for (int k = 0; k < 10; ++k) {
    g.l0[k] = cfg.l0[k]; g.def[k] = cfg.def[k]; g.dd[k] = cfg.dd[k];
    g.rducln[k] = cfg.rducln[k]; g.rducun[k] = cfg.rducun[k];
    g.rducls[k] = cfg.rducls[k]; g.rducus[k] = cfg.rducus[k];
    g.sidedu[k] = cfg.sidedu[k];
    g.hl2n[k] = cfg.hducln[k] * cfg.hducln[k]; g.hl2s[k] = cfg.hducls[k] * cfg.hducls[k];
    g.hu2n[k] = cfg.hducun[k] * cfg.hducun[k]; g.hu2s[k] = cfg.hducus[k] * cfg.hducus[k];
  }
}
// ane0 <- ane0*dsdens/ani(1) at (dsrrng, dsrlat)  (:120-123): the arguments of that one call of dens -- z(1), sin^2 z(2); the
// latitude dens() sees during it is the last satellite latitude read (:64), cfg.last_latitu.  grarad is built on the float32 pi.
inline void ngo_norm_point(const srt_host::NgoConfig &cfg, const NgoModel &g, double &z1, double &sinz22) {
  const double radgra = 180.0 / g.pi32, grarad = 1.0 / radgra;
  const double z2 = (90.0 - cfg.dsrlat) * grarad;
  z1 = cfg.dsrrng * g.r0;
  const double s2 = sin(z2);
  sinz22 = s2 * s2;
}

} // namespace srt
