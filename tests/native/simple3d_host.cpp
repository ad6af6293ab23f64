// Host build of stanford_raytracer_amd/csrc/srt_simple3d.hpp for the CPU tests (tests/test_simple3d_host.py): the same source
// the device compiles, checked on the CPU against goldens captured from the reference's simple_3d_model_adapter.
#include "../../stanford_raytracer_amd/csrc/srt_simple3d.hpp"
// x[n][3] -> Ns[n][4]
extern "C" void s3dh_density(double kp, int yearday, int fixed_mlt, double mlt, long n, const double *x, double *Ns) {
  srt::Simple3dModel m;
  m.c.kp = kp;
  m.c.year = yearday / 1000;
  m.c.doy = yearday - m.c.year * 1000;
  m.c.fixed_mlt = fixed_mlt;
  m.c.mlt = mlt;
  for (long i = 0; i < n; ++i) {
    const srt::Simple3dModel::Dens d = m.dens_point(x[3 * i], x[3 * i + 1], x[3 * i + 2]);
    for (int s = 0; s < 4; ++s) Ns[4 * i + s] = d.n[s];
  }
}
// the MLT-only terms of a point: a8, a9, geosync trough, season term, zl
extern "C" void s3dh_mlt_terms(double amlt, double kp, double doy, double *out) {
  const srt::s3d::MltTerms t = srt::s3d::mlt_terms(amlt, kp, doy);
  out[0] = t.a8, out[1] = t.a9, out[2] = t.geosync, out[3] = t.season, out[4] = t.zl;
}
