// Host build of the Ngo density path -- stanford_raytracer_amd/csrc/srt_ngo3d.hpp's per-point head and srt_models.hpp's
// dens_core / ducts / taper, the very source the device compiles -- for the CPU tests (tests/test_ngo3d_host.py), checked against
// goldens captured from the reference's ngo_3d_dens_model_adapter.  Compiled as HIP for the host alone and linked
// against the library for its card-file reader (srt_host::read_newray); the cross-lane stencil code is device-only and is not
// built.
#include "../../stanford_raytracer_amd/csrc/srt_ngo3d.hpp"
#include "../../stanford_raytracer_amd/csrc/srt_ngo_setup.hpp"

// modelnum 5 of `configfile`: x[n][3] -> Ns[n][4], lk[n] (the plasmapause each point was evaluated with).  0, or -1 when the
// card file cannot be read.
extern "C" int ngo3dh_density(const char *configfile, double kp, int fixed_mlt, double mlt, long n, const double *x, double *Ns,
                              double *lk) {
  srt_host::NgoConfig cfg;
  std::string err;
  if (!srt_host::read_newray(configfile, cfg, err)) return -1;
  srt::Ngo3dModel m;
  srt::ngo_fill(cfg, m.ngo);
  double z1, sinz22, N0[4];
  srt::ngo_norm_point(cfg, m.ngo, z1, sinz22);
  m.ngo.dens_core(z1, sinz22, cfg.last_latitu, N0); // readinput's normalisation, with the file's lk
  m.ngo.ane0 = m.ngo.ane0 * cfg.dsdens / (N0[0] * 1.0e-6);
  m.kp = kp;
  m.fixed_mlt = fixed_mlt;
  m.mlt = mlt;
  for (long i = 0; i < n; ++i) {
    m.dens_point(x[3 * i], x[3 * i + 1], x[3 * i + 2], Ns + 4 * i);
    lk[i] = m.lk_at(x[3 * i], x[3 * i + 1]);
  }
  return 0;
}
