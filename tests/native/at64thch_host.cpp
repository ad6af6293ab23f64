// Host build of modelnum 7 -- stanford_raytracer_amd/csrc/srt_fieldline.hpp (the tracer) and srt_at64thch.hpp (the model around
// it), the very source the device compiles, with T04_s from srt_t04.hpp and a plain one-point IGRF loop -- for the CPU tests
// (tests/test_at64thch_host.py), checked against goldens captured from the reference's AT64ThCh_adapter and geopack's TRACE_08.
// Compiled as HIP for the host alone and linked against the library for the date's constants (srt_host::igrf_setup,
// srt_host::dipole_tilt).
#include <cmath>
#include <cstring>
#include <string>

#include "../../stanford_raytracer_amd/csrc/srt_at64thch.hpp"
#include "../../stanford_raytracer_amd/csrc/srt_host.hpp"

namespace {
struct Handle {
  srt::FieldConst f;
  srt::At64ThChModel m;
};
} // namespace

// the constants of a handle as srt_model_create_at64thch + srt_model_set_field leave them; NULL when the table cannot be read
extern "C" void *at64h_create(const char *coeff_file, int yearday, int msec, int gcpm_kp, const double *parmod, int use_igrf) {
  Handle *h = new Handle;
  memset(&h->f, 0, sizeof h->f);
  const double mu = srt_host::dipole_tilt(yearday, msec);
  h->f.cm = cos(mu);
  h->f.sm = sin(mu);
  h->f.bo_re3 = (.312 / 10000.0) * srt::R_E * srt::R_E * srt::R_E;
  h->f.yearday = yearday;
  h->f.msec = msec;
  h->f.use_igrf = use_igrf;
  std::string err;
  float G[105], H[105], REC[105], st0, psi;
  if (!srt_host::igrf_setup(coeff_file, yearday, msec, G, H, REC, h->f.A, &st0, err, &psi)) {
    delete h;
    return nullptr;
  }
  srt::igrf_pack_terms(G, H, REC, h->f);
  for (int i = 0; i < 10; ++i) h->f.parmod[i] = (float)parmod[i];
  h->m.fld = &h->f;
  h->m.psi = psi;
  h->m.gcpm_kp = gcpm_kp;
  return h;
}
extern "C" void at64h_destroy(void *p) { delete (Handle *)p; }
extern "C" float at64h_psi(void *p) { return ((Handle *)p)->m.psi; }

// x[n][3] (SM, metres) -> Ns[n][3]
extern "C" void at64h_density(void *p, long n, const double *x, double *Ns) {
  const Handle *h = (const Handle *)p;
  for (long i = 0; i < n; ++i) {
    const srt::At64ThChModel::Dens d = h->m.dens_point(x[3 * i], x[3 * i + 1], x[3 * i + 2]);
    for (int s = 0; s < 3; ++s) Ns[3 * i + s] = d.n[s];
  }
}
// the densities of funcPlasmaParams :217-274 for a given zbrat, no trace
extern "C" void at64h_closed_form(int gcpm_kp, long n, const double *x, double zbrat, double *Ns) {
  for (long i = 0; i < n; ++i) srt::at64::plasma_density(gcpm_kp, x[3 * i], x[3 * i + 1], x[3 * i + 2], zbrat, Ns + 3 * i);
}
// TRACE_08 from x[n][3] (SM, metres) with the adapter's constants, but DSMAX and LMAX as given; out[n][6] as srt_field_line_foot
extern "C" void at64h_foot(void *p, long n, const double *x, float dsmax, int lmax, double *out) {
  const Handle *h = (const Handle *)p;
  const srt::FieldConst &f = h->f;
  srt::fl::TraceConst c = srt::at64::trace_const();
  c.dsmax = dsmax;
  c.lmax = lmax;
  const srt::at64::HostField field{&f, h->m.psi};
  for (long i = 0; i < n; ++i) {
    const double px = x[3 * i], py = x[3 * i + 1], pz = x[3 * i + 2];
    const float xg = (float)((px * f.cm - pz * f.sm) / srt::R_E), yg = (float)(py / srt::R_E), zg = (float)((pz * f.cm + px * f.sm) / srt::R_E);
    const srt::fl::Foot ft = srt::fl::trace(field, c, xg, yg, zg, true);
    float bx, by, bz;
    srt::at64::igrf_point(f, ft.x, ft.y, ft.z, bx, by, bz);
    double *o = out + 6 * i;
    o[0] = ft.x;
    o[1] = ft.y;
    o[2] = ft.z;
    o[3] = sqrtf(bx * bx + by * by + bz * bz);
    o[4] = ft.kind;
    o[5] = ft.npts;
  }
}
