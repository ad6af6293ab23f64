// srt_api_model.hpp -- a model handle's life apart from the interp grids: the constants every model carries (fill_common), the
// device copies and events (model_finish), destroy and trim, the field options (IGRF table, T04_s parameters), the srt_model_*
// getters, and the constructors of the Ngo, Ngo3d, simple3d, AT64ThCh and scattered models: a ModelPtr owns a model under
// construction and model_hand_over is every constructor's tail (the interp ones' too).  Also the scattered model's scratch
// policy, which the per-point calls (srt_api_points.hpp) and the trace launch (srt_api_trace.hpp) share.
// A part of srt_api.hip (srt_api_core.hpp).
#pragma once
#include <dlfcn.h>

#include "srt_api_core.hpp"
#include "srt_host.hpp"
#include "srt_ngo_setup.hpp"

static void fill_common(Common &cm, int nspec, const double *qs, const double *ms, int yearday, int msec) {
  memset(&cm, 0, sizeof cm);
  cm.sp.nspec = nspec;
  double maxq = 0.0, minm = 0.0;
  for (int s = 0; s < nspec; ++s) {
    cm.sp.q[s] = qs[s];
    cm.sp.m[s] = ms[s];
    cm.sp.c[s] = qs[s] * qs[s] / ms[s] / EPS0;
    cm.sp.g[s] = qs[s] / ms[s];
    if (fabs(qs[s]) > maxq) maxq = fabs(qs[s]);
    if (s == 0 || ms[s] < minm) minm = ms[s];
  }
  cm.sp.maxq2 = maxq * maxq;
  cm.sp.minm_eps0 = minm * EPS0;
  const double MU0 = PI * 4e-7; // constants.f95:6
  cm.C = sqrt(1.0 / EPS0 / MU0); // constants.f95:7
  cm.fld.yearday = yearday;
  cm.fld.msec = msec;
  double mu = srt_host::dipole_tilt(yearday, msec);
  cm.fld.cm = cos(mu);
  cm.fld.sm = sin(mu);
  cm.fld.bo_re3 = (.312 / 10000.0) * R_E * R_E * R_E;
}

static int model_finish(srt_model *m) {
  HIP_OK(m->d_common.alloc(1));
  HIP_OK(hipMemcpy(m->d_common.p, &m->cm, sizeof(Common), hipMemcpyHostToDevice));
  int rc = with_model(m, [&](auto tag) -> int {
    using M = typename decltype(tag)::Model;
    HIP_OK(m->d_model.alloc(sizeof(M)));
    HIP_OK(hipMemcpy(m->d_model.p, &m->as<M>(), sizeof(M), hipMemcpyHostToDevice));
    return SRT_OK;
  });
  if (rc) return rc;
  hipDeviceProp_t p;
  m->device = current_device();
  HIP_OK(hipGetDeviceProperties(&p, m->device));
  m->cu_count = p.multiProcessorCount;
  for (auto &sl : m->slot) HIP_OK(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
  for (auto &h : m->hist) {
    HIP_OK(hipEventCreate(&h.ev0));
    HIP_OK(hipEventCreate(&h.ev1));
    HIP_OK(h.stats.alloc(STASH_STATS));
  }
  return SRT_OK;
}

extern "C" void srt_model_destroy(srt_model *m) {
  if (!m) return;
  SRT_MODEL_SCOPE; // its tables and events live on m->device; the caller's device is back when this returns
  (void)ensure_model(m);
  for (auto &sl : m->slot) {
    sl.release();
    if (sl.done) (void)hipEventDestroy(sl.done);
  }
  for (auto &h : m->hist) {
    if (h.ev0) (void)hipEventDestroy(h.ev0);
    if (h.ev1) (void)hipEventDestroy(h.ev1);
  }
  m->io.release();
  delete m; // the tables free themselves
}
extern "C" int srt_model_trim(srt_model *m) {
  if (!m) return srt_set_error(SRT_EINVAL, "null model");
  SRT_MODEL_SCOPE;
  int rc = ensure_model(m);
  if (rc) return rc;
  std::lock_guard<std::mutex> hold(m->io_lock);
  for (auto &sl : m->slot) {
    if (sl.used) HIP_OK(hipEventSynchronize(sl.done)); // the launch that used this slot's scratch is over
    sl.release();
  }
  m->io.release();
  return SRT_OK;
}
// A model under construction: destroyed with srt_model_destroy, which takes a half-built handle (null events are skipped, empty
// DevBufs free nothing), unless model_hand_over gives it to the caller.
struct ModelDestroy {
  void operator()(srt_model *m) const { srt_model_destroy(m); }
};
using ModelPtr = std::unique_ptr<srt_model, ModelDestroy>;
static ModelPtr new_model(int kind, int nspec) {
  ModelPtr m(new srt_model);
  m->kind = kind;
  m->nspec = nspec;
  return m;
}
// every constructor's tail: the device copies and events, then what the kind needs behind them (`then`), then the handle is the
// caller's
template <class Then>
static int model_hand_over(ModelPtr &m, srt_model **out, Then &&then) {
  int rc = model_finish(m.get());
  if (rc || (rc = then(m.get()))) return rc;
  *out = m.release();
  return SRT_OK;
}
static int model_hand_over(ModelPtr &m, srt_model **out) {
  return model_hand_over(m, out, [](srt_model *) -> int { return SRT_OK; });
}
// geopack's RECALC_08 for the handle's date: coefficients, GEO->GSM matrix, the adapters' PS and geopack's own PSI
static int load_field_table(srt_model *m, const char *igrf_coeff_file) {
  FieldConst &f = m->cm.fld;
  std::string path;
  if (igrf_coeff_file && *igrf_coeff_file) path = igrf_coeff_file;
  else if (const char *e = getenv("SRT_IGRF_COEFFS")) path = e;
  else { // the table shipped beside the library: <pkg>/lib/libsrt_hip.so -> <pkg>/data/igrf_coeffs.txt
    Dl_info info;
    if (dladdr((const void *)&srt_model_set_field, &info) && info.dli_fname) {
      path = info.dli_fname;
      size_t k = path.rfind('/');
      path = (k == std::string::npos ? std::string(".") : path.substr(0, k)) + "/../data/igrf_coeffs.txt";
    }
  }
  std::string err;
  float G[105], H[105], REC[105];
  if (!srt_host::igrf_setup(path.c_str(), f.yearday, f.msec, G, H, REC, f.A, &f.psi, err, &m->geopack_psi)) return srt_set_error(SRT_EIO, "%s", err.c_str());
  igrf_pack_terms(G, H, REC, f);
  m->have_table = true;
  if (m->kind == KIND_AT64THCH) f.psi = 0.f; // the adapter's unset local (srt_at64thch.hpp, decision 2)
  return SRT_OK;
}
// device copies of the handle's constants (and of modelnum 7's struct, which holds geopack's PSI)
static int upload_constants(srt_model *m) {
  HIP_OK(hipMemcpy(m->d_common.p, &m->cm, sizeof(Common), hipMemcpyHostToDevice));
  if (m->kind == KIND_AT64THCH) {
    At64ThChModel &a = m->as<At64ThChModel>();
    a.psi = m->geopack_psi;
    a.fld = &m->d_common.p->fld;
    HIP_OK(hipMemcpy(m->d_model.p, &a, sizeof a, hipMemcpyHostToDevice));
  }
  return SRT_OK;
}
// use_igrf (raytracer_driver.f95 --use_igrf; interp_dens_model_adapter.f95:236-241 and twins)
extern "C" int srt_model_set_field(srt_model *m, int use_igrf, int use_tsyganenko, const char *igrf_coeff_file) {
  if (!m) return srt_set_error(SRT_EINVAL, "null model");
  if (use_tsyganenko != 0 && use_tsyganenko != 1) return srt_set_error(SRT_EINVAL, "use_tsyganenko must be 0 or 1");
  if (use_igrf != 0 && use_igrf != 1) return srt_set_error(SRT_EINVAL, "use_igrf must be 0 or 1");
  SRT_MODEL_SCOPE;
  int rc = ensure_model(m);
  if (rc) return rc;
  FieldConst &f = m->cm.fld;
  // both need geopack's RECALC_08 for the date: coefficients, GEO->GSM matrix, dipole tilt
  if ((use_igrf || use_tsyganenko) && (rc = load_field_table(m, igrf_coeff_file))) return rc;
  f.use_igrf = use_igrf;
  f.use_tsy = use_tsyganenko;
  return upload_constants(m);
}
// T04_s's PARMOD (driver flags --tsyganenko_Pdyn, _Dst, _ByIMF, _BzIMF, _W1 .. _W6; raytracer_driver.f95:292-341)
extern "C" int srt_model_set_tsyganenko_params(srt_model *m, const double parmod[10]) {
  if (!m || !parmod) return srt_set_error(SRT_EINVAL, "null argument");
  SRT_MODEL_SCOPE;
  int rc = ensure_model(m);
  if (rc) return rc;
  for (int i = 0; i < 10; ++i) m->cm.fld.parmod[i] = (float)parmod[i]; // real(parmod)
  m->have_parmod = true;
  return upload_constants(m);
}
extern "C" int srt_model_kind(const srt_model *m) { return m ? (m->kind == KIND_INTERP_NODES ? (int)KIND_INTERP : m->kind) : 0; }
extern "C" int srt_model_interp_layout(const srt_model *m) {
  return !m ? -1 : m->kind == KIND_INTERP ? SRT_INTERP_EXPANDED : m->kind == KIND_INTERP_NODES ? SRT_INTERP_NODES : -1;
}
extern "C" int srt_model_nspec(const srt_model *m) { return m ? m->nspec : 0; }
extern "C" const void *srt_model_device_struct(const srt_model *m) { return m ? m->d_model.p : nullptr; }
extern "C" int64_t srt_model_device_bytes(const srt_model *m) { return m ? m->device_bytes : 0; }
extern "C" int srt_model_species(const srt_model *m, double qs[SRT_MAXSPEC], double ms[SRT_MAXSPEC]) {
  if (!m) return srt_set_error(SRT_EINVAL, "null model");
  for (int s = 0; s < SRT_MAXSPEC; ++s) {
    qs[s] = s < m->nspec ? m->cm.sp.q[s] : 0.0;
    ms[s] = s < m->nspec ? m->cm.sp.m[s] : 0.0;
  }
  return SRT_OK;
}

// ---- Ngo: normalisation of ane0 (ngo_dens_model.f95:120-123) needs one evaluation of dens() -------
__global__ void ngo_norm_kernel(NgoModel g, double z1, double sinz22, double latitu, double *out) {
  double Ns[4];
  g.dens_core(z1, sinz22, latitu, Ns);
  out[0] = Ns[0] * 1.0e-6; // ani(1)
}

// readinput (ngo_dens_model.f95:29-160; ngo_3d_dens_model.f95 has the same): the card file and the normalisation of ane0
static int ngo_readinput(const char *configfile, NgoModel &g) {
  srt_host::NgoConfig cfg;
  std::string err;
  if (!srt_host::read_newray(configfile, cfg, err)) return srt_set_error(SRT_EIO, "%s: %s", configfile, err.c_str());
  ngo_fill(cfg, g);
  double z1, sinz22;
  ngo_norm_point(cfg, g, z1, sinz22);
  DevBuf<double> d_out;
  double ani1 = 0.0;
  if (d_out.alloc(1) != hipSuccess) return srt_set_error(SRT_ENOMEM, "hipMalloc failed");
  hipLaunchKernelGGL(ngo_norm_kernel, dim3(1), dim3(1), 0, 0, g, z1, sinz22, cfg.last_latitu, d_out.p);
  hipError_t e = hipMemcpy(&ani1, d_out.p, sizeof(double), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return srt_set_error(SRT_EDEVICE, "ngo normalisation kernel failed: %s", hipGetErrorString(e));
  g.ane0 = g.ane0 * cfg.dsdens / ani1;
  return SRT_OK;
}

// electrons, H+, He+, O+: the species constants of both Ngo adapters (ngo_dens_model_adapter.f95:136-138,
// ngo_3d_dens_model_adapter.f95:173-175) and of simple3d's (:813-815), with the field tail's date
static void fill_common_four_species(Common &cm, int yearday, int msec) {
  const double e_ = 1.602e-19;
  double qs[4] = {e_ * -1.0, e_, e_, e_};
  double ms[4] = {9.10938188e-31, 1.6726e-27, 4.0 * 1.6726e-27, 16.0 * 1.6726e-27};
  fill_common(cm, 4, qs, ms, yearday, msec);
}

extern "C" int srt_model_create_ngo(const char *configfile, int yearday, int msec, srt_model **out) {
  if (!configfile || !out) return srt_set_error(SRT_EINVAL, "null argument");
  DeviceScope srt_iscope_;
  int rc = srt_iscope_.enter_default();
  if (rc) return rc;
  ModelPtr m = new_model(KIND_NGO, 4);
  if ((rc = ngo_readinput(configfile, m->as<NgoModel>()))) return rc;
  fill_common_four_species(m->cm, yearday, msec);
  return model_hand_over(m, out);
}

// ---- ngo3d: the Ngo model with the plasmapause of each evaluated point from bulge(MLT, Kp) (srt_ngo3d.hpp) ------
extern "C" int srt_model_create_ngo3d(const char *configfile, double kp, int fixed_MLT, double MLT, int yearday, int msec,
                                      srt_model **out) {
  if (!configfile || !out) return srt_set_error(SRT_EINVAL, "null argument");
  if (fixed_MLT != 0 && fixed_MLT != 1) return srt_set_error(SRT_EINVAL, "fixed_MLT must be 0 or 1");
  if (!std::isfinite(kp) || (fixed_MLT == 1 && !std::isfinite(MLT))) return srt_set_error(SRT_EINVAL, "kp and MLT must be finite");
  DeviceScope srt_iscope_;
  int rc = srt_iscope_.enter_default();
  if (rc) return rc;
  ModelPtr m = new_model(KIND_NGO3D, 4);
  Ngo3dModel &g = m->as<Ngo3dModel>();
  if ((rc = ngo_readinput(configfile, g.ngo))) return rc; // ane0 is normalised with the file's lk (readinput runs once, at setup)
  g.kp = kp;
  g.fixed_mlt = fixed_MLT;
  g.mlt = MLT;
  fill_common_four_species(m->cm, yearday, msec);
  return model_hand_over(m, out);
}

// ---- simple3d: closed form, nothing but a handful of constants (srt_simple3d.hpp) -------------------
extern "C" int srt_model_create_simple3d(double kp, int fixed_MLT, double MLT, int yearday, int msec, srt_model **out) {
  if (!out) return srt_set_error(SRT_EINVAL, "null argument");
  if (fixed_MLT != 0 && fixed_MLT != 1) return srt_set_error(SRT_EINVAL, "fixed_MLT must be 0 or 1");
  if (!std::isfinite(kp) || (fixed_MLT == 1 && !std::isfinite(MLT))) return srt_set_error(SRT_EINVAL, "kp and MLT must be finite");
  DeviceScope srt_iscope_;
  int rc = srt_iscope_.enter_default();
  if (rc) return rc;
  ModelPtr m = new_model(KIND_SIMPLE3D, 4);
  auto &c = m->as<Simple3dModel>().c;
  c.kp = kp;
  c.year = yearday / 1000; // iyear = itime(1)/1000, doy = itime(1) - iyear*1000 (:743-744)
  c.doy = yearday - c.year * 1000;
  c.fixed_mlt = fixed_MLT;
  c.mlt = MLT;
  fill_common_four_species(m->cm, yearday, msec);
  return model_hand_over(m, out);
}

// ---- at64thch: closed form around one field-line trace per point (srt_at64thch.hpp, srt_fieldline.hpp) ----------
extern "C" int srt_model_create_at64thch(int gcpm_kp, const double parmod[10], const char *igrf_coeff_file, int yearday, int msec,
                                         srt_model **out) {
  if (!out || !parmod) return srt_set_error(SRT_EINVAL, "null argument");
  for (int i = 0; i < 10; ++i)
    if (!std::isfinite(parmod[i])) return srt_set_error(SRT_EINVAL, "parmod must be finite");
  DeviceScope srt_iscope_;
  int rc = srt_iscope_.enter_default();
  if (rc) return rc;
  ModelPtr m = new_model(KIND_AT64THCH, 3);
  m->as<At64ThChModel>().gcpm_kp = gcpm_kp;
  // the adapter's own species constants (:272-273): electrons, O+, H+
  const double e_ = 1.602e-19;
  double qs[3] = {e_ * -1.0, e_, e_};
  double ms[3] = {9.10938188e-31, 16.0 * 1.6726e-27, 1.6726e-27};
  fill_common(m->cm, 3, qs, ms, yearday, msec);
  // the trace uses T04_s and IGRF whatever the field options say: the table and parmod are part of the model
  for (int i = 0; i < 10; ++i) m->cm.fld.parmod[i] = (float)parmod[i]; // real(parmod), decision 1
  m->have_parmod = true;
  if ((rc = load_field_table(m.get(), igrf_coeff_file))) return rc;
  return model_hand_over(m, out, upload_constants);
}

extern "C" int srt_model_create_scattered_file(const char *ptsfile, int yearday, int msec, double window_scale,
                                               int order, int exact, double local_window_scale, srt_model **out) {
  return srt_model_create_scattered_file_root(ptsfile, yearday, msec, window_scale, order, exact, local_window_scale, -1, out);
}

extern "C" int srt_model_create_scattered_file_root(const char *ptsfile, int yearday, int msec, double window_scale,
                                                    int order, int exact, double local_window_scale, int64_t root_sample,
                                                    srt_model **out) {
  if (!ptsfile || !out) return srt_set_error(SRT_EINVAL, "null argument");
  if (root_sample < -1) return srt_set_error(SRT_EINVAL, "root_sample must be -1 (none) or a 0-based record number");
  // orders 0..3: tabular_monomials (lsinterp_mod.f95:76-99), their own kernels; 4 and 5: generate_monomials (:114-164), one
  // cooperative path built to answer (srt_scattered.hpp gen_point); beyond: 84+ monomials, no room in a wave's LDS
  if (order < 0 || order > 5)
    return srt_set_error(SRT_EINVAL, "scattered_interp_order=%d: orders 0..5 are supported (the reference's generate_monomials orders "
                                     "N >= 6 are not built: stay on the Fortran path for them)", order);
  if (!(window_scale > 0) || !(local_window_scale > 0)) return srt_set_error(SRT_EINVAL, "window scales must be > 0");
  DeviceScope srt_iscope_;
  int rc = srt_iscope_.enter_default();
  if (rc) return rc;
  srt_host::ScatteredHost h;
  std::string err;
  // reach of the trace kernel's candidate blocks beyond the search radius (srt_scattered.hpp; SRT_SCATTERED_MARGIN overrides
  // the default for experiments; results do not depend on it beyond the order of summation)
  double bmargin = 0.125;
  if (const char *e = getenv("SRT_SCATTERED_MARGIN")) {
    const double v = atof(e);
    if (v >= 0.01 && v <= 1.0) bmargin = v;
  }
  if (!srt_host::build_scattered(ptsfile, window_scale, h, err, 1.0 + bmargin, (long long)root_sample))
    return srt_set_error(SRT_EIO, "%s: %s", ptsfile, err.c_str());
  ModelPtr m = new_model(KIND_SCATTERED, h.nspec);
  std::vector<double> xyz(3 * (size_t)h.npts);
  for (size_t i = 0; i < (size_t)h.npts; ++i)
    for (int c = 0; c < 3; ++c) xyz[(size_t)c * h.npts + i] = h.pts[8 * i + c];
  hipError_t e = m->d_pts.alloc(h.pts.size());
  if (e == hipSuccess) e = m->d_cells.alloc(h.cell_start.size());
  if (e == hipSuccess) e = m->d_xyz.alloc(xyz.size());
  if (e == hipSuccess) e = hipMemcpy(m->d_xyz.p, xyz.data(), xyz.size() * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(m->d_pts.p, h.pts.data(), h.pts.size() * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(m->d_cells.p, h.cell_start.data(), h.cell_start.size() * sizeof(int), hipMemcpyHostToDevice);
  if (e != hipSuccess)
    return srt_set_error(e == hipErrorOutOfMemory ? SRT_ENOMEM : SRT_EDEVICE, "scattered model upload: %s", hipGetErrorString(e));
  m->device_bytes = (int64_t)((h.pts.size() + xyz.size()) * sizeof(double) + h.cell_start.size() * sizeof(int));
  ScatteredModel &s = m->as<ScatteredModel>();
  s.pts = m->d_pts.p;
  s.xyz = m->d_xyz.p;
  s.cell_start = m->d_cells.p;
  for (int k = 0; k < 3; ++k) {
    s.origin[k] = h.origin[k];
    s.dims[k] = h.dims[k];
  }
  s.inv_cell = h.inv_cell;
  s.radius = h.radius;
  s.lws = local_window_scale;
  s.bmargin = bmargin;
  s.u11 = 1.1 * std::pow(h.radius * (1.0 + 5.0e-16), 1.1);
  s.inv_radius = 1.0 / h.radius;
  s.nspec = h.nspec;
  s.order = order;
  s.exact = exact;
  s.npts = h.npts;
  fill_common(m->cm, h.nspec, h.qs, h.ms, yearday, msec);
  return model_hand_over(m, out);
}

// a scratch allocation of the scattered model was refused: say so ONCE per model (the launch still runs -- without staging
// every stencil takes the own-list path, without blocks every stencil scans its cells -- only slower), and do not try that
// size again at every launch (Scratch::failed; srt_model_trim forgets it)
static void scratch_refused(srt_model *m, const char *what, size_t bytes) {
  if (m->warned_scratch) return;
  m->warned_scratch = true;
  fprintf(stderr, "libsrt_hip: hipMalloc of %.2f GB for %s was refused; tracing without them (slower). "
                  "srt_model_trim() on this or other models releases launch scratch.\n", (double)bytes / 1e9, what);
}
// SRT_SCATTERED_STAGING=0 in the environment: no staging buffer, i.e. the own-list path for every stencil (tests hold
// the two paths against each other)
static bool staging_enabled() {
  const char *e = getenv("SRT_SCATTERED_STAGING");
  return !(e && e[0] == '0');
}

// SRT_SCATTERED_BLOCKS=0: no candidate blocks, i.e. every shared-path stencil of the trace kernel scans the cells (A/B, tests)
static bool blocks_enabled() {
  const char *e = getenv("SRT_SCATTERED_BLOCKS");
  return !(e && e[0] == '0');
}

// scattered model: staging records for the one-wave blocks serving n items (srt_scattered.hpp shared_fit); beyond
// 4096 blocks (2 GiB) the kernels run without (own-list path)
static void stage_alloc(DevBuf<double> &b, int64_t n) {
  const int64_t blocks = (n + WAVE - 1) / WAVE;
  if (!staging_enabled() || blocks > 4096 || b.alloc((size_t)blocks * ScatteredModel::REC_CAP * ScatteredModel::REC) != hipSuccess)
    (void)hipGetLastError();
}
