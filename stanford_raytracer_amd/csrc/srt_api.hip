// srt_api.hip -- C ABI (include/srt.h) of the MI355X-native many-ray Haselgrove integrator.
// Host side: model construction (device-resident tables), kernel launches, HIP-event timing.
// There is no CPU fallback: every entry point fails with SRT_EDEVICE when no GPU is usable.
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <tuple>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/srt.h"
#include "srt_host.hpp"
#include "srt_kernels.hpp"
#include "srt_ngo_setup.hpp"
#include "srt_scattered.hpp"
#include "srt_interp_nodes.hpp"
#include "srt_simple3d.hpp"
#include "srt_at64thch.hpp"
#include "srt_sampler.hpp"
#include "srt_damping.hpp"
#include "srt_xform.hpp"
#include "srt_crossings.hpp"
#include "srt_binning.hpp"
#include "srt_approaches.hpp"
#include <hipcub/hipcub.hpp>

using namespace srt;

// ------------------------------------------------------------------------------------------ errors
static thread_local std::string g_err;
int srt_set_error(int code, const char *fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
extern "C" const char *srt_last_error(void) { return g_err.c_str(); }

#define HIP_OK(expr)                                                                          \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess)                                                                     \
      return srt_set_error(e_ == hipErrorOutOfMemory ? SRT_ENOMEM : SRT_EDEVICE, "%s: %s", #expr, \
                           hipGetErrorString(e_));                                            \
  } while (0)

// The one owner of device memory in this file: an array of T that frees itself.  alloc() is exact and drops what was held first;
// reserve() only ever grows, with room to spare, and keeps the first `keep` elements (the sampler's pools).
template <class T>
struct DevBuf {
  T *p = nullptr;
  size_t cap = 0; // elements
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  hipError_t alloc(size_t n) {
    release();
    const hipError_t e = hipMalloc(&p, n * sizeof(T));
    if (e == hipSuccess) cap = n;
    else p = nullptr;
    return e;
  }
  int reserve(size_t n, size_t keep = 0) {
    if (n <= cap) return 0;
    const size_t want = n + n / 2 + 4096;
    T *q = nullptr;
    if (hipMalloc(&q, want * sizeof(T)) != hipSuccess) return -1;
    if (p && keep && hipMemcpy(q, p, keep * sizeof(T), hipMemcpyDeviceToDevice) != hipSuccess) {
      (void)hipFree(q);
      return -1;
    }
    release();
    p = q;
    cap = want;
    return 0;
  }
  void swap(DevBuf &o) {
    std::swap(p, o.p);
    std::swap(cap, o.cap);
  }
  template <class U> U *as() const { return (U *)p; }
};
using DevBytes = DevBuf<char>;

// Device selection.  srt_init(device) binds the CALLING THREAD to a device (and makes it the process default for
// threads that never called srt_init): one host thread per GPU may drive its own models concurrently (the CLI's
// --devices=0,1,..).  A model remembers the device it was created on, and every entry point that takes a model
// switches to that device first, whichever thread calls it.
static std::atomic<int> g_default_device{-1};
static thread_local int t_device = -1;
extern "C" int srt_init(int device) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
    return srt_set_error(SRT_EDEVICE, "no HIP device available (this library has no CPU path)");
  if (device < 0 || device >= n) return srt_set_error(SRT_EINVAL, "device %d out of range (%d devices)", device, n);
  HIP_OK(hipSetDevice(device));
  t_device = device;
  g_default_device.store(device);
  return SRT_OK;
}
// the device the calling thread is bound to right now (srt_init's, or a DeviceScope's)
static int current_device() {
  int d = -1;
  if (hipGetDevice(&d) != hipSuccess) {
    (void)hipGetLastError();
    d = t_device >= 0 ? t_device : 0;
  }
  return d;
}
// An entry point that works on a model (or on buffers that live on some device) binds the calling thread to THAT device
// for its own duration only: the thread's srt_init() binding (t_device) and whatever device the caller's own HIP / torch
// code had selected are back in place when the call returns.
struct DeviceScope {
  int prev = -1;
  int enter(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) {
      prev = -1;
      (void)hipGetLastError();
    }
    if (hipSetDevice(dev) != hipSuccess) return srt_set_error(SRT_EDEVICE, "hipSetDevice(%d) failed", dev);
    return SRT_OK;
  }
  // entry points without a model: the thread's srt_init() device (the process default for threads that never called it;
  // device 0 when nobody did), for the duration of the call only
  int enter_default() {
    int dev = t_device >= 0 ? t_device : g_default_device.load();
    if (dev < 0) {
      int rc = srt_init(0);
      if (rc) return rc;
      dev = 0;
    }
    return enter(dev);
  }
  ~DeviceScope() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};
// the one device that owns every (non-null) buffer of a device-buffer entry point; -1 + error if one is not device memory or
// they live on different devices
static int device_of(const char *who, const void *const *ptrs, int n, int *dev_out) {
  int dev = -1;
  for (int i = 0; i < n; ++i) {
    const void *q = ptrs[i];
    if (!q) continue;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, q) != hipSuccess || at.type != hipMemoryTypeDevice) {
      (void)hipGetLastError();
      return srt_set_error(SRT_EINVAL, "%s: %p is not device memory", who, q);
    }
    if (dev < 0) dev = at.device;
    else if (at.device != dev) return srt_set_error(SRT_EINVAL, "%s: buffers live on devices %d and %d", who, dev, at.device);
  }
  *dev_out = dev;
  return SRT_OK;
}
extern "C" int srt_device_info(char *name, int name_len, int *cu_count, int64_t *hbm_bytes) {
  DeviceScope srt_iscope_;
  int rc = srt_iscope_.enter_default();
  if (rc) return rc;
  hipDeviceProp_t p;
  HIP_OK(hipGetDeviceProperties(&p, current_device()));
  if (name && name_len > 0) snprintf(name, name_len, "%s (%s)", p.name, p.gcnArchName);
  if (cu_count) *cu_count = p.multiProcessorCount;
  if (hbm_bytes) *hbm_bytes = (int64_t)p.totalGlobalMem;
  return SRT_OK;
}

// ------------------------------------------------------------------------------------------ model
enum ModelKind { KIND_NGO = 1, KIND_INTERP = 3, KIND_SCATTERED = 4, KIND_NGO3D = 5, KIND_SIMPLE3D = 6, KIND_AT64THCH = 7, // the driver's modelnum
                 KIND_INTERP_NODES = 30 }; // internal: modelnum 3 in its node-table layout (srt_model_kind answers 3)

struct srt_model {
  int kind = 0, nspec = 0;
  int device = current_device(); // the HIP device the tables live on (the creating thread's)
  Common cm{};
  // what srt_field_line_foot (and modelnum 7's trace) needs beyond Common: has the coefficient table been loaded, has parmod been
  // set, and geopack's own PSI for the table's date (srt_host::igrf_setup)
  bool have_table = false, have_parmod = false;
  float geopack_psi = 0.f;
  std::tuple<NgoModel, InterpModel, ScatteredModel, Ngo3dModel, Simple3dModel, At64ThChModel, InterpNodesModel> host{}; // the host copy of `kind`'s struct
  template <class M> M &as() { return std::get<M>(host); }
  DevBuf<double> d_pts;
  DevBuf<double> d_xyz; // scattered model: the sample positions once more, SoA [3][npts] (the candidate scans read only these)
  DevBuf<int> d_cells;
  DevBuf<double> d_coef;
  DevBuf<InterpModel> d_axes; // node-table layout: the axes in InterpModel's form (no table), for ray_keys_kernel
  DevBytes d_model; // device copy of the host struct (kernels read it through scalar loads)
  template <class M> const M *on_device() const { return (const M *)d_model.p; }
  // Allocated ONCE, in model_finish, and never reallocated: modelnum 7's struct holds a device pointer into it
  // (At64ThChModel::fld = &d_common.p->fld, set by upload_constants).  Whoever reallocates it, or copies a handle, has to call
  // upload_constants again.
  DevBuf<Common> d_common;
  int64_t device_bytes = 0;
  int cu_count = 256;
  // scattered model (grow-only): scratch for the one-wave blocks of a launch, so many doubles per block
  struct Scratch {
    DevBuf<double> buf;
    long long blocks = 0, failed = 0; // (failed: the grid size whose allocation was refused -- not retried per launch)
  };
  // Per-launch scratch in NSLOT slots, so that launches on different streams may overlap.  A launch takes a slot whose previous
  // launch has FINISHED (its `done` event has fired) before it opens a new one: a caller that launches from one stream, one
  // launch after the other, lives in a single slot (scattered model: 9.7 GB of candidate blocks + staging per slot at grid 2048),
  // and only launches that really overlap occupy more.  When every slot is busy the next one in turn is waited for.
  struct LaunchSlot {
    hipEvent_t done = nullptr; // recorded behind the launch that used this slot's scratch last
    bool used = false;
    // ray_order option (grow-only): keys in/out, ids in/out, radix-sort workspace
    DevBuf<unsigned> keys[2];
    DevBuf<int> ids[2];
    DevBytes sorttmp;
    Scratch stage; // staging records of coop_stencil, REC_CAP * REC doubles per block
    Scratch cand;  // the lanes' candidate blocks, BLOCK_DOUBLES per block
    // frees the scratch and forgets refused sizes; the caller has waited for `done` where a launch may still read it
    void release() {
      for (int k = 0; k < 2; ++k) {
        keys[k].release();
        ids[k].release();
      }
      sorttmp.release();
      stage.buf.release();
      cand.buf.release();
      stage.blocks = stage.failed = cand.blocks = cand.failed = 0;
    }
  };
  static constexpr int NSLOT = 4;
  LaunchSlot slot[NSLOT];
  int rr_slot = 0;
  // timing history of the last NHIST launches (srt_last_kernel_ms, srt_launch_ms), its own ring: slots are reused out of turn
  struct LaunchTimes {
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool used = false;
  };
  static constexpr int NHIST = 4;
  LaunchTimes hist[NHIST];
  int next_hist = 0, last_hist = -1;
  bool warned_scratch = false;
  // device staging of the host-buffer entry point srt_trace_batch (grow-only, freed with the model): the CLI calls it
  // once per chunk of the ray file, and a fresh hipMalloc / hipFree of gigabytes per call costs as much as a small launch
  struct HostIO {
    DevBytes buf[9];
    void release() {
      for (auto &b : buf) b.release();
    }
  } io;
  std::mutex io_lock; // one srt_trace_batch (host-buffer call) per model at a time: the staging above is shared
};
static int io_reserve(srt_model *m, int k, size_t bytes, void **out) {
  DevBytes &b = m->io.buf[k];
  if (bytes > b.cap && b.alloc(bytes) != hipSuccess) {
    (void)hipGetLastError();
    return srt_set_error(SRT_ENOMEM, "hipMalloc of %zu bytes failed", bytes);
  }
  *out = b.p;
  return SRT_OK;
}

template <class K, class... Args>
static void launch_wave_blocks(K kernel, long long n, hipStream_t st, Args... args) {
  long long blocks = (n + WAVE - 1) / WAVE;
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(WAVE), 0, st, args...);
}

// The one place that turns a kind number into a type: f is a generic callable and gets a ModelTag -- the model's struct, whether
// its lookups use the wave's LDS tile, and how many one-wave blocks per CU the persistent grid of its trace launch has (interp:
// 34 KiB of LDS per wave, 512 registers per lane: one wave per SIMD; scattered: 18.5 KiB, <= 256 registers: WAVES_PER_EU per
// SIMD; ngo3d, simple3d and at64thch: as Ngo, whose integrator fills the default WaveBudget whatever the density body needs;
// the interp model's node-table layout: no LDS, a lane's gathered values and coefficients in registers, 512 of them: one wave
// per SIMD).
template <class M, bool LDS, int WAVES_PER_CU>
struct ModelTag {
  using Model = M;
  static constexpr bool lds = LDS;
  static constexpr int waves_per_cu = WAVES_PER_CU;
};
template <class F>
static int with_model(const srt_model *m, F &&f) {
  switch (m->kind) {
  case KIND_NGO: return f(ModelTag<NgoModel, false, 8>{});
  case KIND_INTERP: return f(ModelTag<InterpModel, true, 4>{});
  case KIND_SCATTERED: return f(ModelTag<ScatteredModel, true, 4 * ScatteredModel::WAVES_PER_EU>{});
  case KIND_NGO3D: return f(ModelTag<Ngo3dModel, false, 8>{});
  case KIND_SIMPLE3D: return f(ModelTag<Simple3dModel, false, 8>{});
  case KIND_AT64THCH: return f(ModelTag<At64ThChModel, false, 8>{});
  case KIND_INTERP_NODES: return f(ModelTag<InterpNodesModel, false, 4>{});
  }
  return srt_set_error(SRT_EINVAL, "model kind %d unsupported", m->kind);
}

// switch the calling thread to the model's device until the enclosing entry point returns
#define ensure_model(m) (srt_dscope_.enter((m)->device))
#define SRT_MODEL_SCOPE DeviceScope srt_dscope_

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

// species constants of both Ngo adapters (ngo_dens_model_adapter.f95:136-138, ngo_3d_dens_model_adapter.f95:173-175), the
// field tail's date, and the device copies
static int ngo_finish(srt_model *m, int yearday, int msec, srt_model **out) {
  const double e_ = 1.602e-19;
  double qs[4] = {e_ * -1.0, e_, e_, e_};
  double ms[4] = {9.10938188e-31, 1.6726e-27, 4.0 * 1.6726e-27, 16.0 * 1.6726e-27};
  fill_common(m->cm, 4, qs, ms, yearday, msec);
  const int rc = model_finish(m);
  if (rc) {
    srt_model_destroy(m);
    return rc;
  }
  *out = m;
  return SRT_OK;
}

extern "C" int srt_model_create_ngo(const char *configfile, int yearday, int msec, srt_model **out) {
  if (!configfile || !out) return srt_set_error(SRT_EINVAL, "null argument");
  DeviceScope srt_iscope_;
  int rc = srt_iscope_.enter_default();
  if (rc) return rc;
  srt_model *m = new srt_model;
  m->kind = KIND_NGO;
  m->nspec = 4;
  rc = ngo_readinput(configfile, m->as<NgoModel>());
  if (rc) {
    delete m;
    return rc;
  }
  return ngo_finish(m, yearday, msec, out);
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
  srt_model *m = new srt_model;
  m->kind = KIND_NGO3D;
  m->nspec = 4;
  Ngo3dModel &g = m->as<Ngo3dModel>();
  rc = ngo_readinput(configfile, g.ngo); // ane0 is normalised with the file's lk (readinput runs once, at setup)
  if (rc) {
    delete m;
    return rc;
  }
  g.kp = kp;
  g.fixed_mlt = fixed_MLT;
  g.mlt = MLT;
  return ngo_finish(m, yearday, msec, out);
}

// ---- simple3d: closed form, nothing but a handful of constants (srt_simple3d.hpp) -------------------
extern "C" int srt_model_create_simple3d(double kp, int fixed_MLT, double MLT, int yearday, int msec, srt_model **out) {
  if (!out) return srt_set_error(SRT_EINVAL, "null argument");
  if (fixed_MLT != 0 && fixed_MLT != 1) return srt_set_error(SRT_EINVAL, "fixed_MLT must be 0 or 1");
  if (!std::isfinite(kp) || (fixed_MLT == 1 && !std::isfinite(MLT))) return srt_set_error(SRT_EINVAL, "kp and MLT must be finite");
  DeviceScope srt_iscope_;
  int rc = srt_iscope_.enter_default();
  if (rc) return rc;
  srt_model *m = new srt_model;
  m->kind = KIND_SIMPLE3D;
  m->nspec = 4;
  auto &c = m->as<Simple3dModel>().c;
  c.kp = kp;
  c.year = yearday / 1000; // iyear = itime(1)/1000, doy = itime(1) - iyear*1000 (:743-744)
  c.doy = yearday - c.year * 1000;
  c.fixed_mlt = fixed_MLT;
  c.mlt = MLT;
  // the adapter's own species constants (:813-815)
  const double e_ = 1.602e-19;
  double qs[4] = {e_ * -1.0, e_, e_, e_};
  double ms[4] = {9.10938188e-31, 1.6726e-27, 4.0 * 1.6726e-27, 16.0 * 1.6726e-27};
  fill_common(m->cm, 4, qs, ms, yearday, msec);
  rc = model_finish(m);
  if (rc) {
    srt_model_destroy(m);
    return rc;
  }
  *out = m;
  return SRT_OK;
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
  srt_model *m = new srt_model;
  m->kind = KIND_AT64THCH;
  m->nspec = 3;
  m->as<At64ThChModel>().gcpm_kp = gcpm_kp;
  // the adapter's own species constants (:272-273): electrons, O+, H+
  const double e_ = 1.602e-19;
  double qs[3] = {e_ * -1.0, e_, e_};
  double ms[3] = {9.10938188e-31, 16.0 * 1.6726e-27, 1.6726e-27};
  fill_common(m->cm, 3, qs, ms, yearday, msec);
  // the trace uses T04_s and IGRF whatever the field options say: the table and parmod are part of the model
  for (int i = 0; i < 10; ++i) m->cm.fld.parmod[i] = (float)parmod[i]; // real(parmod), decision 1
  m->have_parmod = true;
  if ((rc = load_field_table(m, igrf_coeff_file)) || (rc = model_finish(m)) || (rc = upload_constants(m))) {
    srt_model_destroy(m);
    return rc;
  }
  *out = m;
  return SRT_OK;
}

// ---- interp: finite-difference derivatives + coefficient expansion on the device --------------------
struct GridDims {
  int nspec, nx, ny, nz;
};
__device__ __forceinline__ size_t gidx(const GridDims &g, int s, int i, int j, int k) {
  return (((size_t)k * g.ny + j) * g.nx + i) * g.nspec + s;
}
// tricubic_compute_finite_difference_derivatives, one axis (libtricubic.f95:736-790)
__global__ void fd_axis_kernel(GridDims g, const double *src, double *dst, int axis, double h) {
  size_t total = (size_t)g.nspec * g.nx * g.ny * g.nz;
  for (size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (size_t)gridDim.x * blockDim.x) {
    int s = (int)(id % g.nspec);
    size_t r = id / g.nspec;
    int i = (int)(r % g.nx);
    r /= g.nx;
    int j = (int)(r % g.ny);
    int k = (int)(r / g.ny);
    int c[3] = {i, j, k};
    int n[3] = {g.nx, g.ny, g.nz};
    int lo[3] = {i, j, k}, hi[3] = {i, j, k};
    int a = c[axis], na = n[axis];
    double v;
    if (a == 0) {
      hi[axis] = 1;
      v = (src[gidx(g, s, hi[0], hi[1], hi[2])] - src[gidx(g, s, lo[0], lo[1], lo[2])]) / h;
    } else if (a == na - 1) {
      lo[axis] = na - 2;
      v = (src[gidx(g, s, hi[0], hi[1], hi[2])] - src[gidx(g, s, lo[0], lo[1], lo[2])]) / h;
    } else {
      lo[axis] = a - 1;
      hi[axis] = a + 1;
      v = (src[gidx(g, s, hi[0], hi[1], hi[2])] - src[gidx(g, s, lo[0], lo[1], lo[2])]) / 2.0 / h;
    }
    dst[id] = v;
  }
}

struct ArrPtrs {
  const double *a[8];
};
__constant__ short c_tri_ptr[65];
__constant__ signed char c_tri_col[TRI_NNZ];
__constant__ signed char c_tri_val[TRI_NNZ];

// tricubic_get_coeff for every cell (libtricubic.f95:638-656,715-720) with the corner gathering,
// clamping and sticky derivative-zeroing flags of tricubic_interpolate_at (:859-921; SURVEY A-7).
// One 64-thread block per (cell, species): thread t first gathers constraint b[t] (t = 8*family +
// corner), then computes coefficient row t of the sparse 64x64 product.
__global__ __launch_bounds__(64) void build_coeffs_kernel(GridDims g, ArrPtrs arrs, double dx, double dy, double dz,
                                                          double *coef, long long npairs) {
  __shared__ double b[64];
  const int t = threadIdx.x;
  const int q = t >> 3, l = t & 7;
  for (long long pair = blockIdx.x; pair < npairs; pair += gridDim.x) {
    long long cell = pair / g.nspec;
    int s = (int)(pair % g.nspec);
    int ci = (int)(cell % (g.nx + 1));
    long long r = cell / (g.nx + 1);
    int cj = (int)(r % (g.ny + 1));
    int ck = (int)(r / (g.ny + 1));
    int it = ci + (l & 1), jt = cj + ((l >> 1) & 1), kt = ck + (l >> 2); // 1-based corner indices
    it = it < 1 ? 1 : (it > g.nx ? g.nx : it);
    jt = jt < 1 ? 1 : (jt > g.ny ? g.ny : jt);
    kt = kt < 1 ? 1 : (kt > g.nz ? g.nz : kt);
    // flags are set by the first clamped corner and never reset inside the corner loop
    bool fi = (ci == 0) || (ci == g.nx && l >= 1);
    bool fj = (cj == 0) || (cj == g.ny && l >= 2);
    bool fk = (ck == 0) || (ck == g.nz && l >= 4);
    double v = arrs.a[q][gidx(g, s, it - 1, jt - 1, kt - 1)];
    bool zero = false;
    switch (q) {
    case 1: v = v * dx; zero = fi; break;
    case 2: v = v * dy; zero = fj; break;
    case 3: v = v * dz; zero = fk; break;
    case 4: v = v * dx * dy; zero = fi || fj; break;
    case 5: v = v * dx * dz; zero = fi || fk; break;
    case 6: v = v * dy * dz; zero = fj || fk; break;
    case 7: v = v * dx * dy * dz; zero = fi || fj || fk; break;
    default: break;
    }
    __syncthreads();
    b[t] = zero ? 0.0 : v;
    __syncthreads();
    double acc = 0.0;
    for (int e = c_tri_ptr[t]; e < c_tri_ptr[t + 1]; ++e) acc = tri_term(acc, c_tri_val[e], b[(int)c_tri_col[e]]);
    coef[(size_t)pair * 64 + t] = acc;
  }
}

// The node table of the second layout (srt_interp_nodes.hpp): nodes[node][species][8] = the eight constraint families of
// build_coeffs_kernel, scaled by the spacings with its left-to-right products, so the stored bits are the bits it forms.
// One thread per (node, species); the arrays and the table are indexed alike (gidx).
__global__ void build_nodes_kernel(ArrPtrs arrs, double dx, double dy, double dz, double *nodes, size_t n) {
  for (size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x; id < n; id += (size_t)gridDim.x * blockDim.x) {
    double v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = arrs.a[q][id];
    v[1] = v[1] * dx;
    v[2] = v[2] * dy;
    v[3] = v[3] * dz;
    v[4] = v[4] * dx * dy;
    v[5] = v[5] * dx * dz;
    v[6] = v[6] * dy * dz;
    v[7] = v[7] * dx * dy * dz;
#pragma unroll
    for (int q = 0; q < 8; ++q) nodes[id * 8 + q] = v[q];
  }
}

// ---- the two layouts of modelnum 3: sizes, and the choice SRT_INTERP_AUTO makes (pure host code) ----
static bool layout_known(int layout) { return layout == SRT_INTERP_EXPANDED || layout == SRT_INTERP_NODES || layout == SRT_INTERP_AUTO; }
static int layout_unknown(const char *who, int layout) {
  return srt_set_error(SRT_EINVAL, "%s: unknown layout %d (SRT_INTERP_EXPANDED 0, SRT_INTERP_NODES 1, SRT_INTERP_AUTO 2)", who, layout);
}
extern "C" int srt_interp_layout_bytes(int nspec, int nx, int ny, int nz, int layout, int64_t *table, int64_t *peak) {
  if (layout != SRT_INTERP_EXPANDED && layout != SRT_INTERP_NODES)
    return srt_set_error(SRT_EINVAL, "srt_interp_layout_bytes: layout %d is neither SRT_INTERP_EXPANDED nor SRT_INTERP_NODES", layout);
  if (nspec < 1 || nspec > SRT_MAXSPEC || nx < 2 || ny < 2 || nz < 2) return srt_set_error(SRT_EINVAL, "srt_interp_layout_bytes: bad grid");
  const int64_t n = (int64_t)nx * ny * nz * nspec; // values per grid array
  const int64_t t = layout == SRT_INTERP_EXPANDED ? (int64_t)(nx + 1) * (ny + 1) * (nz + 1) * nspec * 64 * 8 : n * 64;
  if (table) *table = t;
  if (peak) *peak = t + 8 * n * 8; // creation holds the eight grid arrays and the table at the same time
  return SRT_OK;
}
extern "C" int srt_interp_layout_choose(int nspec, int nx, int ny, int nz, int64_t free_bytes) {
  int64_t t, pk;
  int rc = srt_interp_layout_bytes(nspec, nx, ny, nz, SRT_INTERP_EXPANDED, &t, &pk);
  if (rc) return rc;
  if (pk <= free_bytes) return SRT_INTERP_EXPANDED;
  if ((rc = srt_interp_layout_bytes(nspec, nx, ny, nz, SRT_INTERP_NODES, &t, &pk))) return rc;
  if (pk <= free_bytes) return SRT_INTERP_NODES;
  return srt_set_error(SRT_ENOMEM, "interp model %dx%dx%d, %d species: the node table needs %lld bytes at creation, %lld are free", nx,
                       ny, nz, nspec, (long long)pk, (long long)free_bytes);
}
// SRT_INTERP_AUTO -> the layout that fits the current device's free memory (or an error); the others pass through
static int resolve_layout(int nspec, int nx, int ny, int nz, int layout, int *out) {
  *out = layout;
  if (layout != SRT_INTERP_AUTO) return SRT_OK;
  size_t fr = 0, tot = 0;
  HIP_OK(hipMemGetInfo(&fr, &tot));
  const int c = srt_interp_layout_choose(nspec, nx, ny, nz, (int64_t)fr);
  if (c < 0) return c;
  *out = c;
  return SRT_OK;
}

// FD derivatives (unless given) + coefficient expansion (or the node table: `layout`, SRT_INTERP_EXPANDED or _NODES) + model
// object, from the 8 arrays already on the device.
// arr[0] = F; arr[1..7] = derivative blocks (contents ignored when !have_derivs).  The arrays are freed here, before the model
// is made.
static int interp_from_device_arrays(int nspec, int nx, int ny, int nz, const double bounds[6], const double *qs,
                                     const double *ms, DevBuf<double> (&arr)[8], bool have_derivs, int yearday, int msec,
                                     srt_model **out, int layout = SRT_INTERP_EXPANDED) {
  const size_t nnode = (size_t)nx * ny * nz, n = nnode * nspec;
  const size_t ncell = (size_t)(nx + 1) * (ny + 1) * (nz + 1);
  GridDims g{nspec, nx, ny, nz};
  // interp_dens_model_adapter.f95:87-89
  double dx = (bounds[1] - bounds[0]) / (nx - 1.0);
  double dy = (bounds[3] - bounds[2]) / (ny - 1.0);
  double dz = (bounds[5] - bounds[4]) / (nz - 1.0);
  DevBuf<double> coef;
  hipError_t e = hipSuccess;
  if (!have_derivs) {
    for (int a = 1; a < 8 && e == hipSuccess; ++a) e = hipMemset(arr[a].p, 0, n * sizeof(double));
    int blocks = (int)((n + 255) / 256 < 65535 * 4 ? (n + 255) / 256 : 65535 * 4);
    auto fd = [&](int src, int dst, int axis, double h) {
      hipLaunchKernelGGL(fd_axis_kernel, dim3(blocks), dim3(256), 0, 0, g, (const double *)arr[src].p, arr[dst].p, axis, h);
    };
    // order and guards of libtricubic.f95:736-790
    if (nx > 2) fd(0, 1, 0, dx);
    if (ny > 2) fd(0, 2, 1, dy);
    if (nz > 2) fd(0, 3, 2, dz);
    if (nx > 2 && ny > 2) fd(2, 4, 0, dx);
    if (nx > 2 && nz > 2) fd(3, 5, 0, dx);
    if (ny > 2 && nz > 2) fd(3, 6, 1, dy);
    if (nx > 2 && ny > 2 && nz > 2) fd(6, 7, 0, dx);
  }
  const bool as_nodes = layout == SRT_INTERP_NODES;
  if (e == hipSuccess) e = coef.alloc(as_nodes ? n * 8 : ncell * nspec * 64);
  if (e != hipSuccess)
    return srt_set_error(e == hipErrorOutOfMemory ? SRT_ENOMEM : SRT_EDEVICE, "interp model setup: %s", hipGetErrorString(e));
  if (as_nodes) {
    ArrPtrs ap;
    for (int a = 0; a < 8; ++a) ap.a[a] = arr[a].p;
    const int blocks = (int)((n + 255) / 256 < 65535 * 4 ? (n + 255) / 256 : 65535 * 4);
    hipLaunchKernelGGL(build_nodes_kernel, dim3(blocks), dim3(256), 0, 0, ap, dx, dy, dz, coef.p, n);
    e = hipDeviceSynchronize();
    for (auto &b : arr) b.release();
    if (e != hipSuccess) return srt_set_error(SRT_EDEVICE, "node table build failed: %s", hipGetErrorString(e));
    srt_model *m = new srt_model;
    m->kind = KIND_INTERP_NODES;
    m->nspec = nspec;
    m->d_coef.swap(coef);
    m->device_bytes = (int64_t)(n * 8 * sizeof(double));
    InterpNodesModel &nm = m->as<InterpNodesModel>();
    nm.nodes = m->d_coef.p;
    nm.nspec = nspec;
    nm.ax = Axis{bounds[0], dx, 1.0 / dx, nx};
    nm.ay = Axis{bounds[2], dy, 1.0 / dy, ny};
    nm.az = Axis{bounds[4], dz, 1.0 / dz, nz};
    // the launch-cell ray order (srt_trace_batch_device) takes its keys from the axes in InterpModel's form, on both layouts
    InterpModel &im = m->as<InterpModel>();
    im.coef = nullptr;
    im.nspec = nspec;
    im.ax = nm.ax, im.ay = nm.ay, im.az = nm.az;
    fill_common(m->cm, nspec, qs, ms, yearday, msec);
    int rc = model_finish(m);
    if (!rc && m->d_axes.alloc(1) != hipSuccess) rc = srt_set_error(SRT_ENOMEM, "hipMalloc failed");
    if (!rc && hipMemcpy(m->d_axes.p, &im, sizeof im, hipMemcpyHostToDevice) != hipSuccess)
      rc = srt_set_error(SRT_EDEVICE, "upload of the axes failed");
    if (rc) {
      srt_model_destroy(m);
      return rc;
    }
    *out = m;
    return SRT_OK;
  }
  (void)hipMemcpyToSymbol(HIP_SYMBOL(c_tri_ptr), TRI_PTR, sizeof TRI_PTR);
  (void)hipMemcpyToSymbol(HIP_SYMBOL(c_tri_col), TRI_COL, sizeof TRI_COL);
  (void)hipMemcpyToSymbol(HIP_SYMBOL(c_tri_val), TRI_VAL, sizeof TRI_VAL);
  ArrPtrs ap;
  for (int a = 0; a < 8; ++a) ap.a[a] = arr[a].p;
  long long npairs = (long long)ncell * nspec;
  int blocks = (int)(npairs < 262144 ? npairs : 262144);
  hipLaunchKernelGGL(build_coeffs_kernel, dim3(blocks), dim3(64), 0, 0, g, ap, dx, dy, dz, coef.p, npairs);
  e = hipDeviceSynchronize();
  for (auto &b : arr) b.release();
  if (e != hipSuccess) return srt_set_error(SRT_EDEVICE, "coefficient build failed: %s", hipGetErrorString(e));
  srt_model *m = new srt_model;
  m->kind = KIND_INTERP;
  m->nspec = nspec;
  m->d_coef.swap(coef);
  m->device_bytes = (int64_t)(ncell * nspec * 64 * sizeof(double));
  InterpModel &im = m->as<InterpModel>();
  im.coef = m->d_coef.p;
  im.nspec = nspec;
  im.ax = Axis{bounds[0], dx, 1.0 / dx, nx};
  im.ay = Axis{bounds[2], dy, 1.0 / dy, ny};
  im.az = Axis{bounds[4], dz, 1.0 / dz, nz};
  fill_common(m->cm, nspec, qs, ms, yearday, msec);
  int rc = model_finish(m);
  if (rc) {
    srt_model_destroy(m);
    return rc;
  }
  *out = m;
  return SRT_OK;
}

static int alloc_grid_arrays(size_t n, DevBuf<double> (&arr)[8]) {
  for (auto &b : arr)
    if (b.alloc(n) != hipSuccess)
      return srt_set_error(SRT_ENOMEM, "hipMalloc of grid arrays failed (%zu bytes each)", n * sizeof(double));
  return SRT_OK;
}

static int create_interp(int nspec, int nx, int ny, int nz, const double bounds[6], const double *qs, const double *ms,
                         const double *F, const double *const *derivs, int yearday, int msec, int layout, srt_model **out) {
  if (!bounds || !qs || !ms || !F || !out) return srt_set_error(SRT_EINVAL, "null argument");
  if (nspec < 1 || nspec > SRT_MAXSPEC)
    return srt_set_error(SRT_EINVAL, "nspec=%d unsupported (1..%d species: SRT_MAXSPEC, include/srt.h)", nspec, SRT_MAXSPEC);
  if (nx < 2 || ny < 2 || nz < 2) return srt_set_error(SRT_EINVAL, "grid must have >= 2 nodes per axis");
  DeviceScope srt_iscope_;
  int rc = srt_iscope_.enter_default();
  if (rc) return rc;
  const size_t n = (size_t)nx * ny * nz * nspec;
  if ((size_t)(nx + 1) * (ny + 1) * (nz + 1) >= (size_t)1 << 31) return srt_set_error(SRT_EINVAL, "grid too large");
  if ((rc = resolve_layout(nspec, nx, ny, nz, layout, &layout))) return rc;
  DevBuf<double> arr[8];
  rc = alloc_grid_arrays(n, arr);
  if (rc) return rc;
  hipError_t e = hipMemcpy(arr[0].p, F, n * sizeof(double), hipMemcpyHostToDevice);
  if (derivs)
    for (int a = 1; a < 8 && e == hipSuccess; ++a)
      e = hipMemcpy(arr[a].p, derivs[a - 1], n * sizeof(double), hipMemcpyHostToDevice);
  if (e != hipSuccess) return srt_set_error(SRT_EDEVICE, "grid upload: %s", hipGetErrorString(e));
  return interp_from_device_arrays(nspec, nx, ny, nz, bounds, qs, ms, arr, derivs != nullptr, yearday, msec, out, layout);
}
extern "C" int srt_model_create_interp(int nspec, int nx, int ny, int nz, const double bounds[6],
                                       const double *qs, const double *ms, const double *F,
                                       const double *const *derivs, int yearday, int msec, srt_model **out) {
  return create_interp(nspec, nx, ny, nz, bounds, qs, ms, F, derivs, yearday, msec, SRT_INTERP_EXPANDED, out);
}
extern "C" int srt_model_create_interp_layout(int nspec, int nx, int ny, int nz, const double bounds[6], const double *qs,
                                              const double *ms, const double *F, const double *const *derivs, int yearday,
                                              int msec, int layout, srt_model **out) {
  if (!layout_known(layout)) return layout_unknown("srt_model_create_interp_layout", layout);
  return create_interp(nspec, nx, ny, nz, bounds, qs, ms, F, derivs, yearday, msec, layout, out);
}

// ---- the step before the path: sample a model on a regular grid, in log space, on the device ----
// gcpm_dens_model_buildgrid.f95:160-300 with any in-scope model in place of GCPM: node coordinates
// (/ (ind) /)*del + min (:163-179), f = log(Ns) (:212-214), and, for compder = 1, the seven explicit
// finite-difference blocks with d = 1e-3*|pos| (:197-201, :219-296) in the reference's own order of operations.
struct SampleArgs {
  double min[3], del[3];
  double *a[8];
  long long nnode;
  int compder;
};
template <class M, bool USE_LDS>
__global__ __launch_bounds__(64) void sample_grid_kernel(const M *__restrict__ mp, GridDims g, SampleArgs A) {
  const M &m = *mp;
  __shared__ __attribute__((aligned(16))) double tile[USE_LDS ? TILE_DOUBLES : 2];
  const long long id = (long long)blockIdx.x * WAVE + threadIdx.x;
  const bool live = id < A.nnode;
  const long long node = live ? id : A.nnode - 1; // every lane takes part in the (cooperative) lookups
  const int i = (int)(node % g.nx), j = (int)((node / g.nx) % g.ny), k = (int)(node / ((long long)g.nx * g.ny));
  double pos[3];
  {
#pragma clang fp contract(off)
    double px = (double)i * A.del[0], py = (double)j * A.del[1], pz = (double)k * A.del[2];
    pos[0] = px + A.min[0];
    pos[1] = py + A.min[1];
    pos[2] = pz + A.min[2];
  }
  double d = 1.0e-3 * sqrt(pos[0] * pos[0] + pos[1] * pos[1] + pos[2] * pos[2]);
  if (d == 0.0) d = 1.0e-3;
  auto lnN = [&](double sx, double sy, double sz, double (&L)[4]) { // log(Ns) at (pos + sx*dx) + sy*dy) + sz*dz
    double p[1][3] = {{(pos[0] + sx * d) + 0.0, (pos[1] + 0.0) + sy * d, ((pos[2] + 0.0) + 0.0) + sz * d}};
    double Ns[1][4];
    m.template density<1>(p, Ns, tile);
#pragma unroll
    for (int s = 0; s < 4; ++s) L[s] = log(Ns[0][s]);
  };
  auto put = [&](int blk, const double (&v)[4]) {
    if (live)
      for (int s = 0; s < g.nspec; ++s) A.a[blk][(size_t)node * g.nspec + s] = v[s];
  };
  double f[4], t[4], u[4];
  lnN(0, 0, 0, f);
  put(0, f);
  if (!A.compder) return;
  // first derivatives: tmp = log(N+) ; tmp = tmp - log(N-) ; tmp = tmp/d/2
  for (int ax = 0; ax < 3; ++ax) {
    lnN(ax == 0, ax == 1, ax == 2, t);
    lnN(-(ax == 0), -(ax == 1), -(ax == 2), u);
#pragma unroll
    for (int s = 0; s < 4; ++s) t[s] = (t[s] - u[s]) / d / 2.0;
    put(1 + ax, t);
  }
  // mixed second derivatives: (+,+) - (-,+) - (+,-) + (-,-) ; /d/d/4        pairs (x,y) (x,z) (y,z)
  for (int pr = 0; pr < 3; ++pr) {
    const int a0 = pr == 2 ? 1 : 0, a1 = pr == 0 ? 1 : 2;
    double sg[3];
    auto at = [&](double s0, double s1, double (&L)[4]) {
      sg[0] = sg[1] = sg[2] = 0.0;
      sg[a0] = s0;
      sg[a1] = s1;
      lnN(sg[0], sg[1], sg[2], L);
    };
    at(1, 1, t);
    at(-1, 1, u);
#pragma unroll
    for (int s = 0; s < 4; ++s) t[s] = t[s] - u[s];
    at(1, -1, u);
#pragma unroll
    for (int s = 0; s < 4; ++s) t[s] = t[s] - u[s];
    at(-1, -1, u);
#pragma unroll
    for (int s = 0; s < 4; ++s) t[s] = (t[s] + u[s]) / d / d / 4.0;
    put(4 + pr, t);
  }
  // third derivative: +++ -(-++) -(+-+) +(--+) -(++-) +(-+-) +(+--) -(---) ; /d/d/d/8
  {
    const double sx[8] = {1, -1, 1, -1, 1, -1, 1, -1}, sy[8] = {1, 1, -1, -1, 1, 1, -1, -1}, sz[8] = {1, 1, 1, 1, -1, -1, -1, -1};
    const double sign[8] = {1, -1, -1, 1, -1, 1, 1, -1};
    lnN(sx[0], sy[0], sz[0], t);
    for (int q = 1; q < 8; ++q) {
      lnN(sx[q], sy[q], sz[q], u);
#pragma unroll
      for (int s = 0; s < 4; ++s) t[s] = sign[q] > 0 ? t[s] + u[s] : t[s] - u[s];
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) t[s] = t[s] / d / d / d / 8.0;
    put(7, t);
  }
}

// fills arr[0] (and arr[1..7] when compder) on the device
static int sample_model_on_grid(srt_model *src, int compder, int nx, int ny, int nz, const double bounds[6],
                                DevBuf<double> (&arr)[8]) {
  GridDims g{src->nspec, nx, ny, nz};
  SampleArgs A;
  // gcpm_dens_model_buildgrid.f95:161-163
  A.del[0] = (bounds[1] - bounds[0]) / (nx - 1.0);
  A.del[1] = (bounds[3] - bounds[2]) / (ny - 1.0);
  A.del[2] = (bounds[5] - bounds[4]) / (nz - 1.0);
  A.min[0] = bounds[0];
  A.min[1] = bounds[2];
  A.min[2] = bounds[4];
  for (int a = 0; a < 8; ++a) A.a[a] = arr[a].p;
  A.nnode = (long long)nx * ny * nz;
  A.compder = compder;
  const int rc = with_model(src, [&](auto tag) -> int {
    using T = decltype(tag);
    launch_wave_blocks(sample_grid_kernel<typename T::Model, T::lds>, A.nnode, 0, src->on_device<typename T::Model>(), g, A);
    return SRT_OK;
  });
  if (rc) return rc;
  hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) return srt_set_error(SRT_EDEVICE, "grid sampling failed: %s", hipGetErrorString(e));
  return SRT_OK;
}

static int check_grid_request(srt_model *src, int nx, int ny, int nz, const double bounds[6]) {
  if (!src || !bounds) return srt_set_error(SRT_EINVAL, "null argument");
  if (nx < 2 || ny < 2 || nz < 2) return srt_set_error(SRT_EINVAL, "grid must have >= 2 nodes per axis");
  if ((size_t)(nx + 1) * (ny + 1) * (nz + 1) >= (size_t)1 << 31) return srt_set_error(SRT_EINVAL, "grid too large");
  if (!(bounds[1] > bounds[0]) || !(bounds[3] > bounds[2]) || !(bounds[5] > bounds[4])) return srt_set_error(SRT_EINVAL, "empty bounds");
  return SRT_OK;
}

extern "C" int srt_build_grid(srt_model *src, int compder, int nx, int ny, int nz, const double bounds[6], double *F,
                              double *derivs) {
  int rc = check_grid_request(src, nx, ny, nz, bounds);
  if (rc) return rc;
  SRT_MODEL_SCOPE;
  if ((rc = ensure_model(src))) return rc;
  if (!F || (compder && !derivs)) return srt_set_error(SRT_EINVAL, "null output");
  const size_t n = (size_t)nx * ny * nz * src->nspec;
  DevBuf<double> arr[8];
  if ((rc = alloc_grid_arrays(n, arr)) || (rc = sample_model_on_grid(src, compder ? 1 : 0, nx, ny, nz, bounds, arr))) return rc;
  hipError_t e = hipMemcpy(F, arr[0].p, n * sizeof(double), hipMemcpyDeviceToHost);
  if (compder)
    for (int a = 1; a < 8 && e == hipSuccess; ++a)
      e = hipMemcpy(derivs + (size_t)(a - 1) * n, arr[a].p, n * sizeof(double), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return srt_set_error(SRT_EDEVICE, "grid download: %s", hipGetErrorString(e));
  return SRT_OK;
}

// ---- dumpmodel.f95: funcPlasmaParams of any model on a regular grid, in SM or MAG coordinates ----
// Three launches on one stream: the nodes' coordinates (dumpmodel.f95:219-237, and SM_TO_MAG_D for mag_coords = 1,
// :1140-1143), then the UNCHANGED params_kernel on them, then the 19 values of a node packed into the file's 4 nspec + 3.  The
// dump of a node is therefore what srt_plasma_params gives at the node's coordinates, bit for bit, by construction: the
// lookups are the same instruction stream on the same inputs (a kernel that formed the coordinates around the lookup would
// leave the compiler free to fuse other products, HISTORY.md section 22).
struct DumpArgs {
  double min[3], del[3];
  int n[3];
  int mag;
  xform::Chain chain;
};
// x[count][3] = the coordinates of nodes first .. first + count - 1 (linear index = the file's order: x fastest, then y, z)
__global__ __launch_bounds__(256) void dump_points_kernel(DumpArgs A, long long first, long long count, double *__restrict__ x) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count) return;
  const long long node = first + t;
  const int idx[3] = {(int)(node % A.n[0]), (int)((node / A.n[0]) % A.n[1]), (int)(node / ((long long)A.n[0] * A.n[1]))};
  double pos[3];
  {
#pragma clang fp contract(off)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double p = (double)idx[c] * A.del[c]; // (/ (ind) /)*del + min: a product, then a sum
      pos[c] = A.n[c] == 1 ? A.min[c] : p + A.min[c]; // one node: x = (/ minx /), del (a quotient by zero) is never read
    }
  }
  double q[3] = {pos[0], pos[1], pos[2]};
  if (A.mag) xform::apply(A.chain, pos, q);
  x[3 * t] = q[0];
  x[3 * t + 1] = q[1];
  x[3 * t + 2] = q[2];
}
// f[count][4 nspec + 3] = (qs, Ns, ms, nus, B0) from params_kernel's p[count][19] = qs(4) Ns(4) ms(4) nus(4) B0(3): the unused
// species slot of a three-species model is dropped.  One thread per output value: a block writes one contiguous run.
__global__ __launch_bounds__(256) void dump_pack_kernel(long long count, int nspec, const double *__restrict__ p, double *__restrict__ f) {
  const int per = 4 * nspec + 3;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count * per) return;
  const long long node = t / per;
  const int c = (int)(t - node * per);
  const int src = c < 4 * nspec ? 4 * (c / nspec) + c % nspec : 16 + (c - 4 * nspec);
  f[t] = p[19 * node + src];
}

extern "C" int srt_dump_model(srt_model *m, int nx, int ny, int nz, const double bounds[6], int mag_coords, double *f) {
  // every refusal by name comes before the device is touched
  if (!bounds || !f) return srt_set_error(SRT_EINVAL, "srt_dump_model: null argument");
  if (nx < 1 || ny < 1 || nz < 1) return srt_set_error(SRT_EINVAL, "srt_dump_model: nx, ny, nz = %d, %d, %d: every axis needs at least 1 node", nx, ny, nz);
  const int n3[3] = {nx, ny, nz};
  for (int c = 0; c < 3; ++c)
    if (n3[c] > 1 && !(bounds[2 * c + 1] > bounds[2 * c]))
      return srt_set_error(SRT_EINVAL, "srt_dump_model: empty bounds on the %c axis (%d nodes need max > min)", "xyz"[c], n3[c]);
  const long long nxy = (long long)nx * ny, nnode = nxy <= 2147483647ll ? nxy * nz : -1; // (either product fits 63 bits)
  if (nnode < 0 || nnode > 2147483647ll)
    return srt_set_error(SRT_EINVAL, "srt_dump_model: %d x %d x %d is more than 2^31 - 1 nodes", nx, ny, nz);
  if (mag_coords != 0 && mag_coords != 1) return srt_set_error(SRT_EINVAL, "srt_dump_model: mag_coords = %d is neither 0 (SM) nor 1 (MAG)", mag_coords);
  if (!m) return srt_set_error(SRT_EINVAL, "srt_dump_model: null model");
  SRT_MODEL_SCOPE;
  int rc = ensure_model(m);
  if (rc) return rc;
  DumpArgs A;
  memset(&A, 0, sizeof A);
  for (int c = 0; c < 3; ++c) {
    A.n[c] = n3[c];
    A.min[c] = bounds[2 * c];
    A.del[c] = n3[c] > 1 ? (bounds[2 * c + 1] - bounds[2 * c]) / (n3[c] - 1.0) : 0.0; // dumpmodel.f95:220-222
  }
  A.mag = mag_coords;
  if (mag_coords) A.chain = xform::chain(m->cm.fld.yearday, m->cm.fld.msec, false);
  const int per = 4 * m->nspec + 3;
  // the output is whole on the device; the coordinates and params_kernel's 19 values per node exist for one piece at a time
  const long long PIECE = 1ll << 20;
  const long long piece = nnode < PIECE ? nnode : PIECE;
  DevBuf<double> dx, dp19, df;
  if (df.alloc((size_t)nnode * per) != hipSuccess || dx.alloc((size_t)3 * piece) != hipSuccess || dp19.alloc((size_t)19 * piece) != hipSuccess) {
    (void)hipGetLastError();
    return srt_set_error(SRT_ENOMEM, "srt_dump_model: %lld nodes of %d values do not fit on the device", nnode, per);
  }
  srt_model::LaunchTimes &lt = m->hist[m->next_hist];
  HIP_OK(hipEventRecord(lt.ev0, 0));
  for (long long first = 0; first < nnode; first += piece) {
    const long long count = nnode - first < piece ? nnode - first : piece;
    hipLaunchKernelGGL(dump_points_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, 0, A, first, count, dx.p);
    rc = with_model(m, [&](auto tag) -> int {
      using T = decltype(tag);
      launch_wave_blocks(params_kernel<typename T::Model, T::lds>, count, 0, m->on_device<typename T::Model>(), m->d_common.p, count,
                         (const double *)dx.p, dp19.p);
      return SRT_OK;
    });
    if (rc) return rc;
    hipLaunchKernelGGL(dump_pack_kernel, dim3((unsigned)((count * per + 255) / 256)), dim3(256), 0, 0, count, m->nspec,
                       (const double *)dp19.p, df.p + (size_t)first * per);
  }
  HIP_OK(hipGetLastError());
  HIP_OK(hipEventRecord(lt.ev1, 0));
  lt.used = true;
  m->last_hist = m->next_hist;
  m->next_hist = (m->next_hist + 1) % srt_model::NHIST;
  HIP_OK(hipMemcpy(f, df.p, (size_t)nnode * per * sizeof(double), hipMemcpyDeviceToHost));
  return SRT_OK;
}

static int create_interp_from_model(srt_model *src, int compder, int nx, int ny, int nz, const double bounds[6], int yearday,
                                    int msec, int layout, srt_model **out) {
  int rc = check_grid_request(src, nx, ny, nz, bounds);
  if (rc) return rc;
  if (!out) return srt_set_error(SRT_EINVAL, "null argument");
  SRT_MODEL_SCOPE; // the new model is built beside its source, on the source's device
  if ((rc = ensure_model(src))) return rc;
  const size_t n = (size_t)nx * ny * nz * src->nspec;
  if ((rc = resolve_layout(src->nspec, nx, ny, nz, layout, &layout))) return rc;
  DevBuf<double> arr[8];
  if ((rc = alloc_grid_arrays(n, arr)) || (rc = sample_model_on_grid(src, compder ? 1 : 0, nx, ny, nz, bounds, arr))) return rc;
  return interp_from_device_arrays(src->nspec, nx, ny, nz, bounds, src->cm.sp.q, src->cm.sp.m, arr, compder != 0,
                                   yearday, msec, out, layout);
}
extern "C" int srt_model_create_interp_from_model(srt_model *src, int compder, int nx, int ny, int nz,
                                                  const double bounds[6], int yearday, int msec, srt_model **out) {
  return create_interp_from_model(src, compder, nx, ny, nz, bounds, yearday, msec, SRT_INTERP_EXPANDED, out);
}
extern "C" int srt_model_create_interp_from_model_layout(srt_model *src, int compder, int nx, int ny, int nz,
                                                         const double bounds[6], int yearday, int msec, int layout,
                                                         srt_model **out) {
  if (!layout_known(layout)) return layout_unknown("srt_model_create_interp_from_model_layout", layout);
  return create_interp_from_model(src, compder, nx, ny, nz, bounds, yearday, msec, layout, out);
}

static int create_interp_file(const char *gridfile, int yearday, int msec, int layout, srt_model **out) {
  if (!gridfile || !out) return srt_set_error(SRT_EINVAL, "null argument");
  srt_host::GridFile gf;
  std::string err;
  if (!srt_host::read_grid_file(gridfile, gf, err)) return srt_set_error(SRT_EIO, "%s: %s", gridfile, err.c_str());
  const double *dptr[7];
  for (int a = 0; a < 7; ++a) dptr[a] = gf.have_derivs ? gf.derivs[a].data() : nullptr;
  return create_interp(gf.nspec, gf.nx, gf.ny, gf.nz, gf.bounds, gf.qs, gf.ms, gf.F.data(), gf.have_derivs ? dptr : nullptr, yearday,
                       msec, layout, out);
}
extern "C" int srt_model_create_interp_file(const char *gridfile, int yearday, int msec, srt_model **out) {
  return create_interp_file(gridfile, yearday, msec, SRT_INTERP_EXPANDED, out);
}
extern "C" int srt_model_create_interp_file_layout(const char *gridfile, int yearday, int msec, int layout, srt_model **out) {
  if (!layout_known(layout)) return layout_unknown("srt_model_create_interp_file_layout", layout);
  return create_interp_file(gridfile, yearday, msec, layout, out);
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
  srt_model *m = new srt_model;
  m->kind = KIND_SCATTERED;
  m->nspec = h.nspec;
  std::vector<double> xyz(3 * (size_t)h.npts);
  for (size_t i = 0; i < (size_t)h.npts; ++i)
    for (int c = 0; c < 3; ++c) xyz[(size_t)c * h.npts + i] = h.pts[8 * i + c];
  hipError_t e = m->d_pts.alloc(h.pts.size());
  if (e == hipSuccess) e = m->d_cells.alloc(h.cell_start.size());
  if (e == hipSuccess) e = m->d_xyz.alloc(xyz.size());
  if (e == hipSuccess) e = hipMemcpy(m->d_xyz.p, xyz.data(), xyz.size() * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(m->d_pts.p, h.pts.data(), h.pts.size() * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(m->d_cells.p, h.cell_start.data(), h.cell_start.size() * sizeof(int), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    srt_model_destroy(m);
    return srt_set_error(e == hipErrorOutOfMemory ? SRT_ENOMEM : SRT_EDEVICE, "scattered model upload: %s", hipGetErrorString(e));
  }
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
  rc = model_finish(m);
  if (rc) {
    srt_model_destroy(m);
    return rc;
  }
  *out = m;
  return SRT_OK;
}

// ------------------------------------------------------------------------------------------ per-point entry points
// a scratch allocation of the scattered model was refused: say so ONCE per model (the launch still runs -- without staging
// every stencil takes the own-list path, without blocks every stencil scans its cells -- only slower), and do not try that
// size again at every launch (Scratch::failed; srt_model_trim forgets it)
static void scratch_refused(srt_model *m, const char *what, size_t bytes) {
  if (m->warned_scratch) return;
  m->warned_scratch = true;
  fprintf(stderr, "libsrt_hip: hipMalloc of %.2f GB for the scattered model's %s was refused; tracing without them (slower). "
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

static int upload(DevBuf<double> &b, const double *h, size_t n) {
  if (b.alloc(n) != hipSuccess) return srt_set_error(SRT_ENOMEM, "hipMalloc failed");
  HIP_OK(hipMemcpy(b.p, h, n * sizeof(double), hipMemcpyHostToDevice));
  return SRT_OK;
}

extern "C" int srt_plasma_params(srt_model *m, int64_t n, const double *x, double *qs, double *Ns, double *ms,
                                 double *nus, double *B0) {
  if (!m || !x || n < 0) return srt_set_error(SRT_EINVAL, "bad argument");
  if (n == 0) return SRT_OK;
  SRT_MODEL_SCOPE;
  int rc = ensure_model(m);
  if (rc) return rc;
  DevBuf<double> dx, dout;
  if ((rc = upload(dx, x, 3 * n))) return rc;
  if (dout.alloc(19 * n) != hipSuccess) return srt_set_error(SRT_ENOMEM, "hipMalloc failed");
  rc = with_model(m, [&](auto tag) -> int {
    using T = decltype(tag);
    launch_wave_blocks(params_kernel<typename T::Model, T::lds>, n, 0, m->on_device<typename T::Model>(), m->d_common.p, (long long)n,
                       dx.p, dout.p);
    return SRT_OK;
  });
  if (rc) return rc;
  std::vector<double> h(19 * n);
  HIP_OK(hipMemcpy(h.data(), dout.p, h.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (int64_t i = 0; i < n; ++i) {
    for (int s = 0; s < 4; ++s) {
      if (qs) qs[4 * i + s] = h[19 * i + s];
      if (Ns) Ns[4 * i + s] = h[19 * i + 4 + s];
      if (ms) ms[4 * i + s] = h[19 * i + 8 + s];
      if (nus) nus[4 * i + s] = h[19 * i + 12 + s];
    }
    if (B0)
      for (int c = 0; c < 3; ++c) B0[3 * i + c] = h[19 * i + 16 + c];
  }
  return SRT_OK;
}

extern "C" int srt_dispersion(srt_model *m, int64_t n, const double *x, const double *k, const double *w, double *out) {
  if (!m || !x || !k || !w || !out || n < 0) return srt_set_error(SRT_EINVAL, "bad argument");
  if (n == 0) return SRT_OK;
  SRT_MODEL_SCOPE;
  int rc = ensure_model(m);
  if (rc) return rc;
  DevBuf<double> dx, dk, dw, dout;
  if ((rc = upload(dx, x, 3 * n)) || (rc = upload(dk, k, 3 * n)) || (rc = upload(dw, w, n))) return rc;
  if (dout.alloc(10 * n) != hipSuccess) return srt_set_error(SRT_ENOMEM, "hipMalloc failed");
  rc = with_model(m, [&](auto tag) -> int {
    using T = decltype(tag);
    launch_wave_blocks(dispersion_kernel<typename T::Model, T::lds>, n, 0, m->on_device<typename T::Model>(), m->d_common.p,
                       (long long)n, dx.p, dk.p, dw.p, dout.p);
    return SRT_OK;
  });
  if (rc) return rc;
  HIP_OK(hipMemcpy(out, dout.p, 10 * n * sizeof(double), hipMemcpyDeviceToHost));
  return SRT_OK;
}

// TRACE_08, batched: one line per lane with the adapter's constants; out[n][6] = XF, YF, ZF, |IGRF| there, ending, points
__global__ __launch_bounds__(64) void foot_kernel(const Common *__restrict__ cp, float psi, long long n, const double *x, double *out) {
  const FieldConst &f = cp->fld;
  const long long i = (long long)blockIdx.x * WAVE + threadIdx.x;
  const long long j = i < n ? i : n - 1; // every lane takes part (the synthesis is wave-uniform)
  const double px = x[3 * j], py = x[3 * j + 1], pz = x[3 * j + 2];
  const float xg = (float)((px * f.cm - pz * f.sm) / R_E), yg = (float)(py / R_E), zg = (float)((pz * f.cm + px * f.sm) / R_E);
  const fl::Foot ft = at64::foot_device(f, psi, at64::trace_const(), xg, yg, zg, true);
  float bx, by, bz;
  at64::igrf1_device(f, ft.x, ft.y, ft.z, bx, by, bz);
  if (i < n) {
#pragma clang fp contract(off)
    double *o = out + 6 * i;
    o[0] = ft.x;
    o[1] = ft.y;
    o[2] = ft.z;
    o[3] = sqrtf(bx * bx + by * by + bz * bz);
    o[4] = ft.kind;
    o[5] = ft.npts;
  }
}
extern "C" int srt_field_line_foot(srt_model *m, int64_t n, const double *x, double *out) {
  if (!m || !x || !out || n < 0) return srt_set_error(SRT_EINVAL, "bad argument");
  if (!m->have_table)
    return srt_set_error(SRT_EINVAL, "srt_field_line_foot: the model has no IGRF coefficient table (srt_model_set_field with use_igrf "
                                     "or use_tsyganenko loads it)");
  if (!m->have_parmod)
    return srt_set_error(SRT_EINVAL, "srt_field_line_foot: the model has no T04_s parameters (srt_model_set_tsyganenko_params)");
  if (n == 0) return SRT_OK;
  SRT_MODEL_SCOPE;
  int rc = ensure_model(m);
  if (rc) return rc;
  DevBuf<double> dx, dout;
  if ((rc = upload(dx, x, 3 * n))) return rc;
  if (dout.alloc(6 * n) != hipSuccess) return srt_set_error(SRT_ENOMEM, "hipMalloc failed");
  launch_wave_blocks(foot_kernel, n, 0, (const Common *)m->d_common.p, m->geopack_psi, (long long)n, (const double *)dx.p, dout.p);
  HIP_OK(hipMemcpy(out, dout.p, 6 * n * sizeof(double), hipMemcpyDeviceToHost));
  return SRT_OK;
}

extern "C" int srt_is_right_handed(int64_t n, const double *in, int32_t *out) {
  if (!in || !out || n < 0) return srt_set_error(SRT_EINVAL, "bad argument");
  if (n == 0) return SRT_OK;
  DeviceScope srt_iscope_;
  int rc = srt_iscope_.enter_default();
  if (rc) return rc;
  DevBuf<double> din;
  DevBuf<int> dout;
  if ((rc = upload(din, in, 5 * n))) return rc;
  HIP_OK(dout.alloc(n));
  hipLaunchKernelGGL(handedness_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, (long long)n, (const double *)din.p, dout.p);
  hipError_t e = hipMemcpy(out, dout.p, n * sizeof(int), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return srt_set_error(SRT_EDEVICE, "handedness kernel: %s", hipGetErrorString(e));
  return SRT_OK;
}

extern "C" int srt_gradients(srt_model *m, int64_t n, const double *x, const double *k, const double *w, double del, double *out) {
  if (!m || !x || !k || !w || !out || n < 0) return srt_set_error(SRT_EINVAL, "bad argument");
  if (n == 0) return SRT_OK;
  SRT_MODEL_SCOPE;
  int rc = ensure_model(m);
  if (rc) return rc;
  DevBuf<double> dx, dk, dw, dout;
  if ((rc = upload(dx, x, 3 * n)) || (rc = upload(dk, k, 3 * n)) || (rc = upload(dw, w, n))) return rc;
  if (dout.alloc(14 * n) != hipSuccess) return srt_set_error(SRT_ENOMEM, "hipMalloc failed");
  rc = with_model(m, [&](auto tag) -> int {
    using T = decltype(tag);
    using M = typename T::Model;
    DevBuf<double> stage; // scattered model only; null for the others
    if constexpr (std::is_same<M, ScatteredModel>::value) stage_alloc(stage, n);
    launch_wave_blocks(gradients_kernel<M, T::lds>, n, 0, m->on_device<M>(), m->d_common.p, (long long)n, dx.p, dk.p, dw.p, del, dout.p,
                       stage.p);
    if constexpr (std::is_same<M, ScatteredModel>::value) HIP_OK(hipDeviceSynchronize()); // `stage` is freed at the end of this scope
    return SRT_OK;
  });
  if (rc) return rc;
  HIP_OK(hipMemcpy(out, dout.p, 14 * n * sizeof(double), hipMemcpyDeviceToHost));
  return SRT_OK;
}

extern "C" int srt_rk_step(srt_model *m, int64_t n, const double *args, const double *dt, double del, double *out) {
  if (!m || !args || !dt || !out || n < 0) return srt_set_error(SRT_EINVAL, "bad argument");
  if (n == 0) return SRT_OK;
  SRT_MODEL_SCOPE;
  int rc = ensure_model(m);
  if (rc) return rc;
  DevBuf<double> da, dd, dout;
  if ((rc = upload(da, args, 7 * n)) || (rc = upload(dd, dt, n))) return rc;
  if (dout.alloc(21 * n) != hipSuccess) return srt_set_error(SRT_ENOMEM, "hipMalloc failed");
  rc = with_model(m, [&](auto tag) -> int {
    using T = decltype(tag);
    using M = typename T::Model;
    DevBuf<double> stage; // scattered model only; null for the others
    if constexpr (std::is_same<M, ScatteredModel>::value) stage_alloc(stage, n);
    launch_wave_blocks(rkstep_kernel<M, T::lds>, n, 0, m->on_device<M>(), m->d_common.p, (long long)n, da.p, dd.p, del, dout.p, stage.p);
    if constexpr (std::is_same<M, ScatteredModel>::value) HIP_OK(hipDeviceSynchronize()); // `stage` is freed at the end of this scope
    return SRT_OK;
  });
  if (rc) return rc;
  HIP_OK(hipMemcpy(out, dout.p, 21 * n * sizeof(double), hipMemcpyDeviceToHost));
  return SRT_OK;
}


// ---- the random / adaptive sample-set builder (kernels and the level-by-level scheme: srt_sampler.hpp) ----
static int smp_eval(srt_model *src, long long n, double *rec) {
  if (n <= 0) return SRT_OK;
  return with_model(src, [&](auto tag) -> int {
    using T = decltype(tag);
    launch_wave_blocks(smp_eval_kernel<typename T::Model, T::lds>, n, 0, src->on_device<typename T::Model>(), n, rec);
    return SRT_OK;
  });
}

extern "C" int srt_build_samples(srt_model *src, const srt_sampler_params *sp, int64_t n_in, const double *in_pts,
                                 int64_t *n_out, double **out, int64_t stage_counts[6]) {
  if (!src || !sp || !n_out || !out || n_in < 0 || (n_in > 0 && !in_pts)) return srt_set_error(SRT_EINVAL, "bad argument");
  if (const int bad = with_model(src, [](auto) -> int { return SRT_OK; })) return bad; // an unknown kind fails before anything is allocated
  const double *bd = sp->bounds;
  if (!(bd[1] > bd[0]) || !(bd[3] > bd[2]) || !(bd[5] > bd[4])) return srt_set_error(SRT_EINVAL, "empty bounds");
  if (sp->n_zero_altitude < 0 || sp->n_iri_pad < 0 || sp->n_initial_radial < 0 || sp->n_initial_uniform < 0 || sp->max_recursion < 0 ||
      sp->numincrease < 0)
    return srt_set_error(SRT_EINVAL, "negative count");
  SRT_MODEL_SCOPE;
  int rc = ensure_model(src);
  if (rc) return rc;
  const int nspec = src->nspec, ninc = sp->numincrease ? sp->numincrease : 5;
  if (ninc > WAVE) return srt_set_error(SRT_EINVAL, "numincrease > %d", WAVE);
  const int max_passes = sp->max_passes > 0 ? sp->max_passes : 64;
  SmpBox root;
  for (int c = 0; c < 3; ++c) {
    root.lo[c] = bd[2 * c];
    root.hi[c] = bd[2 * c + 1];
  }
  root.id = 1;
  int64_t counts[6] = {n_in, 0, 0, 0, 0, 0};
  const size_t RB = SMP_REC * sizeof(double);
  DevBytes pool, slot, stage, valid;
  long long npool = 0;
#define SMP_OK(expr)                                                                        \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess) return srt_set_error(SRT_EDEVICE, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)
#define SMP_MEM(expr)                                                           \
  do {                                                                          \
    if ((expr)) return srt_set_error(SRT_ENOMEM, "device allocation failed (sampler)"); \
  } while (0)

  // (0) points of an existing file: part of the initial set and of the output (:210-227)
  if (n_in > 0) {
    std::vector<double> h((size_t)n_in * SMP_REC, 0.0);
    for (int64_t i = 0; i < n_in; ++i)
      for (int c = 0; c < 3 + nspec; ++c) h[(size_t)i * SMP_REC + c] = in_pts[(size_t)i * (3 + nspec) + c];
    SMP_MEM(pool.reserve(h.size() * sizeof(double)));
    SMP_OK(hipMemcpy(pool.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
    npool = n_in;
  }
  // shell and uniform stages share one routine: positions, f(x), then append (device) or compact (host)
  std::vector<double> tail; // zero-altitude and ionosphere samples, appended to the output after the pool
  auto run_stage = [&](int stg, long long n, double rmin, double rmax, bool to_pool, int64_t &count) -> int {
    if (n <= 0) return SRT_OK;
    SMP_MEM(stage.reserve((size_t)n * RB));
    SMP_MEM(valid.reserve((size_t)n * sizeof(int)));
    hipLaunchKernelGGL(smp_stage_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, stg, n, (unsigned long long)sp->seed, root, rmin,
                       rmax, stage.as<double>(), valid.as<int>());
    if (const int bad = smp_eval(src, n, stage.as<double>())) return bad;
    SMP_OK(hipDeviceSynchronize());
    if (to_pool) {
      std::vector<int> hv((size_t)n);
      SMP_OK(hipMemcpy(hv.data(), valid.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
      for (long long i = 0; i < n; ++i)
        if (!hv[i])
          return srt_set_error(SRT_EINVAL, "radial stage: sample %lld found no point of the shell inside the box in %d attempts", i, SMP_MAXTRY);
      SMP_MEM(pool.reserve((size_t)(npool + n) * RB, (size_t)npool * RB));
      SMP_OK(hipMemcpy(pool.as<double>() + (size_t)npool * SMP_REC, stage.p, (size_t)n * RB, hipMemcpyDeviceToDevice));
      npool += n;
      count = n;
    } else {
      std::vector<int> hv((size_t)n);
      std::vector<double> hr((size_t)n * SMP_REC);
      SMP_OK(hipMemcpy(hv.data(), valid.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
      SMP_OK(hipMemcpy(hr.data(), stage.p, (size_t)n * RB, hipMemcpyDeviceToHost));
      for (long long i = 0; i < n; ++i)
        if (hv[i]) {
          for (int c = 0; c < 3 + nspec; ++c) tail.push_back(hr[(size_t)i * SMP_REC + c]);
          ++count;
        }
    }
    return SRT_OK;
  };
  // (1) radial (:228-272): rmin = R_E, rmax = the farthest corner of the box
  {
    double r2 = 0.0;
    for (int q = 0; q < 8; ++q) {
      const double x = bd[q & 4 ? 1 : 0], y = bd[q & 2 ? 3 : 2], z = bd[q & 1 ? 5 : 4];
      const double v = x * x + y * y + z * z;
      if (v > r2) r2 = v;
    }
    if ((rc = run_stage(SMP_RADIAL, sp->n_initial_radial, R_E, sqrt(r2), true, counts[1]))) return rc;
  }
  // (2) uniform (:275-296)
  if ((rc = run_stage(SMP_UNIFORM, sp->n_initial_uniform, 0.0, 0.0, true, counts[2]))) return rc;

  // (3) adaptive (:298-347): tol halves until adaptive_nmax adaptive samples exist
  if (sp->adaptive_nmax > 0) {
    DevBytes keys0, keys1, idx0, idx1, sorttmp, callsA, callsB, halves, cand, nadd, refine, addA, addoff, childoff, scantmp;
    DevBytes *calls = &callsA, *children = &callsB;
    int64_t nsamples = 0;
    double tol = sp->initial_tol;
    for (int pass = 0; nsamples < sp->adaptive_nmax && pass < max_passes; ++pass, tol = tol / 2.0) {
      if (npool >= (1ll << 31) - (1ll << 26)) return srt_set_error(SRT_EINVAL, "sample pool too large");
      SMP_MEM(slot.reserve((size_t)npool * sizeof(int)));
      if (npool > 0) hipLaunchKernelGGL(smp_fill_int, dim3((unsigned)((npool + 255) / 256)), dim3(256), 0, 0, npool, slot.as<int>(), 0);
      SMP_MEM(calls->reserve(sizeof(SmpBox)));
      SMP_OK(hipMemcpy(calls->p, &root, sizeof(SmpBox), hipMemcpyHostToDevice));
      long long ncalls = 1;
      for (int depth = 0; depth <= sp->max_recursion && ncalls > 0; ++depth) {
        const int dim = depth % 3;
        const long long nhalf = 2 * ncalls;
        if (nhalf > (1ll << 26)) return srt_set_error(SRT_EINVAL, "adaptive sampler: %lld half-boxes at depth %d (tolerance too small)", nhalf, depth);
        const long long ncand = nhalf * 2 * ninc;
        SMP_MEM(keys0.reserve((size_t)npool * 4 + 4) || keys1.reserve((size_t)npool * 4 + 4) || idx0.reserve((size_t)npool * 4 + 4) ||
                idx1.reserve((size_t)npool * 4 + 4));
        SMP_MEM(halves.reserve((size_t)nhalf * sizeof(SmpBox)) || cand.reserve((size_t)ncand * RB));
        SMP_MEM(nadd.reserve((size_t)nhalf * 4) || refine.reserve((size_t)nhalf * 4) || addA.reserve((size_t)nhalf * 4) ||
                addoff.reserve((size_t)nhalf * 4) || childoff.reserve((size_t)nhalf * 4));
        if (npool > 0) {
          hipLaunchKernelGGL(smp_keys_kernel, dim3((unsigned)((npool + 255) / 256)), dim3(256), 0, 0, npool, pool.as<double>(), slot.as<int>(),
                             calls->as<SmpBox>(), dim, (unsigned)nhalf, keys0.as<unsigned>(), idx0.as<int>());
          int bits = 1;
          while ((1ll << bits) <= nhalf) ++bits;
          size_t need = 0;
          SMP_OK(hipcub::DeviceRadixSort::SortPairs(nullptr, need, keys0.as<unsigned>(), keys1.as<unsigned>(), idx0.as<int>(), idx1.as<int>(),
                                                    (int)npool, 0, bits, 0));
          SMP_MEM(sorttmp.reserve(need));
          SMP_OK(hipcub::DeviceRadixSort::SortPairs(sorttmp.p, need, keys0.as<unsigned>(), keys1.as<unsigned>(), idx0.as<int>(), idx1.as<int>(),
                                                    (int)npool, 0, bits, 0));
        }
        hipLaunchKernelGGL(smp_cand_kernel, dim3((unsigned)((ncand + 255) / 256)), dim3(256), 0, 0, (int)nhalf, calls->as<SmpBox>(), dim,
                           (unsigned long long)sp->seed, (unsigned long long)pass, ninc, halves.as<SmpBox>(), cand.as<double>());
        if ((rc = smp_eval(src, ncand, cand.as<double>()))) return rc;
        hipLaunchKernelGGL(smp_stats_kernel, dim3((unsigned)nhalf), dim3(WAVE), 0, 0, (int)nhalf, npool, keys1.as<unsigned>(), idx1.as<int>(),
                           pool.as<double>(), cand.as<double>(), halves.as<SmpBox>(), dim, nspec, ninc, tol, nadd.as<int>(), refine.as<int>(),
                           addA.as<int>());
        size_t need = 0;
        SMP_OK(hipcub::DeviceScan::ExclusiveSum(nullptr, need, nadd.as<int>(), addoff.as<int>(), (int)nhalf, 0));
        SMP_MEM(scantmp.reserve(need));
        SMP_OK(hipcub::DeviceScan::ExclusiveSum(scantmp.p, need, nadd.as<int>(), addoff.as<int>(), (int)nhalf, 0));
        SMP_OK(hipcub::DeviceScan::ExclusiveSum(scantmp.p, need, refine.as<int>(), childoff.as<int>(), (int)nhalf, 0));
        int last[4];
        SMP_OK(hipMemcpy(&last[0], addoff.as<int>() + nhalf - 1, 4, hipMemcpyDeviceToHost));
        SMP_OK(hipMemcpy(&last[1], nadd.as<int>() + nhalf - 1, 4, hipMemcpyDeviceToHost));
        SMP_OK(hipMemcpy(&last[2], childoff.as<int>() + nhalf - 1, 4, hipMemcpyDeviceToHost));
        SMP_OK(hipMemcpy(&last[3], refine.as<int>() + nhalf - 1, 4, hipMemcpyDeviceToHost));
        const long long total_add = (long long)last[0] + last[1], nchild = (long long)last[2] + last[3];
        const int make_children = depth + 1 <= sp->max_recursion ? 1 : 0; // a call beyond maxdepth returns at once (:65-68)
        if (npool + total_add >= (1ll << 31) - (1ll << 26)) return srt_set_error(SRT_EINVAL, "sample pool too large");
        SMP_MEM(pool.reserve((size_t)(npool + total_add) * RB, (size_t)npool * RB));
        SMP_MEM(slot.reserve((size_t)(npool + total_add) * sizeof(int), (size_t)npool * sizeof(int)));
        SMP_MEM(children->reserve((size_t)(nchild > 0 ? nchild : 1) * sizeof(SmpBox)));
        if (npool > 0)
          hipLaunchKernelGGL(smp_reslot_kernel, dim3((unsigned)((npool + 255) / 256)), dim3(256), 0, 0, npool, keys0.as<unsigned>(),
                             (unsigned)nhalf, refine.as<int>(), childoff.as<int>(), make_children, slot.as<int>());
        hipLaunchKernelGGL(smp_commit_kernel, dim3((unsigned)((nhalf + 255) / 256)), dim3(256), 0, 0, (int)nhalf, ninc, addA.as<int>(),
                           refine.as<int>(), addoff.as<int>(), childoff.as<int>(), make_children, cand.as<double>(), halves.as<SmpBox>(),
                           npool, pool.as<double>(), slot.as<int>(), children->as<SmpBox>());
        SMP_OK(hipDeviceSynchronize());
        npool += total_add;
        nsamples += total_add;
        std::swap(calls, children);
        ncalls = make_children ? nchild : 0;
      }
    }
    counts[3] = nsamples;
  }
  // (4) zero altitude (:349-377), (5) ionosphere shell R_E .. R_E + 2000 km (:379-405): one draw each, kept when inside
  if ((rc = run_stage(SMP_ZEROALT, sp->n_zero_altitude, R_E, R_E, false, counts[4]))) return rc;
  if ((rc = run_stage(SMP_IRI, sp->n_iri_pad, R_E, R_E + 2000000.0, false, counts[5]))) return rc;

  const size_t w = 3 + (size_t)nspec, ntail = tail.size() / w;
  double *res = (double *)malloc(((size_t)npool + ntail + 1) * w * sizeof(double));
  if (!res) return srt_set_error(SRT_ENOMEM, "malloc failed");
  if (npool > 0) {
    std::vector<double> h((size_t)npool * SMP_REC);
    hipError_t e = hipMemcpy(h.data(), pool.p, h.size() * sizeof(double), hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
      free(res);
      return srt_set_error(SRT_EDEVICE, "sample download: %s", hipGetErrorString(e));
    }
    for (long long i = 0; i < npool; ++i)
      for (size_t c = 0; c < w; ++c) res[(size_t)i * w + c] = h[(size_t)i * SMP_REC + c];
  }
  if (ntail) memcpy(res + (size_t)npool * w, tail.data(), tail.size() * sizeof(double));
  *out = res;
  *n_out = npool + (int64_t)ntail;
  if (stage_counts)
    for (int q = 0; q < 6; ++q) stage_counts[q] = counts[q];
  return SRT_OK;
#undef SMP_OK
#undef SMP_MEM
}

// ------------------------------------------------------------------------------------------ hot path
extern "C" int32_t srt_rows_per_ray(const srt_params *p) {
  if (!p || p->maxsteps < 1) return 0;
  int per = p->outputper < 1 ? 1 : p->outputper;
  return (p->maxsteps + per - 1) / per;
}

static int check_params(const srt_params *p) {
  if (!p) return srt_set_error(SRT_EINVAL, "null params");
  if (p->maxsteps < 1) return srt_set_error(SRT_EINVAL, "maxsteps must be >= 1");
  if (p->root != 1 && p->root != 2) return srt_set_error(SRT_EINVAL, "root must be 1 or 2");
  if (!(p->del > 0.0)) return srt_set_error(SRT_EINVAL, "del must be > 0");
  if (p->ray_order < 0 || p->ray_order > 2) return srt_set_error(SRT_EINVAL, "ray_order must be 0, 1 or 2");
  return SRT_OK;
}

// ray_order = 1: Morton code of the launch cell (9 bits per axis) per ray
__device__ __forceinline__ unsigned spread3(unsigned v) { // 0b abc -> 0b a00b00c
  v &= 0x3ffu;
  v = (v | (v << 16)) & 0x030000ffu;
  v = (v | (v << 8)) & 0x0300f00fu;
  v = (v | (v << 4)) & 0x030c30c3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}
// two_class (ray_order = 2, an experiment switch: HISTORY.md section 9): rays that are likely to stop early -- above 6 kHz and
// launched inwards: 8.5 % of the BASELINE launch set, mean 75 rows against 197 -- sort behind all others (key bit 30: above the Morton code, 10 bits per axis = bits 0..29)
__global__ void ray_keys_kernel(const InterpModel *mp, const double *pos0 /* SoA [3][n] */, const double *dir0, const double *w0,
                                int two_class, long long n, unsigned *keys, int *ids) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const InterpModel &m = *mp;
  double xl;
  const double x = pos0[i], y = pos0[n + i], z = pos0[2 * n + i];
  unsigned ci = (unsigned)m.ax.locate(x, xl), cj = (unsigned)m.ay.locate(y, xl), ck = (unsigned)m.az.locate(z, xl);
  unsigned key = spread3(ci) | (spread3(cj) << 1) | (spread3(ck) << 2);
  if (two_class) {
    const bool inward = dir0[i] * x + dir0[n + i] * y + dir0[2 * n + i] * z < 0.0;
    if (inward && w0[i] > 2.0 * PI * 6.0e3) key |= 1u << 30;
  }
  keys[i] = key;
  ids[i] = (int)i;
}

// scattered model: one of a slot's two scratch blocks, `per_block` doubles for each one-wave block of the grid, regrown when the
// grid outgrows it; *out = null when it was refused
static int slot_scratch(srt_model *m, srt_model::LaunchSlot &sl, srt_model::Scratch &s, long long grid, size_t per_block,
                        const char *what, double **out) {
  if (grid > s.blocks && !(s.failed > 0 && grid >= s.failed)) {
    if (sl.used) HIP_OK(hipEventSynchronize(sl.done)); // about to free what that launch may still read
    s.blocks = 0;
    if (s.buf.alloc((size_t)grid * per_block) == hipSuccess) s.blocks = grid;
    else {
      (void)hipGetLastError();
      s.failed = grid;
      scratch_refused(m, what, (size_t)grid * per_block * sizeof(double));
    }
  }
  *out = grid <= s.blocks ? s.buf.p : nullptr;
  return SRT_OK;
}

// one segment of a segmented trace (srt_trace_segment_device); nullptr = the unsegmented launch
struct SegLaunch {
  int32_t rows, segment;
  const int32_t *queue;
  int64_t nqueue;
  double *state;
};
static_assert(SRT_STATE == TRACE_STATE, "srt.h and srt_kernels.hpp disagree on a paused ray's record");

// the one launch path of the trace kernels: arguments checked by the two entry points below
static int trace_launch(srt_model *m, const srt_params *p, int64_t nrays, const double *d_pos0, const double *d_dir0,
                        const double *d_w0, double *d_rows, int32_t *d_nrows, int32_t *d_stopcond, int64_t *d_counters,
                        void *stream, const SegLaunch *sg) {
  int rc;
  SRT_MODEL_SCOPE;
  if ((rc = ensure_model(m))) return rc;
  hipStream_t st = (hipStream_t)stream;
  TraceSegArgs a; // (the unsegmented kernels take its TraceArgs part)
  a.pos0 = d_pos0;
  a.dir0 = d_dir0;
  a.w0 = d_w0;
  a.nrays = nrays;
  a.rows = d_rows;
  a.nrows = d_nrows;
  a.stopcond = d_stopcond;
  a.counters = (unsigned long long *)d_counters;
  a.p.dt0 = p->dt0; a.p.dtmax = p->dtmax; a.p.tmax = p->tmax; a.p.maxerr = p->maxerr;
  a.p.minalt = p->minalt; a.p.del = p->del;
  a.p.maxsteps = p->maxsteps; a.p.root = p->root; a.p.fixedstep = p->fixedstep;
  a.p.outputper = p->outputper < 1 ? 1 : p->outputper;
  a.p.first_attempt_policy = p->first_attempt_policy;
  a.p.refill_threshold = p->refill_threshold;
  a.p.slots = srt_rows_per_ray(p);
  a.order = sg ? sg->queue : nullptr;
  a.state = sg ? sg->state : nullptr;
  a.nqueue = sg && sg->segment > 0 ? sg->nqueue : nrays;
  a.seg_rows = sg ? sg->rows : 0;
  a.segment = sg ? sg->segment : 0;
  const long long nwork = a.nqueue; // rays this launch works on
  HIP_OK(hipMemsetAsync(d_counters, 0, 4 * sizeof(int64_t), st));
  if (nwork == 0 && sg) return SRT_OK;
  // persistent grid: enough one-wave blocks to fill the chip, never more than the rays need
  int per_cu = 0;
  rc = with_model(m, [&](auto tag) -> int {
    per_cu = decltype(tag)::waves_per_cu;
    return SRT_OK;
  });
  if (rc) return rc;
  if (const char *e = getenv("SRT_WAVES_PER_CU")) {
    const int v = atoi(e);
    if (v >= 1 && v <= per_cu) per_cu = v;
  }
  long long grid = (long long)m->cu_count * per_cu;
  // Rays a wave holds at most.  64 = every lane.  (Measured for the Ngo model, whose launch at BASELINE config[1] is as long as
  // its longest ray: with at most 8 rays per wave every trip runs in tail mode -- the 8 stencil points of a ray on 8 lanes,
  // srt_models.hpp -- but a tail-mode trip is only 2.2x shorter than a full one while serving 8x fewer rays: 47.5 -> 51.6 ms.
  // SRT_WAVE_CAP / SRT_WAVES_PER_CU remain as experiment switches; a ray's arithmetic does not depend on either.)
  int cap = WAVE;
  if (const char *e = getenv("SRT_WAVE_CAP")) {
    const int v = atoi(e);
    if (v >= 1 && v <= WAVE) cap = v;
  }
  a.p.wave_cap = cap;
  long long want = (nwork + cap - 1) / cap;
  if (grid > want) grid = want;
  if (grid < 1) grid = 1;
  // scratch slot: one whose last launch is over (preferring one that holds buffers already), else a fresh one, else -- all
  // busy -- the next in turn, which this stream then waits for
  int si = -1;
  for (int k = 0; k < srt_model::NSLOT && si < 0; ++k)
    if (m->slot[k].used) {
      const hipError_t q = hipEventQuery(m->slot[k].done);
      if (q == hipSuccess) si = k;
      else if (q != hipErrorNotReady) HIP_OK(q);
      else (void)hipGetLastError();
    }
  for (int k = 0; k < srt_model::NSLOT && si < 0; ++k)
    if (!m->slot[k].used) si = k;
  if (si < 0) {
    si = m->rr_slot;
    m->rr_slot = (m->rr_slot + 1) % srt_model::NSLOT;
  }
  srt_model::LaunchSlot &sl = m->slot[si];
  if (sl.used) HIP_OK(hipStreamWaitEvent(st, sl.done, 0)); // the slot's previous launch (maybe on another stream) is over
  srt_model::LaunchTimes &lt = m->hist[m->next_hist];
  HIP_OK(hipEventRecord(lt.ev0, st));
  const InterpModel &im = m->as<InterpModel>();
  if (p->ray_order >= 1 && a.segment == 0 && (m->kind == KIND_INTERP || m->kind == KIND_INTERP_NODES) && nrays > WAVE && nrays < (1ll << 31) && im.ax.n < 1023 && im.ay.n < 1023 &&
      im.az.n < 1023) {
    // work through the launch set in the order of the rays' launch cells (inside the timed region)
    if ((size_t)nrays > sl.ids[1].cap) {
      if (sl.used) HIP_OK(hipEventSynchronize(sl.done)); // about to free what that launch may still read
      // all four are dropped before the first is allocated, and ids[1] comes last: after a refused allocation it is empty, so
      // the next launch on this slot allocates all four again
      for (int k = 0; k < 2; ++k) {
        sl.keys[k].release();
        sl.ids[k].release();
      }
      for (int k = 0; k < 2; ++k) {
        HIP_OK(sl.keys[k].alloc((size_t)nrays));
        HIP_OK(sl.ids[k].alloc((size_t)nrays));
      }
    }
    size_t need = 0;
    HIP_OK(hipcub::DeviceRadixSort::SortPairs(nullptr, need, sl.keys[0].p, sl.keys[1].p, sl.ids[0].p, sl.ids[1].p, (int)nrays, 0, 31, st));
    if (need > sl.sorttmp.cap) {
      if (sl.used) HIP_OK(hipEventSynchronize(sl.done));
      HIP_OK(sl.sorttmp.alloc(need));
    }
    hipLaunchKernelGGL(ray_keys_kernel, dim3((unsigned)((nrays + 255) / 256)), dim3(256), 0, st,
                       m->kind == KIND_INTERP ? m->on_device<InterpModel>() : (const InterpModel *)m->d_axes.p, d_pos0,
                       d_dir0, d_w0, p->ray_order == 2 ? 1 : 0, (long long)nrays, sl.keys[0].p, sl.ids[0].p);
    size_t tb = sl.sorttmp.cap;
    HIP_OK(hipcub::DeviceRadixSort::SortPairs(sl.sorttmp.p, tb, sl.keys[0].p, sl.keys[1].p, sl.ids[0].p, sl.ids[1].p, (int)nrays, 0, 31, st));
    a.order = sl.ids[1].p;
  }
  // scattered model: without the staging records the kernel still runs (own-list path everywhere), without the candidate blocks
  // it scans the cells for every stencil -- only slower
  a.scratch = a.scratch2 = nullptr;
  if (m->kind == KIND_SCATTERED && staging_enabled() &&
      (rc = slot_scratch(m, sl, sl.stage, grid, (size_t)ScatteredModel::REC_CAP * ScatteredModel::REC, "staging records", &a.scratch)))
    return rc;
  if (m->kind == KIND_SCATTERED && a.scratch != nullptr && blocks_enabled() &&
      (rc = slot_scratch(m, sl, sl.cand, grid, ScatteredModel::BLOCK_DOUBLES, "candidate blocks", &a.scratch2)))
    return rc;
  const bool fixed = p->fixedstep != 0;
  const int fopt = m->cm.fld.use_tsy != 0 ? 2 : (m->cm.fld.use_igrf != 0 ? 1 : 0);
  // one instantiation per (model, integrator, field option): the dipole kernels carry none of the IGRF code, the
  // IGRF-alone kernels none of the T04 call sites
  rc = with_model(m, [&](auto tag) -> int {
    using T = decltype(tag);
    using M = typename T::Model;
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(WAVE), 0, st, m->on_device<M>(), m->d_common.p, a);
    };
    auto pick = [&](auto seg) { // (its segmented twin beside every kernel)
      constexpr bool SEG = decltype(seg)::value;
      if (fixed) {
        if (fopt == 2) launch(trace_kernel<M, true, T::lds, 2, SEG>);
        else if (fopt == 1) launch(trace_kernel<M, true, T::lds, 1, SEG>);
        else launch(trace_kernel<M, true, T::lds, 0, SEG>);
      } else {
        if (fopt == 2) launch(trace_kernel<M, false, T::lds, 2, SEG>);
        else if (fopt == 1) launch(trace_kernel<M, false, T::lds, 1, SEG>);
        else launch(trace_kernel<M, false, T::lds, 0, SEG>);
      }
    };
    if (sg) pick(std::true_type{});
    else pick(std::false_type{});
    return SRT_OK;
  });
  if (rc) return rc;
  HIP_OK(hipGetLastError());
  HIP_OK(hipEventRecord(lt.ev1, st));
  HIP_OK(hipEventRecord(sl.done, st));
#ifdef SRT_TRIP_TIMING
  if (getenv("SRT_TRIP_TIMING")) {
    unsigned long long h[srt::TT_SLOTS];
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpyFromSymbol(h, HIP_SYMBOL(srt_trip_cycles), sizeof h));
    fprintf(stderr, "srt trip cycles:");
    for (int i = 0; i < srt::TT_SLOTS; ++i) fprintf(stderr, " %llu", h[i]);
    fprintf(stderr, "\n");
    memset(h, 0, sizeof h);
    HIP_OK(hipMemcpyToSymbol(HIP_SYMBOL(srt_trip_cycles), h, sizeof h));
  }
#endif
#ifdef SRT_PHASE_TIMING
  if (m->kind == KIND_SCATTERED && getenv("SRT_PHASE_TIMING")) {
    unsigned long long h[16];
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpyFromSymbol(h, HIP_SYMBOL(srt_phase_cycles), sizeof h));
    fprintf(stderr, "srt phase cycles:");
    for (int i = 0; i < 16; ++i) fprintf(stderr, " %llu", h[i]);
    fprintf(stderr, "\n");
    memset(h, 0, sizeof h);
    HIP_OK(hipMemcpyToSymbol(HIP_SYMBOL(srt_phase_cycles), h, sizeof h));
    {
      unsigned long long ts[8];
      HIP_OK(hipMemcpyFromSymbol(ts, HIP_SYMBOL(srt_tier_stats), sizeof ts));
      fprintf(stderr, "srt tier stats (stencils, second-order, no centre, near sample, L bound, h bound, free point, other):");
      for (int i = 0; i < 8; ++i) fprintf(stderr, " %llu", ts[i]);
      fprintf(stderr, "\n");
      memset(ts, 0, sizeof ts);
      HIP_OK(hipMemcpyToSymbol(HIP_SYMBOL(srt_tier_stats), ts, sizeof ts));
    }
    unsigned long long ws[4];
    float ms = 0.f;
    HIP_OK(hipMemcpyFromSymbol(ws, HIP_SYMBOL(srt_wave_stats), sizeof ws));
    HIP_OK(hipEventElapsedTime(&ms, lt.ev0, lt.ev1));
    // (the timers of the eight XCDs are not aligned with each other: only a wave's own span means something)
    fprintf(stderr, "srt wave stats: grid %lld, working waves %llu, launch %.1f ms, mean span of a working wave %.4g ticks = %.1f MHz if it ran for the whole launch\n",
            grid, ws[0], ms, ws[0] ? (double)ws[1] / (double)ws[0] : 0.0, ws[0] ? (double)ws[1] / (double)ws[0] / (ms * 1e3) : 0.0);
    const unsigned long long z[4] = {0ull, 0ull, ~0ull, 0ull};
    HIP_OK(hipMemcpyToSymbol(HIP_SYMBOL(srt_wave_stats), z, sizeof z));
  }
#endif
  sl.used = true;
  lt.used = true;
  m->last_hist = m->next_hist;
  m->next_hist = (m->next_hist + 1) % srt_model::NHIST;
  return SRT_OK;
}

extern "C" int srt_trace_batch_device(srt_model *m, const srt_params *p, int64_t nrays, const double *d_pos0,
                                      const double *d_dir0, const double *d_w0, double *d_rows, int32_t *d_nrows,
                                      int32_t *d_stopcond, int64_t *d_counters, void *stream) {
  if (!m || !d_pos0 || !d_dir0 || !d_w0 || !d_rows || !d_nrows || !d_stopcond || !d_counters || nrays < 0)
    return srt_set_error(SRT_EINVAL, "bad argument");
  int rc = check_params(p);
  if (rc) return rc;
  return trace_launch(m, p, nrays, d_pos0, d_dir0, d_w0, d_rows, d_nrows, d_stopcond, d_counters, stream, nullptr);
}

// ---- the hot path in segments (srt.h): pure host code first
extern "C" int32_t srt_trace_segments(const srt_params *p, int32_t segment_rows) {
  const int32_t slots = srt_rows_per_ray(p);
  if (slots < 1 || segment_rows < 1) return 0;
  return (int32_t)(((int64_t)slots + segment_rows - 1) / segment_rows);
}
// the refusals every segmented entry point shares, by name, before the device is touched
static int check_segments(const srt_params *p, int64_t nrays, int32_t segment_rows) {
  int rc = check_params(p);
  if (rc) return rc;
  if (segment_rows < 1) return srt_set_error(SRT_EINVAL, "segment_rows=%d: a segment keeps at least one row per ray", (int)segment_rows);
  if (segment_rows > srt_rows_per_ray(p))
    return srt_set_error(SRT_EINVAL, "segment_rows=%d exceeds the %d rows a ray keeps at most (srt_rows_per_ray)", (int)segment_rows,
                         (int)srt_rows_per_ray(p));
  if (nrays < 0) return srt_set_error(SRT_EINVAL, "nrays=%lld is negative", (long long)nrays);
  if (nrays >= (1ll << 31)) return srt_set_error(SRT_EINVAL, "nrays=%lld: a segmented trace takes fewer than 2^31 rays (ray ids are int32)", (long long)nrays);
  return SRT_OK;
}

extern "C" int srt_trace_segment_device(srt_model *m, const srt_params *p, int64_t nrays, const double *d_pos0, const double *d_dir0,
                                        const double *d_w0, int32_t segment_rows, int32_t segment, const int32_t *d_queue,
                                        int64_t nqueue, double *d_state, double *d_rows, int32_t *d_nrows, int32_t *d_stopcond,
                                        int64_t *d_counters, void *stream) {
  int rc = check_segments(p, nrays, segment_rows);
  if (rc) return rc;
  if (segment < 0) return srt_set_error(SRT_EINVAL, "segment=%d is negative", (int)segment);
  if (segment > 0 && !d_queue) return srt_set_error(SRT_EINVAL, "segment %d without a queue: later segments resume the rays d_queue names", (int)segment);
  if (segment == 0 && d_queue) return srt_set_error(SRT_EINVAL, "segment 0 launches every ray: d_queue must be NULL");
  if (segment > 0 && (nqueue < 0 || nqueue > nrays)) return srt_set_error(SRT_EINVAL, "nqueue=%lld is not within 0 .. nrays", (long long)nqueue);
  if (!m || !d_pos0 || !d_dir0 || !d_w0 || !d_state || !d_rows || !d_nrows || !d_stopcond || !d_counters)
    return srt_set_error(SRT_EINVAL, "null argument");
  const SegLaunch sg = {segment_rows, segment, d_queue, nqueue, d_state};
  return trace_launch(m, p, nrays, d_pos0, d_dir0, d_w0, d_rows, d_nrows, d_stopcond, d_counters, stream, &sg);
}

struct IsRunning {
  __host__ __device__ int operator()(int32_t stop) const { return stop == SRT_RUNNING ? 1 : 0; }
};
extern "C" int srt_running_rays_device(int64_t nrays, const int32_t *d_stopcond, int32_t *d_queue, int32_t *d_count, void *stream) {
  if (nrays < 0 || !d_count || (nrays > 0 && (!d_stopcond || !d_queue))) return srt_set_error(SRT_EINVAL, "bad argument");
  if (nrays >= (1ll << 31)) return srt_set_error(SRT_EINVAL, "nrays=%lld: ray ids are int32", (long long)nrays);
  int dev = -1, rc;
  {
    const void *ptrs[3] = {d_count, nrays > 0 ? (const void *)d_stopcond : nullptr, nrays > 0 ? (const void *)d_queue : nullptr};
    if ((rc = device_of("srt_running_rays_device", ptrs, 3, &dev))) return rc;
  }
  DeviceScope scope;
  if ((rc = scope.enter(dev))) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (nrays == 0) {
    HIP_OK(hipMemsetAsync(d_count, 0, sizeof(int32_t), st));
    return SRT_OK;
  }
  // ids 0 .. nrays - 1 selected by their flag; DeviceSelect keeps the input's order, so the queue is ascending
  hipcub::CountingInputIterator<int32_t> ids(0);
  auto flags = hipcub::TransformInputIterator<int, IsRunning, const int32_t *>(d_stopcond, IsRunning{});
  size_t need = 0;
  HIP_OK(hipcub::DeviceSelect::Flagged(nullptr, need, ids, flags, d_queue, d_count, (int)nrays, st));
  void *tmp = nullptr;
  HIP_OK(hipMallocAsync(&tmp, need ? need : 16, st));
  const hipError_t e = hipcub::DeviceSelect::Flagged(tmp, need, ids, flags, d_queue, d_count, (int)nrays, st);
  const hipError_t ef = hipFreeAsync(tmp, st); // (also on the error path)
  HIP_OK(e);
  HIP_OK(ef);
  return SRT_OK;
}

extern "C" int srt_launch_ms(srt_model *m, int back, float *ms) {
  if (!m || !ms) return srt_set_error(SRT_EINVAL, "null argument");
  if (back < 0 || back >= srt_model::NHIST || m->last_hist < 0) return srt_set_error(SRT_EINVAL, "no such launch");
  srt_model::LaunchTimes &lt = m->hist[(m->last_hist - back + srt_model::NHIST) % srt_model::NHIST];
  if (!lt.used) return srt_set_error(SRT_EINVAL, "no such launch");
  SRT_MODEL_SCOPE;
  int rc = ensure_model(m);
  if (rc) return rc;
  HIP_OK(hipEventSynchronize(lt.ev1));
  HIP_OK(hipEventElapsedTime(ms, lt.ev0, lt.ev1));
  return SRT_OK;
}

extern "C" int srt_last_kernel_ms(srt_model *m, float *ms) { return srt_launch_ms(m, 0, ms); }


// ---- the step after the path: hot-plasma damping along the kept rows (kernels: srt_damping.hpp) ----
extern "C" int srt_damping_device(const srt_damping_params *dp, int nspec, const double *qs, const double *ms, int32_t slots,
                                  int32_t outputper, int64_t nrays, const double *d_rows, const int32_t *d_nrows,
                                  const double *d_w0, double *d_rate, double *d_magnitude, int32_t *d_flag, void *stream) {
  if (!dp || !qs || !ms || !d_rows || !d_nrows || !d_w0 || !d_rate || !d_flag || nrays < 0)
    return srt_set_error(SRT_EINVAL, "bad argument");
  if (nspec < 1 || nspec > SRT_MAXSPEC) return srt_set_error(SRT_EINVAL, "nspec=%d unsupported", nspec);
  if (slots < 1 || outputper < 1) return srt_set_error(SRT_EINVAL, "slots and outputper must be >= 1");
  if (dp->dist != 0 && dp->dist != 1) return srt_set_error(SRT_EINVAL, "dist must be 0 (suprathermal) or 1 (Maxwell-Boltzmann)");
  if (dp->mode != 0 && dp->mode != 1) return srt_set_error(SRT_EINVAL, "mode must be 0 (spatial) or 1 (temporal)");
  if (dp->nres < 0 || dp->nres > DMP_MAXRES) return srt_set_error(SRT_EINVAL, "nres out of range (0..%d)", DMP_MAXRES);
  if (dp->dist == 1 && (!(dp->kT > 0.0) || !(dp->Ne_h >= 0.0))) return srt_set_error(SRT_EINVAL, "Maxwell-Boltzmann needs kT > 0 and Ne_h >= 0");
  if (!(dp->tol >= 0.0)) return srt_set_error(SRT_EINVAL, "tol must be >= 0");
  if (nrays == 0) return SRT_OK;
  // the work goes to the device that owns the buffers (as srt_pack_rows_device), for the duration of the call
  int dev = -1, rc;
  {
    const void *ptrs[6] = {d_rows, d_nrows, d_w0, d_rate, d_magnitude, d_flag};
    if ((rc = device_of("srt_damping_device", ptrs, 6, &dev))) return rc;
  }
  DeviceScope scope;
  if ((rc = scope.enter(dev))) return rc;
  if (nrays * (long long)slots >= (1ll << 40)) return srt_set_error(SRT_EINVAL, "too many rows");
  DampArgs a;
  a.rows = d_rows;
  a.nrows = d_nrows;
  a.w0 = d_w0;
  a.nrays = nrays;
  a.slots = slots;
  a.outputper = outputper;
  a.nspec = nspec;
  for (int s = 0; s < MAXSPEC; ++s) {
    a.q[s] = s < nspec ? qs[s] : 0.0;
    a.ms[s] = s < nspec ? ms[s] : 1.0;
  }
  a.p.dist = dp->dist;
  a.p.mode = dp->mode;
  a.p.nres = dp->nres ? dp->nres : 3;
  for (int i = 0; i < DMP_MAXRES; ++i) a.p.m[i] = dp->nres ? dp->m[i] : (i < 3 ? i - 1 : 0);
  for (int i = 0; i < a.p.nres; ++i)
    if (a.p.m[i] < -16 || a.p.m[i] > 16) return srt_set_error(SRT_EINVAL, "resonance order %d out of range", a.p.m[i]);
  a.p.Ne_h = dp->Ne_h;
  a.p.kT = dp->kT;
  a.p.tol = dp->tol > 0.0 ? dp->tol : 1e-3;
  a.p.qh = -1.60217646e-19; // const.m
  a.p.mh = 9.10938188e-31;
  a.rate = d_rate;
  a.flag = d_flag;
  hipStream_t st = (hipStream_t)stream;
  const long long total = nrays * slots;
  const long long grid = total < (1ll << 30) ? total : (1ll << 30);
  hipLaunchKernelGGL(damping_rate_kernel, dim3((unsigned)grid), dim3(WAVE), 0, st, a);
  if (d_magnitude) hipLaunchKernelGGL(damping_magnitude_kernel, dim3((unsigned)((nrays + 63) / 64)), dim3(64), 0, st, a, d_magnitude);
  HIP_OK(hipGetLastError());
  return SRT_OK;
}

extern "C" int srt_damping(const srt_damping_params *dp, int nspec, const double *qs, const double *ms, int32_t slots,
                           int32_t outputper, int64_t nrays, const double *rows, const int32_t *nrows, const double *w0,
                           double *rate, double *magnitude, int32_t *flag) {
  if (!rows || !nrows || !w0 || !rate || nrays < 0 || slots < 1) return srt_set_error(SRT_EINVAL, "bad argument");
  DeviceScope srt_iscope_;
  int rc = srt_iscope_.enter_default();
  if (rc) return rc;
  if (nrays == 0) return SRT_OK;
  const size_t nr = (size_t)nrays * slots;
  DevBuf<double> d_rows, d_w0, d_rate, d_mag;
  DevBuf<int> d_nrows, d_flag;
  if ((rc = upload(d_rows, rows, nr * SRT_ROW)) || (rc = upload(d_w0, w0, nrays))) return rc;
  if (d_rate.alloc(nr) != hipSuccess || d_mag.alloc(nr) != hipSuccess) return srt_set_error(SRT_ENOMEM, "hipMalloc failed");
  hipError_t e = d_nrows.alloc(nrays);
  if (e == hipSuccess) e = d_flag.alloc(nr);
  if (e == hipSuccess) e = hipMemcpy(d_nrows.p, nrows, nrays * sizeof(int), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    rc = srt_damping_device(dp, nspec, qs, ms, slots, outputper, nrays, d_rows.p, d_nrows.p, d_w0.p, d_rate.p, d_mag.p, d_flag.p, nullptr);
    if (!rc) e = hipDeviceSynchronize();
    if (!rc && e == hipSuccess) e = hipMemcpy(rate, d_rate.p, nr * sizeof(double), hipMemcpyDeviceToHost);
    if (!rc && e == hipSuccess && magnitude) e = hipMemcpy(magnitude, d_mag.p, nr * sizeof(double), hipMemcpyDeviceToHost);
    if (!rc && e == hipSuccess && flag) e = hipMemcpy(flag, d_flag.p, nr * sizeof(int), hipMemcpyDeviceToHost);
  }
  if (rc) return rc;
  if (e != hipSuccess) return srt_set_error(SRT_EDEVICE, "damping: %s", hipGetErrorString(e));
  return SRT_OK;
}


// ---- packed trajectory rows (multi-GPU gather, SURVEY 8e: only the rows a ray produced travel) ----
// kept rows of a ray = rows 0, outputper, 2*outputper, .. < nrows  (raytracer_driver.f95:1197)
struct KeptRows {
  const int32_t *nrows;
  int32_t outputper, slots;
  __host__ __device__ long long operator()(long long i) const {
    const int32_t n = nrows[i];
    int32_t k = n > 0 ? (n - 1) / outputper + 1 : 0;
    return k < slots ? k : slots;
  }
};
// the blocks of a grid-stride launch over n items, `per` to a block: ceil(n / per), 65536 at most
static unsigned grid_blocks(long long n, long long per) {
  const long long blocks = (n + per - 1) / per;
  return (unsigned)(blocks < 65536 ? blocks : 65536);
}
__global__ void pack_total_kernel(KeptRows kr, long long nrays, long long *offsets) {
  offsets[nrays] = offsets[nrays - 1] + kr(nrays - 1);
}
// one wave per ray: the ray's kept rows are one contiguous run of 160-B records in both buffers
__global__ __launch_bounds__(256) void pack_rows_kernel(long long nrays, int slots, const double *__restrict__ rows,
                                                        const long long *__restrict__ offsets, double *__restrict__ packed,
                                                        long long capacity) {
  const int lane = threadIdx.x & 63;
  for (long long ray = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); ray < nrays; ray += (long long)gridDim.x * 4) {
    const long long o0 = offsets[ray], o1 = offsets[ray + 1];
    if (o1 > capacity) continue; // the caller sees offsets[nrays] > capacity and fails the call
    const long long ndbl = (o1 - o0) * SRT_ROW;
    const double2 *src = (const double2 *)(rows + (size_t)ray * slots * SRT_ROW);
    double2 *dst = (double2 *)(packed + (size_t)o0 * SRT_ROW);
    for (long long q = lane; q < ndbl / 2; q += 64) dst[q] = src[q];
  }
}

extern "C" int srt_pack_rows_device(int32_t slots, int32_t outputper, int64_t nrays, const double *d_rows,
                                    const int32_t *d_nrows, int64_t *d_offsets, double *d_packed,
                                    int64_t capacity_rows, void *stream) {
  if (!d_offsets || nrays < 0 || slots < 1 || outputper < 1 || capacity_rows < 0 ||
      (nrays > 0 && (!d_rows || !d_nrows || (!d_packed && capacity_rows > 0))))
    return srt_set_error(SRT_EINVAL, "bad argument");
  // The work goes to the device that OWNS the buffers (not to whatever device the calling thread happens to be bound to):
  // a process may drive several GPUs from one thread.  All buffers must live on one device.
  int dev = -1, rc;
  {
    const void *ptrs[4] = {d_offsets, nrays > 0 ? (const void *)d_rows : nullptr, nrays > 0 ? (const void *)d_nrows : nullptr,
                           nrays > 0 && capacity_rows > 0 ? (const void *)d_packed : nullptr};
    if ((rc = device_of("srt_pack_rows_device", ptrs, 4, &dev))) return rc;
  }
  DeviceScope scope;
  if ((rc = scope.enter(dev))) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (nrays == 0) {
    HIP_OK(hipMemsetAsync(d_offsets, 0, sizeof(int64_t), st));
    return SRT_OK;
  }
  if (nrays >= (1ll << 31) - 1) return srt_set_error(SRT_EINVAL, "too many rays for one pack call");
  // offsets[0 .. nrays] = exclusive prefix sums of the kept-row counts (one extra item so the total lands in [nrays])
  static_assert(sizeof(long long) == sizeof(int64_t), "int64");
  auto counts = hipcub::TransformInputIterator<long long, KeptRows, hipcub::CountingInputIterator<long long>>(
      hipcub::CountingInputIterator<long long>(0), KeptRows{d_nrows, outputper, slots});
  size_t need = 0;
  HIP_OK(hipcub::DeviceScan::ExclusiveSum(nullptr, need, counts, (long long *)d_offsets, (int)nrays, st));
  void *tmp = nullptr;
  HIP_OK(hipMallocAsync(&tmp, need ? need : 16, st));
  hipError_t e = hipcub::DeviceScan::ExclusiveSum(tmp, need, counts, (long long *)d_offsets, (int)nrays, st);
  const hipError_t ef = hipFreeAsync(tmp, st); // (also on the error path)
  HIP_OK(e);
  HIP_OK(ef);
  // offsets[nrays] = offsets[nrays-1] + kept(nrays-1)
  hipLaunchKernelGGL(pack_total_kernel, dim3(1), dim3(1), 0, st, KeptRows{d_nrows, outputper, slots}, (long long)nrays, (long long *)d_offsets);
  if (capacity_rows > 0)
    hipLaunchKernelGGL(pack_rows_kernel, dim3(grid_blocks(nrays, 4)), dim3(256), 0, st, (long long)nrays, (int)slots, d_rows,
                       (const long long *)d_offsets, d_packed, (long long)capacity_rows);
  HIP_OK(hipGetLastError());
  return SRT_OK;
}

// ---- what a packed row set must satisfy: offsets[nrays + 1], rows[offsets[nrays]][SRT_ROW] (layout and curve: srt_rows.hpp) ----
// Said once for every entry point that takes one; `who` is the entry point's name, the prefix of every refusal.
// does [q, q + bytes) lie inside the allocation q points into?  (true when the runtime cannot say)
static bool within_allocation(const void *q, size_t bytes) {
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)q) != hipSuccess) {
    (void)hipGetLastError();
    return true;
  }
  return (const char *)q + bytes <= (const char *)base + size;
}

// Host form: the row set in host memory.  -> offsets[nrays], or -1 with the refusal set (SRT_EINVAL)
static int64_t packed_rows_host(const char *who, int64_t nrays, const int64_t *offsets, const double *rows) {
  if (nrays < 0) return srt_set_error(-1, "%s: nrays = %lld is negative", who, (long long)nrays);
  if (!offsets) return srt_set_error(-1, "%s: null offsets", who);
  if (offsets[0] != 0) return srt_set_error(-1, "%s: offsets[0] = %lld: the first ray's rows start at 0", who, (long long)offsets[0]);
  for (int64_t r = 0; r < nrays; ++r)
    if (offsets[r + 1] < offsets[r]) return srt_set_error(-1, "%s: offsets decrease at ray %lld", who, (long long)r);
  if (offsets[nrays] > 0 && !rows) return srt_set_error(-1, "%s: null rows", who);
  return offsets[nrays];
}

// Device form, first half: the refusals made before any pointer is looked at, the one device that owns every buffer (`scope` is
// entered there), and room in d_offsets for nrays + 1 entries.  `counter` names d_counter in the refusal (d_count, d_counters).
// An entry point that writes events passes its capacity, and whether an output that capacity needs is null; others pass nullptr.
static int packed_rows_device(const char *who, int64_t nrays, const int64_t *d_offsets, const void *d_counter, const char *counter,
                              const int64_t *capacity, bool null_output, const void *const *ptrs, int nptrs, DeviceScope &scope) {
  if (nrays < 0) return srt_set_error(SRT_EINVAL, "%s: nrays = %lld is negative", who, (long long)nrays);
  if (capacity) {
    if (nrays >= (1ll << 31)) return srt_set_error(SRT_EINVAL, "%s: nrays = %lld: an event names its ray in an int32", who, (long long)nrays);
    if (*capacity < 0) return srt_set_error(SRT_EINVAL, "%s: capacity = %lld is negative", who, (long long)*capacity);
  }
  if (!d_offsets || !d_counter) return srt_set_error(SRT_EINVAL, "%s: null d_offsets or %s", who, counter);
  if (null_output) return srt_set_error(SRT_EINVAL, "%s: capacity = %lld with a null output", who, (long long)*capacity);
  int dev = -1, rc;
  if ((rc = device_of(who, ptrs, nptrs, &dev))) return rc;
  if ((rc = scope.enter(dev))) return rc;
  if (!within_allocation(d_offsets, ((size_t)nrays + 1) * sizeof(int64_t)))
    return srt_set_error(SRT_EINVAL, "%s: d_offsets has no room for nrays + 1 = %lld entries", who, (long long)nrays + 1);
  return SRT_OK;
}

// Device form, second half: total = offsets[nrays] as the entry point fetched it (each decides when that 8-byte copy is enqueued
// and waited for).  -> nullptr, or what is wrong with it: the refusal reads "<who>: offsets[nrays] = <total> <this>"
static const char *packed_total_refusal(long long total, const double *d_rows) {
  if (total < 0) return "is negative";
  if (total >= (1ll << 31) - 1) return "rows are too many for one call (2^31 - 2 at most)";
  if (total >= 2 && !d_rows) return "rows, and d_rows is null";
  if (total >= 2 && !within_allocation(d_rows, (size_t)total * SRT_ROW * sizeof(double))) return "rows, more than the allocation of d_rows holds";
  return nullptr;
}

// ---- surface crossings along packed rows (kernels and point functions: srt_crossings.hpp) ----
extern "C" int srt_crossings_device(int nsurf, const srt_surface *surfaces, int64_t nrays, const int64_t *d_offsets,
                                    const double *d_rows, double *d_event_rows, int32_t *d_event_meta, int64_t capacity,
                                    int64_t *d_count, void *stream) {
  namespace cx = srt::crossings;
  cx::Surfaces S;
  char why[200];
  if (cx::prepare(nsurf, surfaces, &S, why, sizeof why)) return srt_set_error(SRT_EINVAL, "srt_crossings_device: %s", why);
  const void *ptrs[5] = {d_offsets, d_count, d_rows, capacity > 0 ? (const void *)d_event_rows : nullptr,
                         capacity > 0 ? (const void *)d_event_meta : nullptr};
  DeviceScope scope;
  // (an event call: its capacity is judged, and a null output that capacity needs is refused in its place in the order)
  int rc = packed_rows_device("srt_crossings_device", nrays, d_offsets, d_count, "d_count", &capacity,
                              capacity > 0 && (!d_event_rows || !d_event_meta), ptrs, 5, scope);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  // the one thing the host has to know: how many rows there are
  long long total = 0;
  HIP_OK(hipMemcpyAsync(&total, d_offsets + nrays, sizeof total, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  if (const char *refuse = packed_total_refusal(total, d_rows))
    return srt_set_error(SRT_EINVAL, "srt_crossings_device: offsets[nrays] = %lld %s", total, refuse);
  if (total < 2) { // no interval
    HIP_OK(hipMemsetAsync(d_count, 0, sizeof(int64_t), st));
    return SRT_OK;
  }
  if (capacity > 0 && (!within_allocation(d_event_rows, (size_t)capacity * SRT_ROW * sizeof(double)) ||
                       !within_allocation(d_event_meta, (size_t)capacity * 4 * sizeof(int32_t))))
    return srt_set_error(SRT_EINVAL, "srt_crossings_device: an output has no room for capacity = %lld events", (long long)capacity);
  // scratch on the stream: mask[total] (2 B a row), evoff[total + 1] (8 B a row), the scan's own
  static_assert(sizeof(long long) == sizeof(int64_t), "int64");
  uint16_t *mask = nullptr;
  long long *evoff = nullptr;
  void *tmp = nullptr;
  HIP_OK(hipMallocAsync((void **)&evoff, ((size_t)total + 1) * sizeof(long long), st));
  hipError_t e = hipMallocAsync((void **)&mask, (size_t)total * sizeof(uint16_t), st);
  size_t need = 0;
  auto counts = hipcub::TransformInputIterator<long long, cx::MaskCount, hipcub::CountingInputIterator<long long>>(
      hipcub::CountingInputIterator<long long>(0), cx::MaskCount{mask, total});
  if (e == hipSuccess) e = hipcub::DeviceScan::ExclusiveSum(nullptr, need, counts, evoff, (int)(total + 1), st);
  if (e == hipSuccess) e = hipMallocAsync(&tmp, need ? need : 16, st);
  if (e == hipSuccess) {
    const unsigned blocks = grid_blocks(total, 256);
    hipLaunchKernelGGL(cx::crossings_count_kernel, dim3(blocks), dim3(256), 0, st, S, (long long)nrays,
                       (const long long *)d_offsets, total, d_rows, mask);
    e = hipcub::DeviceScan::ExclusiveSum(tmp, need, counts, evoff, (int)(total + 1), st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_count, evoff + total, sizeof(int64_t), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess && capacity > 0)
      hipLaunchKernelGGL(cx::crossings_fill_kernel, dim3(blocks), dim3(256), 0, st, S, (long long)nrays,
                         (const long long *)d_offsets, total, d_rows, (const uint16_t *)mask, (const long long *)evoff,
                         (long long)capacity, d_event_rows, d_event_meta);
    if (e == hipSuccess) e = hipGetLastError();
  }
  // (also on the error path)
  if (tmp) (void)hipFreeAsync(tmp, st);
  if (mask) (void)hipFreeAsync(mask, st);
  (void)hipFreeAsync(evoff, st);
  HIP_OK(e);
  return SRT_OK;
}

// device buffer -> a malloc'd host array of n elements, the caller's to srt_free; on an error *out stays null
template <class T>
static hipError_t download(T **out, const T *d, size_t n) {
  T *h = (T *)malloc(n * sizeof(T));
  const hipError_t e = h ? hipMemcpy(h, d, n * sizeof(T), hipMemcpyDeviceToHost) : hipErrorOutOfMemory;
  if (e == hipSuccess) *out = h;
  else free(h);
  return e;
}

// a packed row set goes up: rows[total][SRT_ROW] and offsets[nrays + 1]
static int upload_packed(int64_t nrays, const int64_t *offsets, const double *rows, int64_t total, DevBuf<int64_t> &d_off,
                         DevBuf<double> &d_rows) {
  const int rc = upload(d_rows, rows, (size_t)total * SRT_ROW);
  if (rc) return rc;
  HIP_OK(d_off.alloc((size_t)nrays + 1));
  HIP_OK(hipMemcpy(d_off.p, offsets, ((size_t)nrays + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  return SRT_OK;
}

// The host form of an entry point that writes events: the row set is judged and goes up, a count-only call says how many events
// there are, a second call fills room for exactly that many, and they come down into malloc'd arrays -- all of them, or none.
// device_call(d_offsets, d_rows, d_event_rows, d_event_meta, d_event_dist, capacity, d_count) is the entry point's device form;
// event_dist is null where the events carry no distance.  The caller has looked at its own arguments and outputs.
template <class DeviceCall>
static int host_events(const char *who, int64_t nrays, const int64_t *offsets, const double *rows, DeviceCall device_call,
                       int64_t *nevents, double **event_rows, int32_t **event_meta, double **event_dist) {
  *nevents = 0;
  *event_rows = nullptr;
  *event_meta = nullptr;
  if (event_dist) *event_dist = nullptr;
  const int64_t total = packed_rows_host(who, nrays, offsets, rows);
  if (total < 0) return SRT_EINVAL;
  DeviceScope srt_iscope_;
  int rc = srt_iscope_.enter_default();
  if (rc) return rc;
  if (total < 2) return SRT_OK;
  DevBuf<double> d_rows, d_ev, d_dist;
  DevBuf<int64_t> d_off, d_count;
  DevBuf<int32_t> d_meta;
  if ((rc = upload_packed(nrays, offsets, rows, total, d_off, d_rows))) return rc;
  HIP_OK(d_count.alloc(1));
  if ((rc = device_call(d_off.p, d_rows.p, nullptr, nullptr, nullptr, 0, d_count.p))) return rc;
  int64_t n = 0;
  HIP_OK(hipMemcpy(&n, d_count.p, sizeof n, hipMemcpyDeviceToHost));
  if (n == 0) return SRT_OK;
  HIP_OK(d_ev.alloc((size_t)n * SRT_ROW));
  HIP_OK(d_meta.alloc((size_t)n * 4));
  if (event_dist) HIP_OK(d_dist.alloc((size_t)n));
  if ((rc = device_call(d_off.p, d_rows.p, d_ev.p, d_meta.p, d_dist.p, n, d_count.p))) return rc;
  HIP_OK(hipDeviceSynchronize());
  double *er = nullptr, *ed = nullptr;
  int32_t *em = nullptr;
  hipError_t e = download(&er, d_ev.p, (size_t)n * SRT_ROW);
  if (e == hipSuccess) e = download(&em, d_meta.p, (size_t)n * 4);
  if (e == hipSuccess && event_dist) e = download(&ed, d_dist.p, (size_t)n);
  if (e != hipSuccess) {
    free(er);
    free(em);
    return srt_set_error(e == hipErrorOutOfMemory ? SRT_ENOMEM : SRT_EDEVICE, "%s: %lld events: %s", who, (long long)n, hipGetErrorString(e));
  }
  *nevents = n;
  *event_rows = er;
  *event_meta = em;
  if (event_dist) *event_dist = ed;
  return SRT_OK;
}

extern "C" int srt_crossings(int nsurf, const srt_surface *surfaces, int64_t nrays, const int64_t *offsets, const double *rows,
                             int64_t *nevents, double **event_rows, int32_t **event_meta) {
  srt::crossings::Surfaces S;
  char why[200];
  if (srt::crossings::prepare(nsurf, surfaces, &S, why, sizeof why)) return srt_set_error(SRT_EINVAL, "srt_crossings: %s", why);
  if (!nevents || !event_rows || !event_meta) return srt_set_error(SRT_EINVAL, "srt_crossings: null output");
  return host_events(
      "srt_crossings", nrays, offsets, rows,
      [&](const int64_t *d_off, const double *d_rows, double *d_ev, int32_t *d_meta, double *, int64_t capacity, int64_t *d_count) {
        return srt_crossings_device(nsurf, surfaces, nrays, d_off, d_rows, d_ev, d_meta, capacity, d_count, nullptr);
      },
      nevents, event_rows, event_meta, nullptr);
}

// ---- closest approaches to observer points along packed rows (kernels and point functions: srt_approaches.hpp) ----
extern "C" int srt_approaches_device(int nobs, const srt_observer *observers, int64_t nrays, const int64_t *d_offsets,
                                     const double *d_rows, double *d_event_rows, int32_t *d_event_meta, double *d_event_dist,
                                     int64_t capacity, int64_t *d_count, void *stream) {
  namespace ap = srt::approaches;
  char why[200];
  if (ap::check_observers(nobs, observers, why, sizeof why)) return srt_set_error(SRT_EINVAL, "srt_approaches_device: %s", why);
  const void *ptrs[6] = {d_offsets, d_count, d_rows, capacity > 0 ? (const void *)d_event_rows : nullptr,
                         capacity > 0 ? (const void *)d_event_meta : nullptr, capacity > 0 ? (const void *)d_event_dist : nullptr};
  DeviceScope scope;
  // (an event call, as srt_crossings_device: capacity, and the three outputs it needs)
  int rc = packed_rows_device("srt_approaches_device", nrays, d_offsets, d_count, "d_count", &capacity,
                              capacity > 0 && (!d_event_rows || !d_event_meta || !d_event_dist), ptrs, 6, scope);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  // the one thing the host has to know: how many rows there are
  long long total = 0;
  HIP_OK(hipMemcpyAsync(&total, d_offsets + nrays, sizeof total, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  if (const char *refuse = packed_total_refusal(total, d_rows))
    return srt_set_error(SRT_EINVAL, "srt_approaches_device: offsets[nrays] = %lld %s", total, refuse);
  if (total < 2) { // no interval
    HIP_OK(hipMemsetAsync(d_count, 0, sizeof(int64_t), st));
    return SRT_OK;
  }
  if (capacity > 0 && (!within_allocation(d_event_rows, (size_t)capacity * SRT_ROW * sizeof(double)) ||
                       !within_allocation(d_event_meta, (size_t)capacity * 4 * sizeof(int32_t)) ||
                       !within_allocation(d_event_dist, (size_t)capacity * sizeof(double))))
    return srt_set_error(SRT_EINVAL, "srt_approaches_device: an output has no room for capacity = %lld events", (long long)capacity);
  // Scratch: the observers, count[total] (4 B a row), evoff[total + 1] (8 B a row), the scan's own.  It is NOT taken from the
  // stream-ordered allocator as the crossings take theirs: with hipMallocAsync / hipFreeAsync here, the second call of a process
  // found recycled blocks and counted no events in 4 of 12 fresh processes on an MI355X (the first call never failed).  Plain
  // allocations, a synchronous copy of the observers, and a wait for the stream before they are freed.
  static_assert(sizeof(long long) == sizeof(int64_t), "int64");
  DevBuf<srt_observer> d_obs;
  DevBuf<uint32_t> count;
  DevBuf<long long> evoff;
  DevBytes tmp;
  HIP_OK(evoff.alloc((size_t)total + 1));
  HIP_OK(count.alloc((size_t)total));
  HIP_OK(d_obs.alloc((size_t)nobs));
  HIP_OK(hipMemcpy(d_obs.p, observers, (size_t)nobs * sizeof(srt_observer), hipMemcpyHostToDevice));
  size_t need = 0;
  auto counts = hipcub::TransformInputIterator<long long, ap::RowCount, hipcub::CountingInputIterator<long long>>(
      hipcub::CountingInputIterator<long long>(0), ap::RowCount{count.p, total});
  HIP_OK(hipcub::DeviceScan::ExclusiveSum(nullptr, need, counts, evoff.p, (int)(total + 1), st));
  HIP_OK(tmp.alloc(need ? need : 16));
  const unsigned blocks = grid_blocks(total, ap::BLOCK);
  const double Cl = srt::rows::light_speed();
  hipLaunchKernelGGL(ap::approaches_kernel<false>, dim3(blocks), dim3(ap::BLOCK), 0, st, Cl, nobs, (const srt_observer *)d_obs.p,
                     (long long)nrays, (const long long *)d_offsets, total, d_rows, count.p, (const long long *)nullptr, 0ll,
                     (double *)nullptr, (int32_t *)nullptr, (double *)nullptr);
  hipError_t e = hipcub::DeviceScan::ExclusiveSum((void *)tmp.p, need, counts, evoff.p, (int)(total + 1), st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_count, evoff.p + total, sizeof(int64_t), hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess && capacity > 0)
    hipLaunchKernelGGL(ap::approaches_kernel<true>, dim3(blocks), dim3(ap::BLOCK), 0, st, Cl, nobs, (const srt_observer *)d_obs.p,
                       (long long)nrays, (const long long *)d_offsets, total, d_rows, count.p, (const long long *)evoff.p,
                       (long long)capacity, d_event_rows, d_event_meta, d_event_dist);
  if (e == hipSuccess) e = hipGetLastError();
  const hipError_t es = hipStreamSynchronize(st); // (also on the error path: the scratch goes away when this returns)
  HIP_OK(e);
  HIP_OK(es);
  return SRT_OK;
}

extern "C" int srt_approaches(int nobs, const srt_observer *observers, int64_t nrays, const int64_t *offsets, const double *rows,
                              int64_t *nevents, double **event_rows, int32_t **event_meta, double **event_dist) {
  namespace ap = srt::approaches;
  char why[200];
  if (ap::check_observers(nobs, observers, why, sizeof why)) return srt_set_error(SRT_EINVAL, "srt_approaches: %s", why);
  if (!nevents || !event_rows || !event_meta || !event_dist) return srt_set_error(SRT_EINVAL, "srt_approaches: null output");
  return host_events(
      "srt_approaches", nrays, offsets, rows,
      [&](const int64_t *d_off, const double *d_rows, double *d_ev, int32_t *d_meta, double *d_dist, int64_t capacity, int64_t *d_count) {
        return srt_approaches_device(nobs, observers, nrays, d_off, d_rows, d_ev, d_meta, d_dist, capacity, d_count, nullptr);
      },
      nevents, event_rows, event_meta, event_dist);
}

// ---- traced rays binned onto a grid (kernel and point functions: srt_binning.hpp) ----
extern "C" int srt_bin_cells(const srt_bin_params *params, int64_t *ncells) {
  namespace bn = srt::binning;
  bn::Grid G;
  std::vector<double> edges(3 * (bn::MAXN + 1));
  char why[200];
  if (bn::prepare(params, &G, edges.data(), why, sizeof why)) return srt_set_error(SRT_EINVAL, "srt_bin_cells: %s", why);
  if (!ncells) return srt_set_error(SRT_EINVAL, "srt_bin_cells: null ncells");
  *ncells = G.ncells;
  return SRT_OK;
}

extern "C" int srt_bin_rays_device(const srt_bin_params *params, int64_t nrays, const int64_t *d_offsets, const double *d_rows,
                                   const double *d_rowweight, const double *d_rayweight, int64_t *d_ticks, int64_t *d_hits,
                                   int64_t *d_counters, void *stream) {
  namespace bn = srt::binning;
  bn::Grid G;
  std::vector<double> edges(3 * (bn::MAXN + 1));
  char why[200];
  if (bn::prepare(params, &G, edges.data(), why, sizeof why)) return srt_set_error(SRT_EINVAL, "srt_bin_rays_device: %s", why);
  if (!d_ticks && !d_hits) return srt_set_error(SRT_EINVAL, "srt_bin_rays_device: both outputs (d_ticks and d_hits) are null");
  const void *ptrs[7] = {d_offsets, d_counters, d_rows, d_rowweight, d_rayweight, d_ticks, d_hits};
  DeviceScope scope;
  // (no events: no capacity to judge, no output that depends on one)
  int rc = packed_rows_device("srt_bin_rays_device", nrays, d_offsets, d_counters, "d_counters", nullptr, false, ptrs, 7, scope);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (!within_allocation(d_counters, 4 * sizeof(int64_t)) || (d_ticks && !within_allocation(d_ticks, (size_t)G.ncells * sizeof(int64_t))) ||
      (d_hits && !within_allocation(d_hits, (size_t)G.ncells * sizeof(int64_t))))
    return srt_set_error(SRT_EINVAL, "srt_bin_rays_device: an output has no room for %lld cells (or d_counters for 4 counters)", G.ncells);
  if (d_rayweight && !within_allocation(d_rayweight, (size_t)nrays * sizeof(double)))
    return srt_set_error(SRT_EINVAL, "srt_bin_rays_device: d_rayweight has no room for nrays = %lld entries", (long long)nrays);
  // the edges go up in front of the one thing the host has to know, how many rows there are: one wait covers both, and the
  // host copy of the edges is done with when the wait returns
  double *d_edges = nullptr;
  HIP_OK(hipMallocAsync((void **)&d_edges, (size_t)G.nedges * sizeof(double), st));
  long long total = 0;
  hipError_t e = hipMemcpyAsync(d_edges, edges.data(), (size_t)G.nedges * sizeof(double), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(&total, d_offsets + nrays, sizeof total, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  const char *refuse = nullptr;
  if (e == hipSuccess) {
    refuse = packed_total_refusal(total, d_rows);
    if (!refuse && total >= 2 && d_rowweight && !within_allocation(d_rowweight, (size_t)total * sizeof(double))) refuse = "rows, more than the allocation of d_rowweight holds";
  }
  if (e == hipSuccess && !refuse && total >= 2) {
    static_assert(sizeof(long long) == sizeof(int64_t) && sizeof(unsigned long long) == sizeof(int64_t), "int64");
    const unsigned blocks = bn::launch_blocks(G, total);
    const size_t lds = bn::lds_bytes(G);
    if (G.ncells <= bn::LDS_CELLS)
      hipLaunchKernelGGL(bn::bin_kernel<true>, dim3(blocks), dim3(bn::BLOCK), lds, st, G, (const double *)d_edges, (long long)nrays,
                         (const long long *)d_offsets, total, d_rows, d_rowweight, d_rayweight, (unsigned long long *)d_ticks,
                         (unsigned long long *)d_hits, (unsigned long long *)d_counters);
    else
      hipLaunchKernelGGL(bn::bin_kernel<false>, dim3(blocks), dim3(bn::BLOCK), lds, st, G, (const double *)d_edges, (long long)nrays,
                         (const long long *)d_offsets, total, d_rows, d_rowweight, d_rayweight, (unsigned long long *)d_ticks,
                         (unsigned long long *)d_hits, (unsigned long long *)d_counters);
    e = hipGetLastError();
  }
  (void)hipFreeAsync(d_edges, st); // (also on the error path)
  HIP_OK(e);
  if (refuse) return srt_set_error(SRT_EINVAL, "srt_bin_rays_device: offsets[nrays] = %lld %s", total, refuse);
  return SRT_OK;
}

extern "C" int srt_bin_rays(const srt_bin_params *params, int64_t nrays, const int64_t *offsets, const double *rows,
                            const double *rowweight, const double *rayweight, int64_t **ticks, int64_t **hits, int64_t counters[4]) {
  namespace bn = srt::binning;
  bn::Grid G;
  {
    std::vector<double> edges(3 * (bn::MAXN + 1));
    char why[200];
    if (bn::prepare(params, &G, edges.data(), why, sizeof why)) return srt_set_error(SRT_EINVAL, "srt_bin_rays: %s", why);
  }
  if (!ticks && !hits) return srt_set_error(SRT_EINVAL, "srt_bin_rays: both outputs (ticks and hits) are null");
  if (ticks) *ticks = nullptr;
  if (hits) *hits = nullptr;
  if (!counters) return srt_set_error(SRT_EINVAL, "srt_bin_rays: null counters");
  for (int k = 0; k < 4; ++k) counters[k] = 0;
  const int64_t total = packed_rows_host("srt_bin_rays", nrays, offsets, rows);
  if (total < 0) return SRT_EINVAL;
  DeviceScope srt_iscope_;
  int rc = srt_iscope_.enter_default();
  if (rc) return rc;
  const size_t nc = (size_t)G.ncells;
  DevBuf<double> d_rows, d_roww, d_rayw;
  DevBuf<int64_t> d_off, d_out; // d_out: counters[4], ticks[nc], hits[nc]
  HIP_OK(d_out.alloc(4 + 2 * nc));
  HIP_OK(hipMemset(d_out.p, 0, (4 + 2 * nc) * sizeof(int64_t)));
  if (total >= 2) {
    if ((rc = upload_packed(nrays, offsets, rows, total, d_off, d_rows))) return rc;
    if (rowweight && (rc = upload(d_roww, rowweight, (size_t)total))) return rc;
    if (rayweight && (rc = upload(d_rayw, rayweight, (size_t)nrays))) return rc;
    if ((rc = srt_bin_rays_device(params, nrays, d_off.p, d_rows.p, rowweight ? d_roww.p : nullptr, rayweight ? d_rayw.p : nullptr,
                                  ticks ? d_out.p + 4 : nullptr, hits ? d_out.p + 4 + nc : nullptr, d_out.p, nullptr)))
      return rc;
    HIP_OK(hipDeviceSynchronize());
  }
  int64_t *ht = nullptr, *hh = nullptr;
  hipError_t e = hipMemcpy(counters, d_out.p, 4 * sizeof(int64_t), hipMemcpyDeviceToHost);
  if (e == hipSuccess && ticks) e = download(&ht, (const int64_t *)d_out.p + 4, nc);
  if (e == hipSuccess && hits) e = download(&hh, (const int64_t *)d_out.p + 4 + nc, nc);
  if (e != hipSuccess) {
    free(ht);
    free(hh);
    return srt_set_error(e == hipErrorOutOfMemory ? SRT_ENOMEM : SRT_EDEVICE, "srt_bin_rays: %zu cells: %s", nc, hipGetErrorString(e));
  }
  if (ticks) *ticks = ht;
  if (hits) *hits = hh;
  return SRT_OK;
}

// AoS [n][3] -> SoA [3][n]
__global__ void aos_to_soa3(const double *in, double *out, long long n) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    out[i] = in[3 * i];
    out[n + i] = in[3 * i + 1];
    out[2 * n + i] = in[3 * i + 2];
  }
}

extern "C" int srt_trace_batch(srt_model *m, const srt_params *p, int64_t nrays, const double *pos0,
                               const double *dir0, const double *w0, double *rows, int32_t *nrows,
                               int32_t *stopcond, int64_t *accepted_steps) {
  if (!m || !pos0 || !dir0 || !w0 || !rows || !nrows || !stopcond || nrays < 0) return srt_set_error(SRT_EINVAL, "bad argument");
  int rc = check_params(p);
  if (rc) return rc;
  if (nrays == 0) {
    if (accepted_steps) *accepted_steps = 0;
    return SRT_OK;
  }
  SRT_MODEL_SCOPE;
  if ((rc = ensure_model(m))) return rc;
  std::lock_guard<std::mutex> hold(m->io_lock); // the staging below belongs to the model
  const int slots = srt_rows_per_ray(p);
  const size_t nrow_d = (size_t)nrays * slots * SRT_ROW;
  double *a_pos, *a_dir, *s_pos, *s_dir, *dw, *drows;
  int32_t *d_n, *d_s;
  int64_t *d_c;
  const size_t v3 = (size_t)3 * nrays * sizeof(double);
  if ((rc = io_reserve(m, 0, v3, (void **)&a_pos)) || (rc = io_reserve(m, 1, v3, (void **)&a_dir)) || (rc = io_reserve(m, 2, v3, (void **)&s_pos)) ||
      (rc = io_reserve(m, 3, v3, (void **)&s_dir)) || (rc = io_reserve(m, 4, (size_t)nrays * sizeof(double), (void **)&dw)) ||
      (rc = io_reserve(m, 5, nrow_d * sizeof(double), (void **)&drows)) || (rc = io_reserve(m, 6, (size_t)nrays * sizeof(int32_t), (void **)&d_n)) ||
      (rc = io_reserve(m, 7, (size_t)nrays * sizeof(int32_t), (void **)&d_s)) || (rc = io_reserve(m, 8, 4 * sizeof(int64_t), (void **)&d_c)))
    return rc;
  HIP_OK(hipMemcpy(a_pos, pos0, v3, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(a_dir, dir0, v3, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(dw, w0, (size_t)nrays * sizeof(double), hipMemcpyHostToDevice));
  unsigned blocks = (unsigned)((nrays + 255) / 256);
  hipLaunchKernelGGL(aos_to_soa3, dim3(blocks), dim3(256), 0, 0, (const double *)a_pos, s_pos, (long long)nrays);
  hipLaunchKernelGGL(aos_to_soa3, dim3(blocks), dim3(256), 0, 0, (const double *)a_dir, s_dir, (long long)nrays);
  (void)hipMemsetAsync(drows, 0, nrow_d * sizeof(double), 0);
  rc = srt_trace_batch_device(m, p, nrays, s_pos, s_dir, dw, drows, d_n, d_s, d_c, nullptr);
  if (rc == SRT_OK) {
    hipError_t e = hipMemcpy(rows, drows, nrow_d * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(nrows, d_n, nrays * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(stopcond, d_s, nrays * sizeof(int32_t), hipMemcpyDeviceToHost);
    int64_t c[4] = {0, 0, 0, 0};
    if (e == hipSuccess) e = hipMemcpy(c, d_c, sizeof c, hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = srt_set_error(SRT_EDEVICE, "trace kernel failed: %s", hipGetErrorString(e));
    else if (accepted_steps) *accepted_steps = c[1];
  }
  return rc;
}

// ---- the host iterator over the segments of one launch set (srt.h) ----
// this segment's kept rows of every ray, in the form srt_pack_rows_device counts them: a "row count" whose kept rows are the
// ray's kept rows with index in [segment N, (segment + 1) N) -- none for a ray that stopped in an earlier segment
__global__ void segment_rows_kernel(long long nrays, const int32_t *__restrict__ nrows, int outputper, int slots, int N, int segment,
                                    int32_t *__restrict__ segn) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nrays) return;
  const int32_t n = nrows[i];
  long long k = n > 0 ? (n - 1) / outputper + 1 : 0;
  if (k > slots) k = slots;
  k -= (long long)segment * N;
  if (k > N) k = N;
  segn[i] = k > 0 ? (int32_t)((k - 1) * outputper + 1) : 0;
}

struct srt_trace_run {
  srt_model *m = nullptr;
  int device = 0;
  srt_params p{};
  int64_t nrays = 0, nq = 0; // nq: rays the next segment works on
  int32_t N = 0, nseg = 0, seg = 0;
  DevBuf<double> pos, dir, w, state, rows, packed;
  DevBuf<int32_t> nrows, stop, queue, segn, count;
  DevBuf<int64_t> offsets, counters;
  // host side: the next segment's queue, and what *seg of the last srt_trace_run_next points into
  std::vector<int32_t> hq, ray, h_nrows, h_stop, all_nrows, all_stop;
  std::vector<int64_t> h_off, all_off;
  std::vector<double> h_rows;
};

extern "C" int srt_trace_run_open(srt_model *m, const srt_params *p, int64_t nrays, const double *pos0, const double *dir0,
                                  const double *w0, int32_t segment_rows, srt_trace_run **run) {
  int rc = check_segments(p, nrays, segment_rows);
  if (rc) return rc;
  if (!run) return srt_set_error(SRT_EINVAL, "null argument");
  *run = nullptr;
  {
    DeviceScope probe; // without a GPU there is nothing to trace with, and the call says so before it looks at the model
    if ((rc = probe.enter_default())) return rc;
  }
  if (!m) return srt_set_error(SRT_EINVAL, "null model");
  if (nrays > 0 && (!pos0 || !dir0 || !w0)) return srt_set_error(SRT_EINVAL, "null argument");
  SRT_MODEL_SCOPE;
  if ((rc = ensure_model(m))) return rc;
  std::unique_ptr<srt_trace_run> r(new srt_trace_run);
  r->m = m;
  r->device = m->device;
  r->p = *p;
  r->nrays = r->nq = nrays;
  r->N = segment_rows;
  r->nseg = srt_trace_segments(p, segment_rows);
  if (nrays > 0) {
    const size_t n = (size_t)nrays, nrow = n * (size_t)segment_rows * SRT_ROW;
    DevBuf<double> aos;
    hipError_t e = aos.alloc(3 * n);
    if (e == hipSuccess) e = r->pos.alloc(3 * n);
    if (e == hipSuccess) e = r->dir.alloc(3 * n);
    if (e == hipSuccess) e = r->w.alloc(n);
    if (e == hipSuccess) e = r->state.alloc(n * SRT_STATE);
    if (e == hipSuccess) e = r->rows.alloc(nrow);
    if (e == hipSuccess) e = r->packed.alloc(nrow);
    if (e == hipSuccess) e = r->nrows.alloc(n);
    if (e == hipSuccess) e = r->stop.alloc(n);
    if (e == hipSuccess) e = r->queue.alloc(n);
    if (e == hipSuccess) e = r->segn.alloc(n);
    if (e == hipSuccess) e = r->count.alloc(1);
    if (e == hipSuccess) e = r->offsets.alloc(n + 1);
    if (e == hipSuccess) e = r->counters.alloc(4);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return srt_set_error(SRT_ENOMEM, "segmented trace of %lld rays, %d rows per segment: %s", (long long)nrays, (int)segment_rows,
                           hipGetErrorString(e));
    }
    const unsigned blocks = (unsigned)((nrays + 255) / 256);
    HIP_OK(hipMemcpy(aos.p, pos0, 3 * n * sizeof(double), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(aos_to_soa3, dim3(blocks), dim3(256), 0, 0, (const double *)aos.p, r->pos.p, (long long)nrays);
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(aos.p, dir0, 3 * n * sizeof(double), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(aos_to_soa3, dim3(blocks), dim3(256), 0, 0, (const double *)aos.p, r->dir.p, (long long)nrays);
    HIP_OK(hipMemcpy(r->w.p, w0, n * sizeof(double), hipMemcpyHostToDevice));
    HIP_OK(hipDeviceSynchronize());
  }
  *run = r.release();
  return SRT_OK;
}

extern "C" int srt_trace_run_next(srt_trace_run *r, srt_segment *seg) {
  if (!r || !seg) return srt_set_error(SRT_EINVAL, "null argument");
  memset(seg, 0, sizeof *seg);
  if (r->seg >= r->nseg || r->nq == 0) return 0; // the bound of the loop, and a segment with no rays
  DeviceScope scope;
  int rc = scope.enter(r->device);
  if (rc) return rc;
  const int64_t n = r->nrays, nq = r->nq;
  const int32_t s = r->seg, per = r->p.outputper < 1 ? 1 : r->p.outputper;
  if ((rc = srt_trace_segment_device(r->m, &r->p, n, r->pos.p, r->dir.p, r->w.p, r->N, s, s > 0 ? r->queue.p : nullptr, nq, r->state.p,
                                     r->rows.p, r->nrows.p, r->stop.p, r->counters.p, nullptr)))
    return rc;
  hipLaunchKernelGGL(segment_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, (long long)n, (const int32_t *)r->nrows.p, (int)per,
                     (int)srt_rows_per_ray(&r->p), (int)r->N, (int)s, r->segn.p);
  if ((rc = srt_pack_rows_device(r->N, per, n, r->rows.p, r->segn.p, r->offsets.p, r->packed.p, n * (int64_t)r->N, nullptr))) return rc;
  // (the launch has read its queue by the time the compaction overwrites it: one stream)
  if ((rc = srt_running_rays_device(n, r->stop.p, r->queue.p, r->count.p, nullptr))) return rc;
  r->all_off.resize((size_t)n + 1);
  r->all_nrows.resize((size_t)n);
  r->all_stop.resize((size_t)n);
  int64_t c[4] = {0, 0, 0, 0};
  int32_t next_nq = 0;
  hipError_t e = hipMemcpy(r->all_off.data(), r->offsets.p, ((size_t)n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(r->all_nrows.data(), r->nrows.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(r->all_stop.data(), r->stop.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(c, r->counters.p, sizeof c, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(&next_nq, r->count.p, sizeof next_nq, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return srt_set_error(SRT_EDEVICE, "trace segment %d failed: %s", (int)s, hipGetErrorString(e));
  const int64_t total = r->all_off[(size_t)n];
  if (total < 0 || total > n * (int64_t)r->N) return srt_set_error(SRT_EDEVICE, "trace segment %d: %lld packed rows for room of %lld", (int)s, (long long)total, (long long)(n * (int64_t)r->N));
  r->h_rows.resize((size_t)total * SRT_ROW);
  if (total > 0) HIP_OK(hipMemcpy(r->h_rows.data(), r->packed.p, (size_t)total * SRT_ROW * sizeof(double), hipMemcpyDeviceToHost));
  // the rays that ran: all of them in segment 0, else the queue the previous call brought back.  Rays outside the queue keep
  // no row in this segment, so the offsets of the whole set, read at the queue's ids, are the queue's own prefix sums.
  r->ray.resize((size_t)nq);
  r->h_off.resize((size_t)nq + 1);
  r->h_nrows.resize((size_t)nq);
  r->h_stop.resize((size_t)nq);
  for (int64_t i = 0; i < nq; ++i) {
    const int32_t id = s > 0 ? r->hq[(size_t)i] : (int32_t)i;
    r->ray[(size_t)i] = id;
    r->h_off[(size_t)i] = r->all_off[(size_t)id];
    r->h_nrows[(size_t)i] = r->all_nrows[(size_t)id];
    r->h_stop[(size_t)i] = r->all_stop[(size_t)id];
  }
  r->h_off[(size_t)nq] = total;
  r->hq.resize((size_t)next_nq);
  if (next_nq > 0) HIP_OK(hipMemcpy(r->hq.data(), r->queue.p, (size_t)next_nq * sizeof(int32_t), hipMemcpyDeviceToHost));
  r->nq = next_nq;
  r->seg = s + 1;
  seg->segment = s;
  seg->nrays = nq;
  seg->ray = r->ray.data();
  seg->offsets = r->h_off.data();
  seg->rows = r->h_rows.data();
  seg->nrows = r->h_nrows.data();
  seg->stopcond = r->h_stop.data();
  seg->accepted_steps = c[1];
  return 1;
}

extern "C" void srt_trace_run_close(srt_trace_run *r) {
  if (!r) return;
  DeviceScope scope;
  (void)scope.enter(r->device); // the buffers are freed on the device they live on
  delete r;
}
