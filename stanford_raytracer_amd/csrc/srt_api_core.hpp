// srt_api_core.hpp -- what every unit of the C ABI's host side stands on: the error text and HIP_OK, DevBuf (the owner of device
// memory), device selection and DeviceScope, struct srt_model, with_model (the one place that turns a kind number into a type),
// SRT_MODEL_SCOPE / ensure_model, and the small helpers of the later units: upload, download, grid_blocks, stride_blocks,
// within_allocation, with_cub_temp.
//
// The srt_api_*.hpp headers are the parts of ONE translation unit, srt_api.hip, and are not for inclusion anywhere else: this
// one owns the names they share at global scope (`using namespace srt;` and the three macros).
#pragma once
#include <hip/hip_runtime.h>

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
#include "srt_models.hpp"
#include "srt_ngo3d.hpp"
#include "srt_scattered.hpp"
#include "srt_interp_nodes.hpp"
#include "srt_simple3d.hpp"
#include "srt_at64thch.hpp"
#include "srt_tail_stash.hpp"

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

// The one owner of device memory in these units: an array of T that frees itself.  alloc() is exact and drops what was held first;
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
    Scratch stash; // interp model: the waves' tail stash (srt_tail_stash.hpp), sum of quotas * STASH_REC doubles per block
    // frees the scratch and forgets refused sizes; the caller has waited for `done` where a launch may still read it
    void release() {
      for (int k = 0; k < 2; ++k) {
        keys[k].release();
        ids[k].release();
      }
      sorttmp.release();
      stage.buf.release();
      cand.buf.release();
      stash.buf.release();
      stage.blocks = stage.failed = cand.blocks = cand.failed = stash.blocks = stash.failed = 0;
    }
  };
  static constexpr int NSLOT = 4;
  LaunchSlot slot[NSLOT];
  int rr_slot = 0;
  // timing history of the last NHIST launches (srt_last_kernel_ms, srt_launch_ms), its own ring: slots are reused out of turn
  struct LaunchTimes {
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool used = false;
    DevBuf<unsigned long long> stats; // [STASH_STATS], written by the launch's waves (srt_launch_stash_stats)
    bool stashed = false;             // that launch banked rays: `stats` is its own
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

static int upload(DevBuf<double> &b, const double *h, size_t n) {
  if (b.alloc(n) != hipSuccess) return srt_set_error(SRT_ENOMEM, "hipMalloc failed");
  HIP_OK(hipMemcpy(b.p, h, n * sizeof(double), hipMemcpyHostToDevice));
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

// the blocks of a grid-stride launch over n items, `per` to a block: ceil(n / per), 65536 at most
static unsigned grid_blocks(long long n, long long per) {
  const long long blocks = (n + per - 1) / per;
  return (unsigned)(blocks < 65536 ? blocks : 65536);
}

// the blocks of 256 threads of a grid-stride launch over n items with the older cap of 65535 * 4 (the interp grids' kernels;
// grid_blocks caps elsewhere and is not this function)
static int stride_blocks(size_t n) {
  const size_t blocks = (n + 255) / 256;
  return (int)(blocks < 65535 * 4 ? blocks : 65535 * 4);
}

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

// Temporary storage around one hipCUB call, from the stream-ordered allocator (the callers sit on the multi-GPU gather's timed
// path): cub(tmp, bytes) is the call; it is asked for its size with tmp = null, then run, and the storage is freed behind it on
// `st`, also on the error path.  (srt_crossings_device and srt_approaches_device keep plain allocations, for their own reason.)
template <class Cub>
static int with_cub_temp(hipStream_t st, Cub &&cub) {
  size_t need = 0;
  HIP_OK(cub((void *)nullptr, need));
  void *tmp = nullptr;
  HIP_OK(hipMallocAsync(&tmp, need ? need : 16, st));
  const hipError_t e = cub(tmp, need);
  const hipError_t ef = hipFreeAsync(tmp, st); // (also on the error path)
  HIP_OK(e);
  HIP_OK(ef);
  return SRT_OK;
}
