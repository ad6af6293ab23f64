// srt_api_rows.hpp -- what is done with traced rows: hot-plasma damping along them (srt_damping.hpp), packing the rows a ray
// kept (srt_pack_rows_device), what a packed row set must satisfy, said once for every entry point that takes one, and the four
// post-processors of packed rows: surface crossings (srt_crossings.hpp), closest approaches (srt_approaches.hpp), ray-tube
// sections (srt_tubes.hpp), binning onto a grid (srt_binning.hpp).  The device forms share fetch_packed_total and
// packed_total_refused; the two event calls also event_rows_total and event_outputs_fit.
// A part of srt_api.hip (srt_api_core.hpp).
#pragma once
#include "srt_api_core.hpp"
#include "srt_damping.hpp"
#include "srt_rows.hpp"
#include "srt_crossings.hpp"
#include "srt_binning.hpp"
#include "srt_approaches.hpp"
#include "srt_tubes.hpp"
#include <hipcub/hipcub.hpp>

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
  if ((rc = with_cub_temp(st, [&](void *tmp, size_t &bytes) {
         return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, counts, (long long *)d_offsets, (int)nrays, st);
       })))
    return rc;
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
static int packed_total_refused(const char *who, long long total, const char *refuse) { return srt_set_error(SRT_EINVAL, "%s: offsets[nrays] = %lld %s", who, total, refuse); }
// the one thing the host has to know, how many rows there are: an 8-byte copy behind the work on `st`, and a wait for it
static int fetch_packed_total(int64_t nrays, const int64_t *d_offsets, hipStream_t st, long long *total) {
  HIP_OK(hipMemcpyAsync(total, d_offsets + nrays, sizeof *total, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  return SRT_OK;
}
// The front of an event call's device form behind packed_rows_device: the total, its refusal, and -- fewer than two rows make no
// interval -- a count of zero.  The caller goes on only when this answers SRT_OK with *total >= 2.
static int event_rows_total(const char *who, int64_t nrays, const int64_t *d_offsets, const double *d_rows, int64_t *d_count,
                            hipStream_t st, long long *total) {
  if (const int rc = fetch_packed_total(nrays, d_offsets, st, total)) return rc;
  if (const char *refuse = packed_total_refusal(*total, d_rows)) return packed_total_refused(who, *total, refuse);
  if (*total < 2) HIP_OK(hipMemsetAsync(d_count, 0, sizeof(int64_t), st));
  return SRT_OK;
}
// ... and the room its outputs have for `capacity` events of so many bytes each
static int event_outputs_fit(const char *who, int64_t capacity, std::initializer_list<std::pair<const void *, size_t>> outputs) {
  for (const auto &o : outputs)
    if (capacity > 0 && !within_allocation(o.first, (size_t)capacity * o.second))
      return srt_set_error(SRT_EINVAL, "%s: an output has no room for capacity = %lld events", who, (long long)capacity);
  return SRT_OK;
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
  long long total = 0;
  if ((rc = event_rows_total("srt_crossings_device", nrays, d_offsets, d_rows, d_count, st, &total)) || total < 2) return rc;
  if ((rc = event_outputs_fit("srt_crossings_device", capacity, {{d_event_rows, SRT_ROW * sizeof(double)}, {d_event_meta, 4 * sizeof(int32_t)}}))) return rc;
  // Scratch: mask[total] (2 B a row), evoff[total + 1] (8 B a row), the scan's own.  Plain allocations and a wait for the stream
  // before they are freed, as srt_approaches_device below and for its reason: this call comes in pairs (count, then fill), and
  // with hipMallocAsync / hipFreeAsync the second call of a process found recycled blocks -- a tool-mode run of the executable
  // once wrote its events' metadata as zeros, with the right count.
  static_assert(sizeof(long long) == sizeof(int64_t), "int64");
  DevBuf<uint16_t> mask;
  DevBuf<long long> evoff;
  DevBytes tmp;
  HIP_OK(evoff.alloc((size_t)total + 1));
  HIP_OK(mask.alloc((size_t)total));
  size_t need = 0;
  auto counts = hipcub::TransformInputIterator<long long, cx::MaskCount, hipcub::CountingInputIterator<long long>>(
      hipcub::CountingInputIterator<long long>(0), cx::MaskCount{mask.p, total});
  HIP_OK(hipcub::DeviceScan::ExclusiveSum(nullptr, need, counts, evoff.p, (int)(total + 1), st));
  HIP_OK(tmp.alloc(need ? need : 16));
  const unsigned blocks = grid_blocks(total, 256);
  hipLaunchKernelGGL(cx::crossings_count_kernel, dim3(blocks), dim3(256), 0, st, S, (long long)nrays, (const long long *)d_offsets,
                     total, d_rows, mask.p);
  hipError_t e = hipcub::DeviceScan::ExclusiveSum((void *)tmp.p, need, counts, evoff.p, (int)(total + 1), st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_count, evoff.p + total, sizeof(int64_t), hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess && capacity > 0)
    hipLaunchKernelGGL(cx::crossings_fill_kernel, dim3(blocks), dim3(256), 0, st, S, (long long)nrays,
                       (const long long *)d_offsets, total, d_rows, (const uint16_t *)mask.p, (const long long *)evoff.p,
                       (long long)capacity, d_event_rows, d_event_meta);
  if (e == hipSuccess) e = hipGetLastError();
  const hipError_t es = hipStreamSynchronize(st); // (also on the error path: the scratch goes away when this returns)
  HIP_OK(e);
  HIP_OK(es);
  return SRT_OK;
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
  long long total = 0;
  if ((rc = event_rows_total("srt_approaches_device", nrays, d_offsets, d_rows, d_count, st, &total)) || total < 2) return rc;
  if ((rc = event_outputs_fit("srt_approaches_device", capacity, {{d_event_rows, SRT_ROW * sizeof(double)}, {d_event_meta, 4 * sizeof(int32_t)},
                                                                {d_event_dist, sizeof(double)}}))) return rc;
  // Scratch: the observers, count[total] (4 B a row), evoff[total + 1] (8 B a row), the scan's own.  It is NOT taken from the
  // stream-ordered allocator: with hipMallocAsync / hipFreeAsync here, the second call of a process
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

// ---- ray tubes: the section a ray and two neighbours span, at every packed row (kernel and point functions: srt_tubes.hpp) ----
extern "C" int srt_tubes_device(int64_t nrays, const int64_t *neighbours, const int64_t *d_offsets, const double *d_rows,
                                double *d_section, int32_t *d_flag, void *stream) {
  namespace tb = srt::tubes;
  static_assert(sizeof(long long) == sizeof(int64_t), "int64");
  char why[200];
  if (tb::check_neighbours(nrays, (const long long *)neighbours, why, sizeof why)) return srt_set_error(SRT_EINVAL, "srt_tubes_device: %s", why);
  if (!d_section && !d_flag) return srt_set_error(SRT_EINVAL, "srt_tubes_device: both outputs (d_section and d_flag) are null");
  const void *ptrs[4] = {d_offsets, d_rows, d_section, d_flag};
  DeviceScope scope;
  // (no events: no capacity to judge; the output that is there stands where the others pass their counter)
  int rc = packed_rows_device("srt_tubes_device", nrays, d_offsets, d_section ? (const void *)d_section : (const void *)d_flag,
                              "an output", nullptr, false, ptrs, 4, scope);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  long long total = 0;
  if ((rc = fetch_packed_total(nrays, d_offsets, st, &total))) return rc;
  const char *refuse = packed_total_refusal(total, d_rows);
  // (a single row is a centre row here, where the crossings need two for an interval)
  if (!refuse && total == 1 && !d_rows) refuse = "row, and d_rows is null";
  if (!refuse && total == 1 && !within_allocation(d_rows, (size_t)SRT_ROW * sizeof(double))) refuse = "row, more than the allocation of d_rows holds";
  if (refuse) return packed_total_refused("srt_tubes_device", total, refuse);
  if (total == 0) return SRT_OK;
  if ((d_section && !within_allocation(d_section, (size_t)total * 4 * sizeof(double))) ||
      (d_flag && !within_allocation(d_flag, (size_t)total * sizeof(int32_t))))
    return srt_set_error(SRT_EINVAL, "srt_tubes_device: an output has no room for offsets[nrays] = %lld rows", total);
  // the neighbours go up as the approaches' observers do: a plain allocation, a synchronous copy, and a wait for the stream
  // before it is freed
  DevBuf<long long> d_nb;
  HIP_OK(d_nb.alloc(nrays > 0 ? (size_t)nrays * 2 : 2));
  HIP_OK(hipMemcpy(d_nb.p, neighbours, (size_t)nrays * 2 * sizeof(long long), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(tb::tubes_kernel<tb::BLOCK>, dim3(grid_blocks(total, tb::BLOCK)), dim3(tb::BLOCK), 0, st, srt::rows::light_speed(),
                     (long long)nrays, (const long long *)d_offsets, total, d_rows, (const long long *)d_nb.p, d_section, d_flag);
  const hipError_t e = hipGetLastError();
  const hipError_t es = hipStreamSynchronize(st); // (also on the error path: the neighbours go away when this returns)
  HIP_OK(e);
  HIP_OK(es);
  return SRT_OK;
}

extern "C" int srt_tubes(int64_t nrays, const int64_t *neighbours, const int64_t *offsets, const double *rows, double *section,
                         int32_t *flag) {
  char why[200];
  if (srt::tubes::check_neighbours(nrays, (const long long *)neighbours, why, sizeof why)) return srt_set_error(SRT_EINVAL, "srt_tubes: %s", why);
  if (!section && !flag) return srt_set_error(SRT_EINVAL, "srt_tubes: both outputs (section and flag) are null");
  const int64_t total = packed_rows_host("srt_tubes", nrays, offsets, rows);
  if (total < 0) return SRT_EINVAL;
  DeviceScope srt_iscope_;
  int rc = srt_iscope_.enter_default();
  if (rc) return rc;
  if (total == 0) return SRT_OK;
  DevBuf<double> d_rows, d_section;
  DevBuf<int64_t> d_off;
  DevBuf<int32_t> d_flag;
  if ((rc = upload_packed(nrays, offsets, rows, total, d_off, d_rows))) return rc;
  if (section) HIP_OK(d_section.alloc((size_t)total * 4));
  if (flag) HIP_OK(d_flag.alloc((size_t)total));
  if ((rc = srt_tubes_device(nrays, neighbours, d_off.p, d_rows.p, d_section.p, d_flag.p, nullptr))) return rc;
  HIP_OK(hipDeviceSynchronize());
  if (section) HIP_OK(hipMemcpy(section, d_section.p, (size_t)total * 4 * sizeof(double), hipMemcpyDeviceToHost));
  if (flag) HIP_OK(hipMemcpy(flag, d_flag.p, (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost));
  return SRT_OK;
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
  if (refuse) return packed_total_refused("srt_bin_rays_device", total, refuse);
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
