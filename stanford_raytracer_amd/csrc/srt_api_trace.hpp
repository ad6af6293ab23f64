// srt_api_trace.hpp -- the hot path's host side: the checks on srt_params, the launch-cell ray order, a launch's scratch slot,
// trace_launch (the one launch path of the trace kernels, srt_kernels.hpp) behind the device-buffer entry points, whole and in
// segments, the queue of running rays, launch timing, the host-buffer entry point srt_trace_batch, and the host iterator over
// the segments of one launch set (srt_trace_run_*).  upload_soa3 is the one AoS -> SoA upload of the two host-buffer entry points.
// A part of srt_api.hip (srt_api_core.hpp).
#pragma once
#include "srt_api_core.hpp"
#include "srt_api_model.hpp"
#include "srt_kernels.hpp"
#include <hipcub/hipcub.hpp>

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
static_assert(SRT_STASH_STATS == STASH_STATS, "srt.h and srt_tail_stash.hpp disagree on the stash statistics");

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
  // SRT_MAX_BLOCKS=n caps the persistent grid (an experiment and test switch like the two above: a few hundred rays then queue
  // up behind a handful of waves)
  if (const char *e = getenv("SRT_MAX_BLOCKS")) {
    const long long v = atoll(e);
    if (v >= 1 && grid > v) grid = v;
  }
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
      (rc = slot_scratch(m, sl, sl.stage, grid, (size_t)ScatteredModel::REC_CAP * ScatteredModel::REC, "the scattered model's staging records", &a.scratch)))
    return rc;
  if (m->kind == KIND_SCATTERED && a.scratch != nullptr && blocks_enabled() &&
      (rc = slot_scratch(m, sl, sl.cand, grid, ScatteredModel::BLOCK_DOUBLES, "the scattered model's candidate blocks", &a.scratch2)))
    return rc;
  // Tail stash of the unsegmented interp kernels (srt_tail_stash.hpp): a block of the slot's scratch per wave; a refused
  // allocation means a launch without banking.  SRT_TAIL_STASH=n caps the quota of every mark at n records; 0 = no banking.
  TraceStashArgs sa;
  sa.stash = nullptr;
  sa.stats = nullptr;
  lt.stashed = false;
  {
    int quota_cap = -1;
    if (const char *e = getenv("SRT_TAIL_STASH")) quota_cap = atoi(e) < 0 ? 0 : atoi(e);
    const bool traits = !sg && (m->kind == KIND_INTERP || m->kind == KIND_INTERP_NODES);
    sa.sp = stash_policy(p->maxsteps, traits ? nwork : 0, grid * cap, quota_cap);
    const int per_wave = stash_total_quota(sa.sp);
    if (per_wave > 0) {
      const size_t need = (size_t)grid * (size_t)per_wave * STASH_REC;
      if (sl.stash.buf.cap < need) sl.stash.blocks = 0; // (the block per wave grew with the quota: what is held counts for nothing)
      if ((rc = slot_scratch(m, sl, sl.stash, grid, (size_t)per_wave * STASH_REC, "the interp model's tail stash", &sa.stash))) return rc;
      if (sa.stash != nullptr && sl.stash.buf.cap >= need) {
        sa.stats = lt.stats.p;
        lt.stashed = true;
        HIP_OK(hipMemsetAsync(sa.stats, 0, STASH_STATS * sizeof(unsigned long long), st));
      } else {
        sa.stash = nullptr;
        sa.sp = stash_policy(p->maxsteps, 0, 0, 0);
      }
    }
  }
  const bool fixed = p->fixedstep != 0;
  const int fopt = m->cm.fld.use_tsy != 0 ? 2 : (m->cm.fld.use_igrf != 0 ? 1 : 0);
  // one instantiation per (model, integrator, field option): the dipole kernels carry none of the IGRF code, the
  // IGRF-alone kernels none of the T04 call sites
  rc = with_model(m, [&](auto tag) -> int {
    using T = decltype(tag);
    using M = typename T::Model;
    auto pick = [&](auto seg) { // (its segmented twin beside every kernel)
      constexpr bool SEG = decltype(seg)::value;
      auto launch = [&](auto kernel) {
        if constexpr (!SEG && tail_stash<M>()) {
          static_cast<TraceArgs &>(sa) = a; // (the TraceArgs part of `a`)
          hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(WAVE), 0, st, m->on_device<M>(), m->d_common.p, sa);
        } else
          hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(WAVE), 0, st, m->on_device<M>(), m->d_common.p, a);
      };
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
  return with_cub_temp(st, [&](void *tmp, size_t &bytes) {
    return hipcub::DeviceSelect::Flagged(tmp, bytes, ids, flags, d_queue, d_count, (int)nrays, st);
  });
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

extern "C" int srt_launch_stash_stats(srt_model *m, int back, int64_t *stats) {
  if (!m || !stats) return srt_set_error(SRT_EINVAL, "null argument");
  if (back < 0 || back >= srt_model::NHIST || m->last_hist < 0) return srt_set_error(SRT_EINVAL, "no such launch");
  srt_model::LaunchTimes &lt = m->hist[(m->last_hist - back + srt_model::NHIST) % srt_model::NHIST];
  if (!lt.used) return srt_set_error(SRT_EINVAL, "no such launch");
  for (int i = 0; i < SRT_STASH_STATS; ++i) stats[i] = 0;
  if (!lt.stashed) return SRT_OK; // a launch without banking
  SRT_MODEL_SCOPE;
  int rc = ensure_model(m);
  if (rc) return rc;
  HIP_OK(hipEventSynchronize(lt.ev1));
  HIP_OK(hipMemcpy(stats, lt.stats.p, SRT_STASH_STATS * sizeof(int64_t), hipMemcpyDeviceToHost));
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
// a host array [n][3] goes up into `aos` and from there, transposed, into `soa`: a copy and a launch on the null stream, no wait
// (a caller that reuses `aos` waits before it does)
static int upload_soa3(const double *h, double *aos, double *soa, int64_t n) {
  HIP_OK(hipMemcpy(aos, h, (size_t)3 * n * sizeof(double), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(aos_to_soa3, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, (const double *)aos, soa, (long long)n);
  return SRT_OK;
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
  if ((rc = upload_soa3(pos0, a_pos, s_pos, nrays)) || (rc = upload_soa3(dir0, a_dir, s_dir, nrays))) return rc;
  HIP_OK(hipMemcpy(dw, w0, (size_t)nrays * sizeof(double), hipMemcpyHostToDevice));
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
    if ((rc = upload_soa3(pos0, aos.p, r->pos.p, nrays))) return rc;
    HIP_OK(hipDeviceSynchronize()); // (one AoS buffer serves both: the positions are out of it before the directions go in)
    if ((rc = upload_soa3(dir0, aos.p, r->dir.p, nrays))) return rc;
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
