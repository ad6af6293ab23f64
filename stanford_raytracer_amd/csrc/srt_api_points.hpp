// srt_api_points.hpp -- the entry points that evaluate something at n given points, host arrays in and out: plasma parameters,
// the dispersion relation, a field line's foot, handedness, the gradients, one Runge-Kutta step (kernels: srt_kernels.hpp).
// point_call / model_point_call are the one shape of such a call, with_stage the scattered model's staging around a launch.
// A part of srt_api.hip (srt_api_core.hpp).
#pragma once
#include "srt_api_core.hpp"
#include "srt_api_model.hpp"
#include "srt_kernels.hpp"
#include "srt_at64thch.hpp"

// ------------------------------------------------------------------------------------------ per-point entry points
// The one shape of a per-point call, after the entry point's own refusals: nothing to do for n == 0; the model's device; the
// inputs go up (in[k].h holds in[k].width doubles a point); width * n doubles of output; run(d, dout) launches on the null
// stream with d[k] the k-th input on the device; the output comes down into out.
struct PointIn {
  const double *h;
  int width;
};
template <class Run>
static int point_call(srt_model *m, int64_t n, std::initializer_list<PointIn> in, int width, double *out, Run &&run) {
  if (n == 0) return SRT_OK;
  SRT_MODEL_SCOPE;
  int rc = ensure_model(m);
  if (rc) return rc;
  DevBuf<double> din[3], dout;
  const double *d[3] = {nullptr, nullptr, nullptr};
  int k = 0;
  for (const PointIn &a : in) {
    if ((rc = upload(din[k], a.h, (size_t)a.width * n))) return rc;
    d[k] = din[k].p;
    ++k;
  }
  if (dout.alloc((size_t)width * n) != hipSuccess) return srt_set_error(SRT_ENOMEM, "hipMalloc failed");
  if ((rc = run(d, dout.p))) return rc;
  HIP_OK(hipMemcpy(out, dout.p, (size_t)width * n * sizeof(double), hipMemcpyDeviceToHost));
  return SRT_OK;
}
// ... with the launch dispatched on the model's kind: launch(tag, d, dout), tag a ModelTag (with_model)
template <class Launch>
static int model_point_call(srt_model *m, int64_t n, std::initializer_list<PointIn> in, int width, double *out, Launch &&launch) {
  return point_call(m, n, in, width, out, [&](const double *const *d, double *dout) -> int {
    return with_model(m, [&](auto tag) -> int { return launch(tag, d, dout); });
  });
}
// the scattered model's staging records around a per-point launch of n points: launch(stage) gets null for every other model
template <class M, class Launch>
static int with_stage(int64_t n, Launch &&launch) {
  DevBuf<double> stage;
  if constexpr (std::is_same<M, ScatteredModel>::value) stage_alloc(stage, n);
  launch(stage.p);
  if constexpr (std::is_same<M, ScatteredModel>::value) HIP_OK(hipDeviceSynchronize()); // `stage` is freed at the end of this scope
  return SRT_OK;
}

extern "C" int srt_plasma_params(srt_model *m, int64_t n, const double *x, double *qs, double *Ns, double *ms,
                                 double *nus, double *B0) {
  if (!m || !x || n < 0) return srt_set_error(SRT_EINVAL, "bad argument");
  std::vector<double> h(19 * n);
  const int rc = model_point_call(m, n, {{x, 3}}, 19, h.data(), [&](auto tag, const double *const *d, double *dout) -> int {
    using T = decltype(tag);
    launch_wave_blocks(params_kernel<typename T::Model, T::lds>, n, 0, m->on_device<typename T::Model>(), m->d_common.p, (long long)n,
                       d[0], dout);
    return SRT_OK;
  });
  if (rc) return rc;
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
  return model_point_call(m, n, {{x, 3}, {k, 3}, {w, 1}}, 10, out, [&](auto tag, const double *const *d, double *dout) -> int {
    using T = decltype(tag);
    launch_wave_blocks(dispersion_kernel<typename T::Model, T::lds>, n, 0, m->on_device<typename T::Model>(), m->d_common.p,
                       (long long)n, d[0], d[1], d[2], dout);
    return SRT_OK;
  });
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
  return point_call(m, n, {{x, 3}}, 6, out, [&](const double *const *d, double *dout) -> int { // (no dispatch: one kernel for every kind)
    launch_wave_blocks(foot_kernel, n, 0, (const Common *)m->d_common.p, m->geopack_psi, (long long)n, d[0], dout);
    return SRT_OK;
  });
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
  return model_point_call(m, n, {{x, 3}, {k, 3}, {w, 1}}, 14, out, [&](auto tag, const double *const *d, double *dout) -> int {
    using T = decltype(tag);
    using M = typename T::Model;
    return with_stage<M>(n, [&](double *stage) {
      launch_wave_blocks(gradients_kernel<M, T::lds>, n, 0, m->on_device<M>(), m->d_common.p, (long long)n, d[0], d[1], d[2], del, dout, stage);
    });
  });
}

extern "C" int srt_rk_step(srt_model *m, int64_t n, const double *args, const double *dt, double del, double *out) {
  if (!m || !args || !dt || !out || n < 0) return srt_set_error(SRT_EINVAL, "bad argument");
  return model_point_call(m, n, {{args, 7}, {dt, 1}}, 21, out, [&](auto tag, const double *const *d, double *dout) -> int {
    using T = decltype(tag);
    using M = typename T::Model;
    return with_stage<M>(n, [&](double *stage) {
      launch_wave_blocks(rkstep_kernel<M, T::lds>, n, 0, m->on_device<M>(), m->d_common.p, (long long)n, d[0], d[1], del, dout, stage);
    });
  });
}
