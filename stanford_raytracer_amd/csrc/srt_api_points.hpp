// srt_api_points.hpp -- the entry points that evaluate something at n given points, host arrays in and out: plasma parameters,
// the dispersion relation, a field line's foot, handedness, the gradients, one Runge-Kutta step (kernels: srt_kernels.hpp).
// A part of srt_api.hip (srt_api_core.hpp).
#pragma once
#include "srt_api_core.hpp"
#include "srt_api_model.hpp"
#include "srt_kernels.hpp"
#include "srt_at64thch.hpp"

// ------------------------------------------------------------------------------------------ per-point entry points
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
