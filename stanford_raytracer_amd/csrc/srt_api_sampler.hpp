// srt_api_sampler.hpp -- srt_build_samples: the host loop of the random / adaptive sample-set builder around the kernels of
// srt_sampler.hpp and hipCUB's sort and scan.  The call's state is a SmpCall; its pieces are smp_stage (a shell / uniform stage),
// smp_level (one adaptive level), smp_adaptive (the pass loop) and smp_download.  A part of srt_api.hip (srt_api_core.hpp).
#pragma once
#include "srt_api_core.hpp"
#include "srt_sampler.hpp"
#include <hipcub/hipcub.hpp>

// ---- the random / adaptive sample-set builder (kernels and the level-by-level scheme: srt_sampler.hpp) ----
static int smp_eval(srt_model *src, long long n, double *rec) {
  if (n <= 0) return SRT_OK;
  return with_model(src, [&](auto tag) -> int {
    using T = decltype(tag);
    launch_wave_blocks(smp_eval_kernel<typename T::Model, T::lds>, n, 0, src->on_device<typename T::Model>(), n, rec);
    return SRT_OK;
  });
}

static constexpr size_t SMP_RB = SMP_REC * sizeof(double);
struct SmpCall {
  srt_model *src;
  const srt_sampler_params *sp;
  int nspec, ninc;
  SmpBox root;
  int64_t counts[6]; // per stage (srt.h); [3] counts the adaptive samples as the levels add them
  DevBytes pool, slot, stage, valid;
  long long npool = 0;
  std::vector<double> tail; // zero-altitude and ionosphere samples, appended to the output after the pool
};
// a failed device call of the sampler is SRT_EDEVICE whatever the error (HIP_OK: out-of-memory is SRT_ENOMEM), a refused reserve() SRT_ENOMEM
static int smp_ok(hipError_t e, const char *what) { return e == hipSuccess ? SRT_OK : srt_set_error(SRT_EDEVICE, "sampler, %s: %s", what, hipGetErrorString(e)); }
static int smp_mem(int refused) { return refused ? srt_set_error(SRT_ENOMEM, "device allocation failed (sampler)") : SRT_OK; }
// shell and uniform stages share one routine: positions, f(x), then append to the pool (device) or compact into the tail (host)
static int smp_stage(SmpCall &c, int stg, long long n, double rmin, double rmax, bool to_pool, int64_t &count) {
  if (n <= 0) return SRT_OK;
  int rc;
  if ((rc = smp_mem(c.stage.reserve((size_t)n * SMP_RB) || c.valid.reserve((size_t)n * sizeof(int))))) return rc;
  hipLaunchKernelGGL(smp_stage_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, stg, n, (unsigned long long)c.sp->seed, c.root, rmin,
                     rmax, c.stage.as<double>(), c.valid.as<int>());
  if ((rc = smp_eval(c.src, n, c.stage.as<double>())) || (rc = smp_ok(hipDeviceSynchronize(), "stage"))) return rc;
  std::vector<int> hv((size_t)n);
  if ((rc = smp_ok(hipMemcpy(hv.data(), c.valid.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost), "stage flags"))) return rc;
  if (to_pool) {
    for (long long i = 0; i < n; ++i)
      if (!hv[i])
        return srt_set_error(SRT_EINVAL, "radial stage: sample %lld found no point of the shell inside the box in %d attempts", i, SMP_MAXTRY);
    if ((rc = smp_mem(c.pool.reserve((size_t)(c.npool + n) * SMP_RB, (size_t)c.npool * SMP_RB))) ||
        (rc = smp_ok(hipMemcpy(c.pool.as<double>() + (size_t)c.npool * SMP_REC, c.stage.p, (size_t)n * SMP_RB, hipMemcpyDeviceToDevice), "append")))
      return rc;
    c.npool += n;
    count = n;
  } else {
    std::vector<double> hr((size_t)n * SMP_REC);
    if ((rc = smp_ok(hipMemcpy(hr.data(), c.stage.p, (size_t)n * SMP_RB, hipMemcpyDeviceToHost), "stage records"))) return rc;
    for (long long i = 0; i < n; ++i)
      if (hv[i]) {
        for (int q = 0; q < 3 + c.nspec; ++q) c.tail.push_back(hr[(size_t)i * SMP_REC + q]);
        ++count;
      }
  }
  return SRT_OK;
}
// the adaptive stage's scratch, grow-only across levels and passes; `calls` are the boxes of this level, `children` the next one's
struct SmpScratch {
  DevBytes keys0, keys1, idx0, idx1, sorttmp, callsA, callsB, halves, cand, nadd, refine, addA, addoff, childoff, scantmp;
  DevBytes *calls = &callsA, *children = &callsB;
};
// one level of one pass: the pool's samples sorted by half-box, candidates drawn and judged against `tol`, the accepted ones
// appended to the pool, the boxes to refine made the next level's calls (ncalls: in, this level's; out, the next one's)
static int smp_level(SmpCall &c, SmpScratch &w, int pass, int depth, double tol, long long &ncalls) {
  const int dim = depth % 3, ninc = c.ninc;
  const long long nhalf = 2 * ncalls, npool = c.npool, ncand = nhalf * 2 * ninc;
  if (nhalf > (1ll << 26)) return srt_set_error(SRT_EINVAL, "adaptive sampler: %lld half-boxes at depth %d (tolerance too small)", nhalf, depth);
  int rc;
  if ((rc = smp_mem(w.keys0.reserve((size_t)npool * 4 + 4) || w.keys1.reserve((size_t)npool * 4 + 4) || w.idx0.reserve((size_t)npool * 4 + 4) ||
                    w.idx1.reserve((size_t)npool * 4 + 4) || w.halves.reserve((size_t)nhalf * sizeof(SmpBox)) || w.cand.reserve((size_t)ncand * SMP_RB) ||
                    w.nadd.reserve((size_t)nhalf * 4) || w.refine.reserve((size_t)nhalf * 4) || w.addA.reserve((size_t)nhalf * 4) ||
                    w.addoff.reserve((size_t)nhalf * 4) || w.childoff.reserve((size_t)nhalf * 4))))
    return rc;
  if (npool > 0) { // the pool's samples keyed by the half-box they lie in, and sorted by that key (keys1, idx1)
    hipLaunchKernelGGL(smp_keys_kernel, dim3((unsigned)((npool + 255) / 256)), dim3(256), 0, 0, npool, c.pool.as<double>(), c.slot.as<int>(),
                       w.calls->as<SmpBox>(), dim, (unsigned)nhalf, w.keys0.as<unsigned>(), w.idx0.as<int>());
    int bits = 1;
    while ((1ll << bits) <= nhalf) ++bits;
    size_t need = 0;
    auto sort = [&](void *tmp) {
      return smp_ok(hipcub::DeviceRadixSort::SortPairs(tmp, need, w.keys0.as<unsigned>(), w.keys1.as<unsigned>(), w.idx0.as<int>(), w.idx1.as<int>(),
                                                       (int)npool, 0, bits, 0), "sort");
    };
    if ((rc = sort(nullptr)) || (rc = smp_mem(w.sorttmp.reserve(need))) || (rc = sort(w.sorttmp.p))) return rc;
  }
  hipLaunchKernelGGL(smp_cand_kernel, dim3((unsigned)((ncand + 255) / 256)), dim3(256), 0, 0, (int)nhalf, w.calls->as<SmpBox>(), dim,
                     (unsigned long long)c.sp->seed, (unsigned long long)pass, ninc, w.halves.as<SmpBox>(), w.cand.as<double>());
  if ((rc = smp_eval(c.src, ncand, w.cand.as<double>()))) return rc;
  hipLaunchKernelGGL(smp_stats_kernel, dim3((unsigned)nhalf), dim3(WAVE), 0, 0, (int)nhalf, npool, w.keys1.as<unsigned>(), w.idx1.as<int>(),
                     c.pool.as<double>(), w.cand.as<double>(), w.halves.as<SmpBox>(), dim, c.nspec, ninc, tol, w.nadd.as<int>(), w.refine.as<int>(),
                     w.addA.as<int>());
  size_t need = 0;
  auto scan = [&](void *tmp, DevBytes &in, DevBytes &out) {
    return smp_ok(hipcub::DeviceScan::ExclusiveSum(tmp, need, in.as<int>(), out.as<int>(), (int)nhalf, 0), "scan");
  };
  if ((rc = scan(nullptr, w.nadd, w.addoff)) || (rc = smp_mem(w.scantmp.reserve(need))) || (rc = scan(w.scantmp.p, w.nadd, w.addoff)) ||
      (rc = scan(w.scantmp.p, w.refine, w.childoff)))
    return rc;
  int last[4]; // the last offset and the last count of each scan: their sums are the totals
  DevBytes *const ends[4] = {&w.addoff, &w.nadd, &w.childoff, &w.refine};
  for (int q = 0; q < 4; ++q)
    if ((rc = smp_ok(hipMemcpy(&last[q], ends[q]->as<int>() + nhalf - 1, 4, hipMemcpyDeviceToHost), "totals"))) return rc;
  const long long total_add = (long long)last[0] + last[1], nchild = (long long)last[2] + last[3];
  const int make_children = depth + 1 <= c.sp->max_recursion ? 1 : 0; // a call beyond maxdepth returns at once (:65-68)
  if (npool + total_add >= (1ll << 31) - (1ll << 26)) return srt_set_error(SRT_EINVAL, "sample pool too large");
  if ((rc = smp_mem(c.pool.reserve((size_t)(npool + total_add) * SMP_RB, (size_t)npool * SMP_RB) ||
                    c.slot.reserve((size_t)(npool + total_add) * sizeof(int), (size_t)npool * sizeof(int)) ||
                    w.children->reserve((size_t)(nchild > 0 ? nchild : 1) * sizeof(SmpBox)))))
    return rc;
  if (npool > 0)
    hipLaunchKernelGGL(smp_reslot_kernel, dim3((unsigned)((npool + 255) / 256)), dim3(256), 0, 0, npool, w.keys0.as<unsigned>(),
                       (unsigned)nhalf, w.refine.as<int>(), w.childoff.as<int>(), make_children, c.slot.as<int>());
  hipLaunchKernelGGL(smp_commit_kernel, dim3((unsigned)((nhalf + 255) / 256)), dim3(256), 0, 0, (int)nhalf, ninc, w.addA.as<int>(),
                     w.refine.as<int>(), w.addoff.as<int>(), w.childoff.as<int>(), make_children, w.cand.as<double>(), w.halves.as<SmpBox>(),
                     npool, c.pool.as<double>(), c.slot.as<int>(), w.children->as<SmpBox>());
  if ((rc = smp_ok(hipDeviceSynchronize(), "level"))) return rc;
  c.npool += total_add, c.counts[3] += total_add;
  std::swap(w.calls, w.children);
  ncalls = make_children ? nchild : 0;
  return SRT_OK;
}
// (3) adaptive (:298-347): tol halves until adaptive_nmax adaptive samples exist; every pass starts again from the root box
static int smp_adaptive(SmpCall &c, int max_passes) {
  SmpScratch w;
  double tol = c.sp->initial_tol;
  for (int pass = 0; c.counts[3] < c.sp->adaptive_nmax && pass < max_passes; ++pass, tol = tol / 2.0) {
    if (c.npool >= (1ll << 31) - (1ll << 26)) return srt_set_error(SRT_EINVAL, "sample pool too large");
    int rc = smp_mem(c.slot.reserve((size_t)c.npool * sizeof(int)));
    if (rc) return rc;
    if (c.npool > 0) hipLaunchKernelGGL(smp_fill_int, dim3((unsigned)((c.npool + 255) / 256)), dim3(256), 0, 0, c.npool, c.slot.as<int>(), 0);
    if ((rc = smp_mem(w.calls->reserve(sizeof(SmpBox)))) ||
        (rc = smp_ok(hipMemcpy(w.calls->p, &c.root, sizeof(SmpBox), hipMemcpyHostToDevice), "root box")))
      return rc;
    long long ncalls = 1;
    for (int depth = 0; depth <= c.sp->max_recursion && ncalls > 0; ++depth)
      if ((rc = smp_level(c, w, pass, depth, tol, ncalls))) return rc;
  }
  return SRT_OK;
}
// the pool comes down and the tail goes behind it: a malloc'd array of 3 + nspec doubles a sample
static int smp_download(SmpCall &c, int64_t *n_out, double **out) {
  const size_t w = 3 + (size_t)c.nspec, ntail = c.tail.size() / w;
  double *res = (double *)malloc(((size_t)c.npool + ntail + 1) * w * sizeof(double));
  if (!res) return srt_set_error(SRT_ENOMEM, "malloc failed");
  if (c.npool > 0) {
    std::vector<double> h((size_t)c.npool * SMP_REC);
    hipError_t e = hipMemcpy(h.data(), c.pool.p, h.size() * sizeof(double), hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
      free(res);
      return srt_set_error(SRT_EDEVICE, "sample download: %s", hipGetErrorString(e));
    }
    for (long long i = 0; i < c.npool; ++i)
      for (size_t q = 0; q < w; ++q) res[(size_t)i * w + q] = h[(size_t)i * SMP_REC + q];
  }
  if (ntail) memcpy(res + (size_t)c.npool * w, c.tail.data(), c.tail.size() * sizeof(double));
  *out = res;
  *n_out = c.npool + (int64_t)ntail;
  return SRT_OK;
}

extern "C" int srt_build_samples(srt_model *src, const srt_sampler_params *sp, int64_t n_in, const double *in_pts,
                                 int64_t *n_out, double **out, int64_t stage_counts[6]) {
  if (!src || !sp || !n_out || !out || n_in < 0 || (n_in > 0 && !in_pts)) return srt_set_error(SRT_EINVAL, "bad argument");
  if (const int bad = with_model(src, [](auto) -> int { return SRT_OK; })) return bad; // an unknown kind fails before anything is allocated
  const double *bd = sp->bounds;
  if (!(bd[1] > bd[0]) || !(bd[3] > bd[2]) || !(bd[5] > bd[4])) return srt_set_error(SRT_EINVAL, "empty bounds");
  if (sp->n_zero_altitude < 0 || sp->n_iri_pad < 0 || sp->n_initial_radial < 0 || sp->n_initial_uniform < 0 || sp->max_recursion < 0 || sp->numincrease < 0)
    return srt_set_error(SRT_EINVAL, "negative count");
  SRT_MODEL_SCOPE;
  int rc = ensure_model(src);
  if (rc) return rc;
  const int ninc = sp->numincrease ? sp->numincrease : 5;
  if (ninc > WAVE) return srt_set_error(SRT_EINVAL, "numincrease > %d", WAVE);
  SmpCall c{src, sp, src->nspec, ninc, SmpBox{{bd[0], bd[2], bd[4]}, {bd[1], bd[3], bd[5]}, 1}, {n_in, 0, 0, 0, 0, 0}};
  double r2 = 0.0; // the farthest corner of the box
  for (int q = 0; q < 8; ++q) {
    const double x = bd[q & 4 ? 1 : 0], y = bd[q & 2 ? 3 : 2], z = bd[q & 1 ? 5 : 4];
    const double v = x * x + y * y + z * z;
    if (v > r2) r2 = v;
  }
  // (0) points of an existing file: part of the initial set and of the output (:210-227)
  if (n_in > 0) {
    std::vector<double> h((size_t)n_in * SMP_REC, 0.0);
    for (int64_t i = 0; i < n_in; ++i)
      for (int q = 0; q < 3 + c.nspec; ++q) h[(size_t)i * SMP_REC + q] = in_pts[(size_t)i * (3 + c.nspec) + q];
    if ((rc = smp_mem(c.pool.reserve(h.size() * sizeof(double)))) ||
        (rc = smp_ok(hipMemcpy(c.pool.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice), "input points")))
      return rc;
    c.npool = n_in;
  }
  // (1) radial (:228-272), (2) uniform (:275-296), (3) adaptive, (4) zero altitude (:349-377), (5) ionosphere shell (:379-405)
  if ((rc = smp_stage(c, SMP_RADIAL, sp->n_initial_radial, R_E, sqrt(r2), true, c.counts[1])) ||
      (rc = smp_stage(c, SMP_UNIFORM, sp->n_initial_uniform, 0.0, 0.0, true, c.counts[2])) ||
      (sp->adaptive_nmax > 0 && (rc = smp_adaptive(c, sp->max_passes > 0 ? sp->max_passes : 64))) ||
      (rc = smp_stage(c, SMP_ZEROALT, sp->n_zero_altitude, R_E, R_E, false, c.counts[4])) ||
      (rc = smp_stage(c, SMP_IRI, sp->n_iri_pad, R_E, R_E + 2000000.0, false, c.counts[5])) || (rc = smp_download(c, n_out, out)))
    return rc;
  for (int q = 0; stage_counts && q < 6; ++q) stage_counts[q] = c.counts[q];
  return SRT_OK;
}
