// Host build of srt_host::igrf_setup (stanford_raytracer_amd/csrc/srt_host.cpp, the very source the library compiles) for
// the CPU tests of tests/test_igrf_edges.py: no GPU, no HIP runtime.
#include "../../stanford_raytracer_amd/csrc/srt_host.cpp"

// what srt_host.cpp's file-format entry points take from srt_api_core.hpp and srt_api_trace.hpp (not called here: only igrf_setup is)
int srt_set_error(int code, const char *, ...) { return code; }
extern "C" int srt_rows_per_ray(const srt_params *) { return 0; }

// 1 and G, H, REC (geopack's index), A, psi filled; or 0 and the error text in err[errlen]
extern "C" int igh_setup(const char *coeff_file, int yearday, int msec, float *G, float *H, float *REC, float *A, float *psi,
                         char *err, int errlen) {
  std::string e;
  const bool ok = srt_host::igrf_setup(coeff_file, yearday, msec, G, H, REC, A, psi, e);
  if (err && errlen > 0) snprintf(err, (size_t)errlen, "%s", e.c_str());
  return ok ? 1 : 0;
}
