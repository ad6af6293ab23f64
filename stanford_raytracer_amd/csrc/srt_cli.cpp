// srt_cli.cpp -- `raytracer`: command-line front end with the reference's flag grammar, ray-input format and
// .ray output format (fortran/raytracer_driver.f95), driving the batched HIP path through the C ABI.
//
// Grammar (fortran/util.f95:53-84 getopt_named): every argument is --name=value; the FIRST argument whose
// text between column 3 and the first '=' equals the name wins; unknown flags are ignored.  Numeric integer
// flags are read as reals and floored (driver:195-196).  Where the reference leaves an unset flag
// uninitialised we fail with a message instead (documented divergence).
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <array>
#include <future>
#include <map>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../include/srt.h"

static int g_argc;
static char **g_argv;

static bool getopt_named(const char *name, std::string &out) {
  for (int i = 1; i < g_argc; ++i) {
    const char *a = g_argv[i];
    const char *eq = strchr(a, '=');
    if (!eq || eq - a < 2) continue;
    std::string key(a + 2, eq - (a + 2));
    if (key == name) {
      out = eq + 1;
      return true;
    }
  }
  return false;
}
static bool get_real(const char *name, double &v) {
  std::string s;
  if (!getopt_named(name, s)) return false;
  for (auto &ch : s)
    if (ch == 'd' || ch == 'D') ch = 'e';
  v = strtod(s.c_str(), nullptr);
  return true;
}
static bool get_int(const char *name, int &v) {
  double d;
  if (!get_real(name, d)) return false;
  v = (int)floor(d);
  return true;
}
static void need(bool ok, const char *name) {
  if (!ok) {
    fprintf(stderr, "raytracer: required flag --%s=... is missing\n", name);
    exit(2);
  }
}
#define CHECK(call)                                                      \
  do {                                                                   \
    int rc_ = (call);                                                    \
    if (rc_ != 0) {                                                      \
      fprintf(stderr, "raytracer: %s failed: %s\n", #call, srt_last_error()); \
      return 1;                                                          \
    }                                                                    \
  } while (0)

static double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// model flags of the driver (raytracer_driver.f95:256-770) -> model handle; del = the driver's FD step for the model
static int make_model(int device, srt_model **out, double *del) {
  int modelnum = 0;
  std::string file;
  need(get_int("modelnum", modelnum), "modelnum");
  srt_params p; // only p.del is set here
  memset(&p, 0, sizeof p);
  int yearday = 0, msec = 0, use_tsy = 0, use_igrf = 0;
  need(get_int("yearday", yearday), "yearday");
  need(get_int("milliseconds_day", msec), "milliseconds_day");
  get_int("use_tsyganenko", use_tsy);
  get_int("use_igrf", use_igrf);
  CHECK(srt_init(device));
  srt_model *m = nullptr;
  // FD step for dF/dx: delSP for the single-precision models, delDP otherwise (driver:251-252, :1158-1176)
  if (modelnum == 1) {
    need(getopt_named("ngo_configfile", file), "ngo_configfile");
    p.del = 1.0e-4;
    CHECK(srt_model_create_ngo(file.c_str(), yearday, msec, &m));
  } else if (modelnum == 3) {
    need(getopt_named("interp_interpfile", file), "interp_interpfile");
    p.del = 1.0e-6;
    // ours: --interp_layout=expanded|nodes|auto, the device layout of the table (include/srt.h); default expanded
    int layout = SRT_INTERP_EXPANDED;
    std::string lay;
    if (getopt_named("interp_layout", lay)) {
      if (lay == "expanded") layout = SRT_INTERP_EXPANDED;
      else if (lay == "nodes") layout = SRT_INTERP_NODES;
      else if (lay == "auto") layout = SRT_INTERP_AUTO;
      else {
        fprintf(stderr, "raytracer: --interp_layout=%s is not a layout (expanded, nodes or auto)\n", lay.c_str());
        exit(2);
      }
    }
    printf(" Reading input file\n");
    CHECK(srt_model_create_interp_file_layout(file.c_str(), yearday, msec, layout, &m));
    printf(" Done\n");
  } else if (modelnum == 4) {
    need(getopt_named("interp_interpfile", file), "interp_interpfile");
    double ws = 0, lws = 0;
    int order = 0, exact = 0;
    need(get_real("scattered_interp_window_scale", ws), "scattered_interp_window_scale");
    need(get_int("scattered_interp_order", order), "scattered_interp_order");
    need(get_int("scattered_interp_exact", exact), "scattered_interp_exact");
    need(get_real("scattered_interp_local_window_scale", lws), "scattered_interp_local_window_scale");
    p.del = 1.0e-6;
    // ours (opt-in): --scattered_interp_root_sample=<record number, 1 = the file's first sample>: the sample at the root of the
    // reference's kd-tree keeps a stored spacing of 0 there (kdtree_mod.f95:386-444); default: none
    double root = 0;
    get_real("scattered_interp_root_sample", root);
    CHECK(srt_model_create_scattered_file_root(file.c_str(), yearday, msec, ws, order, exact, lws, (int64_t)floor(root) - 1, &m));
  } else if (modelnum == 6) {
    // simple_3d_model_adapter (raytracer_driver.f95:893-992).  --ngo_configfile is accepted and ignored, as the driver reads
    // it and never uses it.  Required by name (the driver would run on whatever its state block holds): kp, and MLT when
    // fixed_MLT = 1.
    double kp = 0.0, mlt = 0.0;
    int fixed_mlt = 0;
    getopt_named("ngo_configfile", file);
    need(get_real("kp", kp), "kp");
    get_int("fixed_MLT", fixed_mlt);
    if (fixed_mlt == 1) need(get_real("MLT", mlt), "MLT");
    else get_real("MLT", mlt);
    p.del = 1.0e-6; // delDP (:1188)
    CHECK(srt_model_create_simple3d(kp, fixed_mlt, mlt, yearday, msec, &m));
  } else if (modelnum == 7) {
    // AT64ThCh_adapter (raytracer_driver.f95:1024-1136).  Required by name: gcpm_kp, an integer, and the ten T04_s parameters --
    // also with --use_tsyganenko=0, because the model's field-line trace runs through T04_s + IGRF whatever the field options are.
    double kpv = 0.0;
    need(get_real("gcpm_kp", kpv), "gcpm_kp");
    if (!(kpv == floor(kpv)) || fabs(kpv) > 1000.0) {
      fprintf(stderr, "raytracer: --gcpm_kp must be an integer (the AT64ThCh adapter's gcpm_kp is one)\n");
      exit(2);
    }
    const char *names[10] = {"tsyganenko_Pdyn", "tsyganenko_Dst", "tsyganenko_ByIMF", "tsyganenko_BzIMF", "tsyganenko_W1",
                             "tsyganenko_W2",   "tsyganenko_W3",  "tsyganenko_W4",    "tsyganenko_W5",    "tsyganenko_W6"};
    double parmod[10];
    for (int k = 0; k < 10; ++k) need(get_real(names[k], parmod[k]), names[k]);
    std::string coeffs;
    getopt_named("igrf_coeffs", coeffs);
    p.del = 1.0e-4; // delSP (:1189-1194)
    CHECK(srt_model_create_at64thch((int)kpv, parmod, coeffs.empty() ? nullptr : coeffs.c_str(), yearday, msec, &m));
  } else {
    fprintf(stderr, "raytracer: --modelnum=%d is not on the accelerated path (1, 3, 4 and 6 are, and 7 = AT64ThCh; 5 = the 3-D Ngo "
                    "model is in the library, srt_model_create_ngo3d, and not yet reachable from this executable; 2 = GCPM is out "
                    "of scope)\n", modelnum);
    return 2;
  }
  if (use_igrf != 0 || use_tsy != 0) {
    std::string coeffs;
    getopt_named("igrf_coeffs", coeffs); // ours: table of Gauss coefficients (default: shipped beside the library)
    if (use_tsy != 0) { // raytracer_driver.f95:292-341
      const char *names[10] = {"tsyganenko_Pdyn", "tsyganenko_Dst", "tsyganenko_ByIMF", "tsyganenko_BzIMF", "tsyganenko_W1",
                               "tsyganenko_W2",   "tsyganenko_W3",  "tsyganenko_W4",    "tsyganenko_W5",    "tsyganenko_W6"};
      double parmod[10];
      for (int k = 0; k < 10; ++k) need(get_real(names[k], parmod[k]), names[k]);
      CHECK(srt_model_set_tsyganenko_params(m, parmod));
    }
    CHECK(srt_model_set_field(m, use_igrf != 0, use_tsy != 0, coeffs.empty() ? nullptr : coeffs.c_str()));
  }
  *out = m;
  *del = p.del;
  return 0;
}

// ---- readers the modes share ----
// --minx .. --maxz, all six required (gcpm_dens_model_buildgrid.f95:42-160, gcpm_dens_model_buildgrid_random.f95:56-90, dumpmodel.f95:167-213)
static void need_bounds(double b[6]) {
  const char *bn[6] = {"minx", "maxx", "miny", "maxy", "minz", "maxz"};
  for (int k = 0; k < 6; ++k) need(get_real(bn[k], b[k]), bn[k]);
}
// the bounds and --nx --ny --nz (read as reals and floored) of a regular grid.  An axis with fewer than `least` nodes, or more
// than an int holds, is refused with `refusal`, a format that takes the flag's name.  -> 0, or the exit code
static int need_grid(double b[6], int n3[3], double least, const char *refusal) {
  need_bounds(b);
  const char *nn[3] = {"nx", "ny", "nz"};
  for (int k = 0; k < 3; ++k) {
    double v = 0;
    need(get_real(nn[k], v), nn[k]);
    n3[k] = (int)floor(v);
    if (!(v >= least && v < 2147483648.0)) {
      fprintf(stderr, refusal, nn[k]);
      return 2;
    }
  }
  return 0;
}

// --damping_dist --damping_mode --damping_Ne_h --damping_kT_eV --damping_tol (ours)
static void read_damping_flags(srt_damping_params &dpar) {
  get_int("damping_dist", dpar.dist);
  get_int("damping_mode", dpar.mode);
  get_real("damping_Ne_h", dpar.Ne_h);
  double kTeV = 0;
  if (get_real("damping_kT_eV", kTeV)) dpar.kT = kTeV * 1.60217646e-19;
  get_real("damping_tol", dpar.tol);
}

// What srt_read_ray_file returns (n < 0: it failed, srt_last_error() says why) and the offsets of the packed layout, built from
// `kept`: rows[offsets[n]][SRT_ROW] is the row set the post-processors take.  Freed on the way out.
struct RayFile {
  int32_t nspec = 0;
  double qs[4], ms[4], *w0 = nullptr, *rows = nullptr;
  int64_t n = -1, nrec = 0, *raynum = nullptr;
  int32_t *stop = nullptr, *kept = nullptr;
  std::vector<int64_t> offsets;
  explicit RayFile(const std::string &path) {
    n = srt_read_ray_file(path.c_str(), &nspec, qs, ms, &nrec, &raynum, &stop, &kept, &w0, &rows);
    offsets.assign(n > 0 ? (size_t)n + 1 : 1, 0);
    for (int64_t i = 0; i < n; ++i) offsets[i + 1] = offsets[i] + kept[i];
  }
  RayFile(const RayFile &) = delete;
  RayFile &operator=(const RayFile &) = delete;
  ~RayFile() { srt_free(raynum), srt_free(stop), srt_free(kept), srt_free(w0), srt_free(rows); }
};

// A list-directed file of numbers, one record per line, `least` .. `most` (at most 5) numbers each: commas, tabs, CR and LF are
// blanks, a d or D exponent reads as e, empty lines are skipped, values a line leaves out are 0.
// -> 0; -1: the file cannot be opened; > 0: the number of the line that holds a bad token, too few numbers or one too many
static int read_number_lines(const std::string &path, int least, int most, std::vector<std::array<double, 5>> &out) {
  FILE *sf = fopen(path.c_str(), "r");
  if (!sf) return -1;
  char line[1024];
  int lineno = 0, bad_line = 0;
  while (!bad_line && fgets(line, sizeof line, sf)) {
    ++lineno;
    std::array<double, 5> v = {0, 0, 0, 0, 0};
    int nv = 0;
    for (char *q = line; *q; ++q)
      if (*q == ',' || *q == '\t' || *q == '\r' || *q == '\n') *q = ' ';
      else if (*q == 'd' || *q == 'D') *q = 'e';
    char *q = line;
    bool bad = false;
    for (;;) {
      while (*q == ' ') ++q;
      if (!*q) break;
      char *end = nullptr;
      const double x = strtod(q, &end);
      if (end == q || nv == most) {
        bad = true;
        break;
      }
      v[nv++] = x;
      q = end;
    }
    if (nv == 0 && !bad) continue; // an empty line
    if (bad || nv < least) bad_line = lineno;
    else out.push_back(v);
  }
  fclose(sf);
  return bad_line;
}

// ---- the modes: each reads its own flags and returns the exit code ----
// --grid2bin_in / --pts2bin_in: a model-3 grid or a model-4 sample file, text -> binary side-format (no GPU needed)
static int mode_convert() {
  std::string gin, gout, pin, pout;
  if (getopt_named("grid2bin_in", gin)) {
    need(getopt_named("grid2bin_out", gout), "grid2bin_out");
    CHECK(srt_grid_file_convert(gin.c_str(), gout.c_str()));
    return 0;
  }
  need(getopt_named("pts2bin_in", pin), "pts2bin_in");
  need(getopt_named("pts2bin_out", pout), "pts2bin_out");
  CHECK(srt_points_file_convert(pin.c_str(), pout.c_str()));
  return 0;
}

// the reference's gcpm_dens_model_buildgrid with the model of --modelnum in place of GCPM: same flags
// (gcpm_dens_model_buildgrid.f95:42-160: --minx .. --maxz, --nx --ny --nz (reals, floored), --compder, --filename) and
// the builder's exact text layout (:302-327, srt_grid_file_write); ours: --binary=1 (SRTGRID1), --device
static int mode_buildgrid() {
  std::string out;
  need(getopt_named("filename", out), "filename");
  double b[6], v = 0;
  int n3[3] = {0, 0, 0}, compder = 0, device = 0, binary = 0;
  if (int rc = need_grid(b, n3, 2.0, "raytracer: --%s must be >= 2 (the interpolated model needs two nodes per axis)\n")) return rc;
  if (get_real("compder", v)) compder = (int)floor(v);
  get_int("device", device);
  get_int("binary", binary);
  srt_model *m = nullptr;
  double del = 0.0;
  int rc = make_model(device, &m, &del);
  if (rc) return rc;
  const int nspec = srt_model_nspec(m);
  const size_t nval = (size_t)n3[0] * n3[1] * n3[2] * nspec;
  std::vector<double> F(nval), D(compder ? 7 * nval : 0);
  CHECK(srt_build_grid(m, compder ? 1 : 0, n3[0], n3[1], n3[2], b, F.data(), compder ? D.data() : nullptr));
  double qs[SRT_MAXSPEC], ms[SRT_MAXSPEC];
  srt_model_species(m, qs, ms);
  CHECK(srt_grid_file_write(out.c_str(), binary, nspec, n3[0], n3[1], n3[2], b, qs, ms, F.data(), compder ? D.data() : nullptr));
  printf(" %d x %d x %d nodes, %d species%s\n", n3[0], n3[1], n3[2], nspec, compder ? ", 7 derivative blocks" : "");
  srt_model_destroy(m);
  return 0;
}

// the reference's gcpm_dens_model_buildgrid_random with the model of --modelnum in place of GCPM: same flags
// (gcpm_dens_model_buildgrid_random.f95:56-90), --filename = output; ours: --seed, --binary=1
static int mode_buildsamples() {
  std::string out;
  need(getopt_named("filename", out), "filename");
  srt_sampler_params sp;
  memset(&sp, 0, sizeof sp);
  need_bounds(sp.bounds);
  double v = 0;
  if (get_real("n_zero_altitude", v)) sp.n_zero_altitude = (int64_t)floor(v);
  if (get_real("n_iri_pad", v)) sp.n_iri_pad = (int64_t)floor(v);
  if (get_real("n_initial_radial", v)) sp.n_initial_radial = (int64_t)floor(v);
  if (get_real("n_initial_uniform", v)) sp.n_initial_uniform = (int64_t)floor(v);
  sp.adaptive_nmax = 100000; // :92
  if (get_real("adaptive_nmax", v)) sp.adaptive_nmax = (int64_t)floor(v);
  get_real("initial_tol", sp.initial_tol);
  get_int("max_recursion", sp.max_recursion);
  if (get_real("seed", v)) sp.seed = (uint64_t)v;
  int device = 0, binary = 0;
  get_int("device", device);
  get_int("binary", binary);
  srt_model *m = nullptr;
  double del = 0.0;
  int rc = make_model(device, &m, &del);
  if (rc) return rc;
  int64_t n = 0, counts[6];
  double *rec = nullptr;
  CHECK(srt_build_samples(m, &sp, 0, nullptr, &n, &rec, counts));
  double qs[SRT_MAXSPEC], ms[SRT_MAXSPEC];
  srt_model_species(m, qs, ms);
  CHECK(srt_points_file_write(out.c_str(), binary, srt_model_nspec(m), n, sp.bounds, qs, ms, rec));
  printf(" %lld samples: %lld radial, %lld uniform, %lld adaptive, %lld zero-altitude, %lld ionosphere\n", (long long)n,
         (long long)counts[1], (long long)counts[2], (long long)counts[3], (long long)counts[4], (long long)counts[5]);
  srt_free(rec);
  srt_model_destroy(m);
  return 0;
}

// the reference's dumpmodel (fortran/dumpmodel.f95): funcPlasmaParams of the model of --modelnum at every node of a regular
// grid, any axis of which may have one node.  Same flags (:167-213: --minx .. --maxz, --nx --ny --nz read as reals and
// floored, --filename; the model's flags as make_model reads them) and the same text (:1284-1292, srt_dump_file_write).
// --mag_coords (:1086-1091, :1238-1242) is read for modelnum 6 and 7 only, as there; absent = 0, the value the reference's
// toolchain leaves in the unset variable.  Ours: --device, --timing=1.
static int mode_dumpmodel() {
  std::string out;
  need(getopt_named("filename", out), "filename");
  double b[6];
  int n3[3] = {0, 0, 0}, device = 0, timing = 0, modelnum = 0, mag = 0;
  if (int rc = need_grid(b, n3, 1.0, "raytracer: --%s must be >= 1 (one node = a slice: that axis sits at its minimum)\n")) return rc;
  if ((double)n3[0] * n3[1] * n3[2] > 2147483647.0) {
    fprintf(stderr, "raytracer: --nx x --ny x --nz is more than 2^31 - 1 nodes\n");
    return 2;
  }
  get_int("device", device);
  get_int("timing", timing);
  get_int("modelnum", modelnum);
  if (get_int("mag_coords", mag) && modelnum != 6 && modelnum != 7) {
    fprintf(stderr, "raytracer: --mag_coords is read for --modelnum=6 and 7 only (as by the reference's dumpmodel); ignored for "
                    "--modelnum=%d: the grid is in SM coordinates\n", modelnum);
    mag = 0;
  }
  const double t0 = now_s();
  srt_model *m = nullptr;
  double del = 0.0;
  int rc = make_model(device, &m, &del);
  if (rc) return rc;
  const double t1 = now_s();
  const int nspec = srt_model_nspec(m);
  std::vector<double> f((size_t)n3[0] * n3[1] * n3[2] * (4 * (size_t)nspec + 3));
  CHECK(srt_dump_model(m, n3[0], n3[1], n3[2], b, mag, f.data()));
  float kernel_ms = 0.f;
  srt_last_kernel_ms(m, &kernel_ms);
  const double t2 = now_s();
  CHECK(srt_dump_file_write(out.c_str(), nspec, n3[0], n3[1], n3[2], b, f.data()));
  const double t3 = now_s();
  printf(" %d x %d x %d nodes, %d species, %s coordinates\n", n3[0], n3[1], n3[2], nspec, mag ? "MAG" : "SM");
  if (timing)
    printf(" timing: {\"model_s\": %.3f, \"dump_s\": %.3f, \"kernel_ms\": %.3f, \"write_s\": %.3f, \"wall_s\": %.3f}\n", t1 - t0, t2 - t1,
           (double)kernel_ms, t3 - t2, t3 - t0);
  srt_model_destroy(m);
  return 0;
}

// ours: --damping_in=<existing .ray file> --damping_out=<file>: the MATLAB post-processor (matlab/damping/test_dampray.m)
// on a file this program or the reference's driver wrote, without tracing anything
static int mode_damping_in() {
  std::string din, dout;
  need(getopt_named("damping_in", din), "damping_in");
  need(getopt_named("damping_out", dout), "damping_out");
  srt_damping_params dpar;
  memset(&dpar, 0, sizeof dpar);
  read_damping_flags(dpar);
  int device = 0;
  get_int("device", device);
  RayFile ray(din);
  const int64_t n = ray.n;
  if (n < 0) {
    fprintf(stderr, "raytracer: %s\n", srt_last_error());
    return 1;
  }
  FILE *f = fopen(dout.c_str(), "w");
  if (!f) {
    fprintf(stderr, "raytracer: cannot open %s\n", dout.c_str());
    return 1;
  }
  if (n > 0) {
    CHECK(srt_init(device));
    int slots = 1;
    for (int64_t i = 0; i < n; ++i) slots = ray.kept[i] > slots ? ray.kept[i] : slots;
    // the file's records are every row it kept: outputper = 1 with nrows = records of the ray
    std::vector<double> rows((size_t)n * slots * SRT_ROW, 0.0), rate((size_t)n * slots), mag((size_t)n * slots);
    std::vector<int32_t> flag((size_t)n * slots);
    for (int64_t i = 0; i < n; ++i)
      memcpy(rows.data() + (size_t)i * slots * SRT_ROW, ray.rows + (size_t)ray.offsets[i] * SRT_ROW, sizeof(double) * SRT_ROW * (size_t)ray.kept[i]);
    CHECK(srt_damping(&dpar, ray.nspec, ray.qs, ray.ms, slots, 1, n, rows.data(), ray.kept, ray.w0, rate.data(), mag.data(), flag.data()));
    for (int64_t i = 0; i < n; ++i)
      for (int r = 0; r < ray.kept[i]; ++r) {
        const size_t idx = (size_t)i * slots + r;
        fprintf(f, "%10lld%10d%25.15E%25.15E%25.15E%10d\n", (long long)ray.raynum[i], r + 1, rows[idx * SRT_ROW], rate[idx], mag[idx], (int)flag[idx]);
      }
  }
  fclose(f);
  printf(" %lld rays, %lld records\n", (long long)n, (long long)ray.nrec);
  return 0;
}

// ours: --approach_in=<existing .ray file> --approach_observers=<file> --approach_out=<file>: each ray's closest approach to
// the observer points of the second file (include/srt.h), without tracing
static int mode_approach() {
  std::string ain, aobs, aout;
  need(getopt_named("approach_in", ain), "approach_in");
  need(getopt_named("approach_observers", aobs), "approach_observers");
  need(getopt_named("approach_out", aout), "approach_out");
  int device = 0;
  get_int("device", device);
  // one observer per line, list-directed as the surfaces file is: x y z radius
  std::vector<std::array<double, 5>> lines;
  const int bad = read_number_lines(aobs, 4, 4, lines);
  if (bad < 0) {
    fprintf(stderr, "raytracer: --approach_observers: cannot open %s\n", aobs.c_str());
    return 1;
  }
  if (bad > 0) {
    fprintf(stderr, "raytracer: --approach_observers: %s, line %d: expected `x y z radius` (four numbers)\n", aobs.c_str(), bad);
    return 1;
  }
  std::vector<srt_observer> obs;
  for (const auto &v : lines) obs.push_back(srt_observer{{v[0], v[1], v[2]}, v[3]});
  if (obs.empty() || obs.size() > (size_t)SRT_MAXOBS) {
    fprintf(stderr, "raytracer: --approach_observers: %s holds %zu observers (1 .. %d are taken)\n", aobs.c_str(), obs.size(), SRT_MAXOBS);
    return 1;
  }
  RayFile ray(ain);
  if (ray.n < 0) {
    fprintf(stderr, "raytracer: --approach_in: %s\n", srt_last_error());
    return 1;
  }
  int64_t nev = 0;
  double *ev = nullptr, *dist = nullptr;
  int32_t *meta = nullptr;
  if (ray.nrec >= 2) { // (fewer than two records hold no interval: nothing to ask a device for)
    CHECK(srt_init(device));
    CHECK(srt_approaches((int)obs.size(), obs.data(), ray.n, ray.offsets.data(), ray.rows, &nev, &ev, &meta, &dist));
  } else {
    // the observers are still looked at: a bad one is refused whatever the file holds
    int64_t zero[1] = {0};
    const int rc = srt_approaches((int)obs.size(), obs.data(), 0, zero, nullptr, &nev, &ev, &meta, &dist);
    if (rc == SRT_EINVAL) {
      fprintf(stderr, "raytracer: %s\n", srt_last_error());
      return 1;
    }
    nev = 0;
  }
  std::vector<int64_t> evray((size_t)nev);
  for (int64_t e = 0; e < nev; ++e) evray[e] = ray.raynum[meta[4 * e]];
  CHECK(srt_approaches_file_write(aout.c_str(), nev, evray.data(), meta, dist, ev));
  printf(" %lld rays, %lld records, %zu observers, %lld approaches\n", (long long)ray.n, (long long)ray.nrec, obs.size(), (long long)nev);
  srt_free(ev), srt_free(meta), srt_free(dist);
  return 0;
}

// ours: --tube_in=<existing .ray file> --tube_neighbours=<file> --tube_out=<file>: the sections of the ray tubes of the second
// file (include/srt.h, "ray tubes") at every record of their centre rays, without tracing.  Whatever is wrong with the three
// flags or the two input files is refused by name with exit code 2.
static int mode_tube() {
  std::string tin, tnb, tout;
  need(getopt_named("tube_in", tin), "tube_in");
  need(getopt_named("tube_neighbours", tnb), "tube_neighbours");
  need(getopt_named("tube_out", tout), "tube_out");
  int device = 0;
  get_int("device", device);
  // one tube per line, list-directed: centre b c, the ray numbers of the .ray file
  std::vector<std::array<double, 5>> lines;
  const int bad = read_number_lines(tnb, 3, 3, lines);
  if (bad < 0) {
    fprintf(stderr, "raytracer: --tube_neighbours: cannot open %s\n", tnb.c_str());
    return 2;
  }
  if (bad > 0) {
    fprintf(stderr, "raytracer: --tube_neighbours: %s, line %d: expected `centre b c` (three ray numbers)\n", tnb.c_str(), bad);
    return 2;
  }
  RayFile ray(tin);
  if (ray.n < 0) {
    fprintf(stderr, "raytracer: --tube_in: %s\n", srt_last_error());
    return 2;
  }
  std::map<int64_t, int64_t> index; // ray number -> ray of the file
  for (int64_t i = 0; i < ray.n; ++i) index[ray.raynum[i]] = i;
  std::vector<int64_t> nb(ray.n > 0 ? (size_t)ray.n * 2 : 2, -1);
  for (size_t k = 0; k < lines.size(); ++k) {
    int64_t idx[3];
    for (int c = 0; c < 3; ++c) {
      const double v = lines[k][c];
      const auto it = v == std::floor(v) && std::fabs(v) < 1e15 ? index.find((int64_t)v) : index.end();
      if (it == index.end()) {
        fprintf(stderr, "raytracer: --tube_neighbours: %s, tube %zu: %s holds no ray number %.17g\n", tnb.c_str(), k + 1, tin.c_str(), v);
        return 2;
      }
      idx[c] = it->second;
    }
    if (nb[2 * idx[0]] != -1) {
      fprintf(stderr, "raytracer: --tube_neighbours: %s, tube %zu: centre %lld is listed twice\n", tnb.c_str(), k + 1, (long long)ray.raynum[idx[0]]);
      return 2;
    }
    if (idx[1] == idx[2] || idx[1] == idx[0] || idx[2] == idx[0]) {
      fprintf(stderr, "raytracer: --tube_neighbours: %s, tube %zu: a tube takes three different rays\n", tnb.c_str(), k + 1);
      return 2;
    }
    nb[2 * idx[0]] = idx[1], nb[2 * idx[0] + 1] = idx[2];
  }
  std::vector<double> section((size_t)ray.nrec * 4 + 4);
  std::vector<int32_t> flag((size_t)ray.nrec + 1);
  if (ray.nrec > 0) { // (no record: nothing to ask a device for)
    CHECK(srt_init(device));
    CHECK(srt_tubes(ray.n, nb.data(), ray.offsets.data(), ray.rows, section.data(), flag.data()));
  }
  CHECK(srt_tubes_file_write(tout.c_str(), ray.n > 0 ? ray.n : 0, ray.raynum, ray.offsets.data(), ray.rows, section.data(), flag.data()));
  long long ok = 0, with = 0;
  for (int64_t j = 0; j < ray.nrec; ++j) ok += flag[j] == 0, with += flag[j] != 1;
  printf(" %lld rays, %lld records, %zu tubes, %lld sections (%lld ok)\n", (long long)ray.n, (long long)ray.nrec, lines.size(), with, ok);
  return 0;
}

// ours: --crossings_in=<existing .ray file> --crossings_surfaces=<file> --crossings_out=<file>: where and when the rays of a
// file this program or the reference's driver wrote cross the surfaces of the second file (include/srt.h), without tracing
static int mode_crossings() {
  std::string cin_path, csurf, cout_path;
  need(getopt_named("crossings_in", cin_path), "crossings_in");
  need(getopt_named("crossings_surfaces", csurf), "crossings_surfaces");
  need(getopt_named("crossings_out", cout_path), "crossings_out");
  int device = 0;
  get_int("device", device);
  // one surface per line, list-directed: kind p0 p1 p2 p3; trailing values may be absent (0); a real kind is floored
  std::vector<std::array<double, 5>> lines;
  const int bad = read_number_lines(csurf, 1, 5, lines);
  if (bad < 0) {
    fprintf(stderr, "raytracer: --crossings_surfaces: cannot open %s\n", csurf.c_str());
    return 1;
  }
  if (bad > 0) {
    fprintf(stderr, "raytracer: --crossings_surfaces: %s, line %d: expected `kind p0 p1 p2 p3` (at most five numbers)\n", csurf.c_str(), bad);
    return 1;
  }
  std::vector<srt_surface> surf;
  for (const auto &v : lines) {
    srt_surface s;
    memset(&s, 0, sizeof s);
    s.kind = (int32_t)floor(v[0]);
    for (int k = 0; k < 4; ++k) s.p[k] = v[1 + k];
    surf.push_back(s);
  }
  if (surf.empty() || surf.size() > SRT_MAXSURF) {
    fprintf(stderr, "raytracer: --crossings_surfaces: %s holds %zu surfaces (1 .. %d are taken)\n", csurf.c_str(), surf.size(), SRT_MAXSURF);
    return 1;
  }
  RayFile ray(cin_path);
  if (ray.n < 0) {
    fprintf(stderr, "raytracer: --crossings_in: %s\n", srt_last_error());
    return 1;
  }
  int64_t nev = 0;
  double *ev = nullptr;
  int32_t *meta = nullptr;
  if (ray.nrec >= 2) { // (fewer than two records hold no interval: nothing to ask a device for)
    CHECK(srt_init(device));
    CHECK(srt_crossings((int)surf.size(), surf.data(), ray.n, ray.offsets.data(), ray.rows, &nev, &ev, &meta));
  } else {
    // the surfaces are still looked at: a bad one is refused whatever the file holds
    int64_t zero[1] = {0};
    const int rc = srt_crossings((int)surf.size(), surf.data(), 0, zero, nullptr, &nev, &ev, &meta);
    if (rc == SRT_EINVAL) {
      fprintf(stderr, "raytracer: %s\n", srt_last_error());
      return 1;
    }
    nev = 0;
  }
  std::vector<int64_t> evray((size_t)nev);
  for (int64_t e = 0; e < nev; ++e) evray[e] = ray.raynum[meta[4 * e]];
  CHECK(srt_crossings_file_write(cout_path.c_str(), nev, evray.data(), meta, ev));
  printf(" %lld rays, %lld records, %zu surfaces, %lld crossings\n", (long long)ray.n, (long long)ray.nrec, surf.size(), (long long)nev);
  srt_free(ev), srt_free(meta);
  return 0;
}

// ours: --bin_in=<existing .ray file> --bin_axes=<file> --bin_out=<file> [--bin_nsub=8] [--bin_quantum=2^-30]: the dwell-time
// map of the rays of a file this program or the reference's driver wrote on the grid of the second file (include/srt.h),
// without tracing.  What is wrong with the flags or the files is refused by name with exit code 2.
static int mode_bin() {
  std::string bin_path, baxes, bout_path;
  need(getopt_named("bin_in", bin_path), "bin_in");
  need(getopt_named("bin_axes", baxes), "bin_axes");
  need(getopt_named("bin_out", bout_path), "bin_out");
  int device = 0;
  get_int("device", device);
  srt_bin_params bp;
  memset(&bp, 0, sizeof bp);
  bp.nsub = 8;
  bp.quantum = 9.313225746154785e-10; // 2^-30 s
  get_int("bin_nsub", bp.nsub);
  get_real("bin_quantum", bp.quantum);
  // one axis per line: kind n e0 e1 .. en; the kind a number or a name; commas and d exponents are tolerated
  std::vector<std::vector<double>> edges;
  {
    FILE *af = fopen(baxes.c_str(), "r");
    if (!af) {
      fprintf(stderr, "raytracer: --bin_axes: cannot open %s\n", baxes.c_str());
      return 2;
    }
    static const char *names[8] = {"x", "y", "z", "r", "rho", "L", "sinlat", "mlt"};
    std::vector<char> line(1 << 16);
    int lineno = 0;
    while (fgets(line.data(), (int)line.size(), af)) {
      ++lineno;
      for (char *q = line.data(); *q; ++q)
        if (*q == ',' || *q == '\t' || *q == '\r' || *q == '\n') *q = ' ';
      char *q = line.data();
      while (*q == ' ') ++q;
      if (!*q) continue; // an empty line
      const char *what = nullptr;
      int kind = -1;
      char *end = q;
      while (*end && *end != ' ') ++end;
      const std::string word(q, end);
      for (int k = 0; k < 8; ++k)
        if (word == names[k]) kind = k;
      if (kind < 0) {
        char *e2 = nullptr;
        const double v = strtod(q, &e2);
        if (e2 != end || !(v >= -1e9 && v <= 1e9)) what = "the kind is neither a number nor one of x y z r rho L sinlat mlt";
        else kind = (int)floor(v);
      }
      std::vector<double> v;
      for (q = end; !what;) {
        while (*q == ' ') ++q;
        if (!*q) break;
        for (char *s = q; *s && *s != ' '; ++s)
          if (*s == 'd' || *s == 'D') *s = 'e';
        char *e2 = nullptr;
        const double x = strtod(q, &e2);
        if (e2 == q || (*e2 && *e2 != ' ')) what = "not a number";
        v.push_back(x);
        q = e2;
      }
      if (!what && (v.empty() || v[0] != floor(v[0]) || !(v[0] >= 1.0 && v[0] <= 1024.0))) what = "n is not a whole number of 1 .. 1024";
      if (!what && v.size() != (size_t)v[0] + 2) what = "the line does not hold n + 1 edges";
      if (!what && edges.size() == 3) what = "a fourth axis";
      if (what) {
        fclose(af);
        fprintf(stderr, "raytracer: --bin_axes: %s, line %d: %s (expected `kind n e0 e1 .. en`)\n", baxes.c_str(), lineno, what);
        return 2;
      }
      bp.axis[edges.size()].kind = kind;
      bp.axis[edges.size()].n = (int32_t)v[0];
      edges.emplace_back(v.begin() + 1, v.end());
    }
    fclose(af);
    if (edges.empty()) {
      fprintf(stderr, "raytracer: --bin_axes: %s holds no axis (1 .. 3 are taken)\n", baxes.c_str());
      return 2;
    }
    bp.naxes = (int32_t)edges.size();
    for (size_t a = 0; a < edges.size(); ++a) bp.axis[a].edges = edges[a].data();
  }
  int64_t ncells = 0;
  if (srt_bin_cells(&bp, &ncells) != SRT_OK) { // --bin_nsub, --bin_quantum and the edges, by name
    fprintf(stderr, "raytracer: --bin_axes / --bin_nsub / --bin_quantum: %s\n", srt_last_error());
    return 2;
  }
  RayFile ray(bin_path);
  if (ray.n < 0) {
    fprintf(stderr, "raytracer: --bin_in: %s\n", srt_last_error());
    return 2;
  }
  int64_t *ticks = nullptr, *hits = nullptr, counters[4] = {0, 0, 0, 0};
  std::vector<int64_t> zeros;
  if (ray.nrec >= 2) { // (fewer than two records hold no interval: nothing to ask a device for)
    CHECK(srt_init(device));
    CHECK(srt_bin_rays(&bp, ray.n, ray.offsets.data(), ray.rows, nullptr, nullptr, &ticks, &hits, counters));
  } else {
    zeros.assign((size_t)ncells, 0);
  }
  CHECK(srt_bin_file_write(bout_path.c_str(), &bp, ticks ? ticks : zeros.data(), hits ? hits : zeros.data()));
  printf(" %lld rays, %lld records, %lld cells: %lld intervals used, %lld skipped, %lld samples deposited, %lld outside\n",
         (long long)ray.n, (long long)ray.nrec, (long long)ncells, (long long)counters[0], (long long)counters[1], (long long)counters[2],
         (long long)counters[3]);
  srt_free(ticks), srt_free(hits);
  return 0;
}

// the trace itself: the reference driver's run (raytracer_driver.f95) on the batched path
static int mode_trace() {
  srt_params p;
  memset(&p, 0, sizeof p);
  int device = 0, chunk = 0;
  std::string rays_path, out_path;
  need(get_real("dt0", p.dt0), "dt0");
  need(get_real("tmax", p.tmax), "tmax");
  need(get_int("root", p.root), "root");
  need(get_int("fixedstep", p.fixedstep), "fixedstep");
  need(get_int("maxsteps", p.maxsteps), "maxsteps");
  need(get_real("minalt", p.minalt), "minalt");
  need(getopt_named("inputraysfile", rays_path), "inputraysfile");
  need(getopt_named("outputfile", out_path), "outputfile");
  if (p.fixedstep == 0) {
    need(get_real("dtmax", p.dtmax), "dtmax");
    need(get_real("maxerr", p.maxerr), "maxerr");
  } else {
    get_real("dtmax", p.dtmax);
    get_real("maxerr", p.maxerr);
  }
  p.outputper = 1;
  get_int("outputper", p.outputper);
  if (p.outputper < 1) p.outputper = 1; // the reference's mod(i-1, outputper) with outputper <= 0 is undefined; the library clamps too
  get_int("device", device);
  // The first adaptive attempt (SURVEY A-1).  Default 1 = the step pattern of the reference's own
  // toolchain (gfortran: MAX(k_term, NaN) = k_term, Makefile:3,10); 0 = a flang build's (NaN: accept, no growth).
  p.first_attempt_policy = 1;
  get_int("first_attempt_policy", p.first_attempt_policy);
  if (p.first_attempt_policy != 0 && p.first_attempt_policy != 1) {
    fprintf(stderr, "raytracer: --first_attempt_policy must be 0 or 1\n");
    return 2;
  }
  get_int("ray_order", p.ray_order);
  get_int("chunk_rays", chunk);
  // ours: --segment_rows=N, the trace in segments (include/srt.h); 0 = one launch per chunk with every slot up front
  int segment_rows = 0;
  get_int("segment_rows", segment_rows);
  if (segment_rows < 0) {
    fprintf(stderr, "raytracer: --segment_rows must be >= 0\n");
    return 2;
  }
  {
    std::string dummy;
    if (segment_rows > 0 && getopt_named("damping_out", dummy)) {
      fprintf(stderr, "raytracer: --damping_out together with --segment_rows is not supported: the damping's running magnitude needs "
                      "the padded row layout of an unsegmented trace (run without --segment_rows, or --damping_in on the .ray file)\n");
      return 2;
    }
  }
  // ours: --devices=0,1,.. = one host thread and one model replica per GPU, contiguous shards of the ray file
  // (ceil(n/ndev) rays each), records written in ray order.  Default: the one device of --device.
  std::vector<int> devices;
  {
    std::string dl;
    if (getopt_named("devices", dl)) {
      const char *c = dl.c_str();
      while (*c) {
        char *end = nullptr;
        long v = strtol(c, &end, 10);
        if (end == c) break;
        devices.push_back((int)v);
        c = (*end == ',') ? end + 1 : end;
        if (end && *end && *end != ',') break;
      }
    }
    if (devices.empty()) devices.push_back(device);
  }
  const int ndev = (int)devices.size();
  int timing = 0;
  get_int("timing", timing);
  const double t_start = now_s();
  double *pos0 = nullptr, *dir0 = nullptr, *w0 = nullptr;
  int64_t nrays = srt_read_rays_file(rays_path.c_str(), &pos0, &dir0, &w0);
  const double parse_s = now_s() - t_start;
  if (nrays < 0) {
    fprintf(stderr, "raytracer: %s\n", srt_last_error());
    return 1;
  }
  // ours: --damping_out=<file> [--damping_dist=0|1 --damping_mode=0|1 --damping_Ne_h --damping_kT_eV --damping_tol]
  std::string damp_path;
  srt_damping_params dpar;
  memset(&dpar, 0, sizeof dpar);
  if (getopt_named("damping_out", damp_path)) read_damping_flags(dpar);
  // the reference opens the output with status="replace" even when there are no rays
  {
    FILE *f = fopen(out_path.c_str(), "w");
    if (!f) {
      fprintf(stderr, "raytracer: cannot open %s\n", out_path.c_str());
      return 1;
    }
    fclose(f);
  }
  // one shard per device; shard k writes <out>.part<k> (or <out> itself when there is one device), concatenated below
  struct Shard {
    int device = 0;
    int64_t lo = 0, hi = 0, steps = 0;
    std::string out, damp;
    int rc = 0;
    double model_s = 0, trace_s = 0, write_s = 0; // --timing=1: wall clock of the phases (write_s runs beside the next trace)
    int64_t out_bytes = 0;
  };
  std::vector<Shard> shards(ndev);
  const int64_t per_dev = (nrays + ndev - 1) / ndev;
  for (int k = 0; k < ndev; ++k) {
    Shard &sh = shards[k];
    sh.device = devices[k];
    sh.lo = std::min<int64_t>((int64_t)k * per_dev, nrays);
    sh.hi = std::min<int64_t>(sh.lo + per_dev, nrays);
    sh.out = ndev == 1 ? out_path : out_path + ".part" + std::to_string(k);
    sh.damp = damp_path.empty() ? std::string() : (ndev == 1 ? damp_path : damp_path + ".part" + std::to_string(k));
  }
  auto run_shard = [&](Shard &sh) -> int {
    srt_model *m = nullptr;
    double del = 0.0;
    const double tm0 = now_s();
    int rc = make_model(sh.device, &m, &del);
    if (rc) return rc;
    sh.model_s = now_s() - tm0;
    srt_params q = p;
    q.del = del;
    const int slots = srt_rows_per_ray(&q);
    double qs[SRT_MAXSPEC], ms[SRT_MAXSPEC];
    srt_model_species(m, qs, ms);
    const int nspec = srt_model_nspec(m);
    // bound host/device memory: at most ~2 GiB of trajectory rows per launch
    int64_t per = (int64_t)slots * SRT_ROW * 8;
    int64_t maxchunk = chunk > 0 ? chunk : ((int64_t)2 << 30) / (per > 0 ? per : 1);
    if (maxchunk < 64) maxchunk = 64;
    if (ndev > 1) {
      FILE *f = fopen(sh.out.c_str(), "w");
      if (!f) {
        fprintf(stderr, "raytracer: cannot open %s\n", sh.out.c_str());
        return 1;
      }
      fclose(f);
    }
    // chunk k's records are formatted and written (all host cores, srt_write_ray_file) while chunk k+1 is on the GPU
    struct Chunk {
      std::vector<double> rows, rate, mag;
      std::vector<int32_t> nrows, stop, flag;
    };
    std::future<int> pending;
    auto finish = [&]() -> int {
      if (!pending.valid()) return 0;
      const int rc = pending.get();
      if (rc) fprintf(stderr, "raytracer: writing %s failed\n", sh.out.c_str());
      return rc;
    };
    if (segment_rows > 0) {
      // The trace in segments: a chunk's rays go through the iterator, its rows are gathered ray-major on the host and written
      // from the packed layout -- the records of the unsegmented run.  N is at most what a ray can keep.
      const int32_t N = segment_rows < slots ? segment_rows : slots;
      const int32_t nseg = srt_trace_segments(&q, N);
      int64_t segchunk = chunk > 0 ? chunk : 262144;
      if (chunk <= 0) segchunk = std::min<int64_t>(segchunk, ((int64_t)2 << 30) / ((int64_t)N * SRT_ROW * 8));
      if (segchunk < 64) segchunk = 64;
      struct Packed {
        std::vector<int64_t> offsets;
        std::vector<double> rows;
        std::vector<int32_t> stop;
      };
      struct Piece { // one segment's delivery, kept until the chunk is assembled
        std::vector<int32_t> ray;
        std::vector<int64_t> offsets;
        std::vector<double> rows;
      };
      for (int64_t lo = sh.lo; lo < sh.hi; lo += segchunk) {
        const int64_t n = std::min<int64_t>(sh.hi - lo, segchunk);
        auto c = std::make_shared<Packed>();
        c->offsets.assign((size_t)n + 1, 0);
        c->stop.assign((size_t)n, 0);
        std::vector<Piece> pieces;
        const double tt0 = now_s();
        srt_trace_run *run = nullptr;
        CHECK(srt_trace_run_open(m, &q, n, pos0 + 3 * lo, dir0 + 3 * lo, w0 + lo, N, &run));
        for (int32_t s = 0; s < nseg; ++s) { // (bounded by the segment count, never by "until nothing is left" alone)
          srt_segment sg;
          const int got = srt_trace_run_next(run, &sg);
          if (got < 0) {
            fprintf(stderr, "raytracer: srt_trace_run_next failed: %s\n", srt_last_error());
            srt_trace_run_close(run);
            return 1;
          }
          if (got == 0) break;
          Piece pc;
          pc.ray.assign(sg.ray, sg.ray + sg.nrays);
          pc.offsets.assign(sg.offsets, sg.offsets + sg.nrays + 1);
          pc.rows.assign(sg.rows, sg.rows + (size_t)sg.offsets[sg.nrays] * SRT_ROW);
          for (int64_t i = 0; i < sg.nrays; ++i) {
            c->offsets[(size_t)sg.ray[i] + 1] += sg.offsets[i + 1] - sg.offsets[i]; // (counts first, prefix sums below)
            c->stop[(size_t)sg.ray[i]] = sg.stopcond[i];
          }
          sh.steps += sg.accepted_steps;
          pieces.push_back(std::move(pc));
        }
        srt_trace_run_close(run);
        for (int64_t i = 0; i < n; ++i) c->offsets[(size_t)i + 1] += c->offsets[(size_t)i];
        c->rows.resize((size_t)c->offsets[(size_t)n] * SRT_ROW);
        std::vector<int64_t> fill(c->offsets.begin(), c->offsets.end() - 1); // where a ray's next rows go
        for (const Piece &pc : pieces)
          for (size_t i = 0; i < pc.ray.size(); ++i) {
            const int64_t cnt = pc.offsets[i + 1] - pc.offsets[i];
            if (cnt > 0) memcpy(c->rows.data() + (size_t)fill[(size_t)pc.ray[i]] * SRT_ROW, pc.rows.data() + (size_t)pc.offsets[i] * SRT_ROW, (size_t)cnt * SRT_ROW * sizeof(double));
            fill[(size_t)pc.ray[i]] += cnt;
          }
        pieces.clear();
        sh.trace_s += now_s() - tt0;
        if (int rc = finish()) return rc;
        pending = std::async(std::launch::async, [=, &sh]() -> int {
          const double tw0 = now_s();
          if (srt_write_ray_file_packed(sh.out.c_str(), 1, lo + 1, n, nspec, qs, ms, w0 + lo, c->offsets.data(), c->rows.data(), c->stop.data())) return 1;
          sh.write_s += now_s() - tw0;
          return 0;
        });
      }
      if (int rc = finish()) return rc;
      srt_model_destroy(m);
      return 0;
    }
    for (int64_t lo = sh.lo; lo < sh.hi; lo += maxchunk) {
      int64_t n = sh.hi - lo < maxchunk ? sh.hi - lo : maxchunk;
      auto c = std::make_shared<Chunk>();
      c->rows.resize((size_t)n * slots * SRT_ROW);
      c->nrows.resize(n);
      c->stop.resize(n);
      int64_t steps = 0;
      const double tt0 = now_s();
      CHECK(srt_trace_batch(m, &q, n, pos0 + 3 * lo, dir0 + 3 * lo, w0 + lo, c->rows.data(), c->nrows.data(), c->stop.data(), &steps));
      sh.trace_s += now_s() - tt0;
      sh.steps += steps;
      const bool damp = !sh.damp.empty();
      if (damp) {
        // the MATLAB post-processor (matlab/damping/test_dampray.m) on the rows just traced: one record per kept row
        c->rate.resize((size_t)n * slots);
        c->mag.resize((size_t)n * slots);
        c->flag.resize((size_t)n * slots);
        CHECK(srt_damping(&dpar, nspec, qs, ms, slots, q.outputper, n, c->rows.data(), c->nrows.data(), w0 + lo, c->rate.data(), c->mag.data(), c->flag.data()));
      }
      if (int rc = finish()) return rc;
      const bool first = lo == sh.lo;
      pending = std::async(std::launch::async, [=, &sh, &q]() -> int {
        const double tw0 = now_s();
        if (srt_write_ray_file(sh.out.c_str(), 1, lo + 1, n, &q, nspec, qs, ms, w0 + lo, c->rows.data(), c->nrows.data(), c->stop.data())) return 1;
        sh.write_s += now_s() - tw0;
        if (damp) {
          FILE *f = fopen(sh.damp.c_str(), first ? "w" : "a");
          if (!f) return 1;
          for (int64_t i = 0; i < n; ++i) {
            const int kept = c->nrows[i] > 0 ? (c->nrows[i] - 1) / q.outputper + 1 : 0;
            for (int r = 0; r < kept && r < slots; ++r) {
              const size_t idx = (size_t)i * slots + r;
              fprintf(f, "%10lld%10d%25.15E%25.15E%25.15E%10d\n", (long long)(lo + i + 1), r * q.outputper + 1, c->rows[idx * SRT_ROW], c->rate[idx],
                      c->mag[idx], (int)c->flag[idx]);
            }
          }
          if (fclose(f) != 0) return 1;
        }
        return 0;
      });
    }
    if (int rc = finish()) return rc;
    srt_model_destroy(m);
    return 0;
  };
  if (ndev == 1) {
    shards[0].rc = run_shard(shards[0]);
  } else {
    std::vector<std::thread> th;
    for (int k = 0; k < ndev; ++k) th.emplace_back([&, k] { shards[k].rc = run_shard(shards[k]); });
    for (auto &t : th) t.join();
  }
  int64_t total_steps = 0;
  for (auto &sh : shards) {
    if (sh.rc) return sh.rc;
    total_steps += sh.steps;
  }
  if (ndev > 1) { // records in ray order: shard 0's file, then shard 1's, ...
    auto cat = [](const std::string &dst, const std::vector<std::string> &parts) -> bool {
      FILE *o = fopen(dst.c_str(), "w");
      if (!o) return false;
      std::vector<char> buf(1 << 22);
      for (auto &pn : parts) {
        FILE *i = fopen(pn.c_str(), "r");
        if (!i) continue; // an empty shard (fewer rays than devices) wrote nothing
        size_t got;
        while ((got = fread(buf.data(), 1, buf.size(), i)) > 0) fwrite(buf.data(), 1, got, o);
        fclose(i);
        remove(pn.c_str());
      }
      return fclose(o) == 0;
    };
    std::vector<std::string> parts, dparts;
    for (auto &sh : shards) {
      parts.push_back(sh.out);
      if (!sh.damp.empty()) dparts.push_back(sh.damp);
    }
    if (!cat(out_path, parts) || (!damp_path.empty() && !cat(damp_path, dparts))) {
      fprintf(stderr, "raytracer: cannot assemble %s\n", out_path.c_str());
      return 1;
    }
  }
  printf(" %lld rays, %lld accepted steps\n", (long long)nrays, (long long)total_steps);
  if (timing) {
    // ours (--timing=1): wall clock per phase, max over the shards (they run side by side); the writer of chunk k runs beside
    // the trace of chunk k + 1, so trace_s + write_s may exceed wall_s
    double model_s = 0, trace_s = 0, write_s = 0;
    for (auto &sh : shards) {
      model_s = std::max(model_s, sh.model_s);
      trace_s = std::max(trace_s, sh.trace_s);
      write_s = std::max(write_s, sh.write_s);
    }
    long long bytes = 0;
    if (FILE *f = fopen(out_path.c_str(), "rb")) {
      if (fseeko(f, 0, SEEK_END) == 0) bytes = (long long)ftello(f);
      fclose(f);
    }
    printf(" timing: {\"parse_s\": %.3f, \"model_s\": %.3f, \"trace_s\": %.3f, \"write_s\": %.3f, \"wall_s\": %.3f, \"out_bytes\": %lld, "
           "\"first_attempt_policy\": %d, \"devices\": %d}\n", parse_s, model_s, trace_s, write_s, now_s() - t_start, bytes,
           (int)p.first_attempt_policy, ndev);
  }
  srt_free(pos0);
  srt_free(dir0);
  srt_free(w0);
  return 0;
}

static bool have_flag(const char *name) {
  std::string v;
  return getopt_named(name, v);
}
// a mode that is switched on with --name=<anything but 0>
static bool switched_on(const char *name) {
  std::string v;
  return getopt_named(name, v) && v != "0";
}

int main(int argc, char **argv) {
  g_argc = argc;
  g_argv = argv;
  if (argc == 1) {
    puts("Usage:\n  raytracer --param1=value1 --param2=value2 ...\n"
         "  --dt0 --dtmax --tmax --root --fixedstep --maxerr --maxsteps --minalt\n"
         "  --inputraysfile --outputfile --outputper\n"
         "  --modelnum  (1) Ngo model  (3) interpolated model (gridded)  (4) interpolated model (scattered)\n"
         "              (6) simplified GCPM (closed form)  (7) AT64ThCh (one field-line trace per evaluated point)\n"
         "  model 1: --ngo_configfile --yearday --milliseconds_day --use_tsyganenko=0|1 --use_igrf=0|1 --tsyganenko_Pdyn .. _W6\n"
         "  model 3: --interp_interpfile --yearday --milliseconds_day --use_tsyganenko=0|1 --use_igrf=0|1\n"
         "           [--interp_layout=expanded|nodes|auto: the table on the device; nodes = an eighth of the bytes, slower]\n"
         "  model 4: model 3 flags + --scattered_interp_window_scale --scattered_interp_order\n"
         "           --scattered_interp_exact --scattered_interp_local_window_scale\n"
         "           [--scattered_interp_root_sample=N: record N of the file is the root of the reference's kd-tree (spacing 0)]\n"
         "  model 6: --kp --yearday --milliseconds_day [--fixed_MLT=1 --MLT=<hours>] --use_tsyganenko=0|1 --use_igrf=0|1\n"
         "           --tsyganenko_Pdyn .. _W6  (--ngo_configfile is accepted and ignored, as by the reference's driver)\n"
         "  model 7: --gcpm_kp=<integer> --yearday --milliseconds_day --tsyganenko_Pdyn .. _W6 (all ten, also with\n"
         "           --use_tsyganenko=0: the model's field-line trace always runs through T04_s + IGRF)\n"
         "           --use_tsyganenko=0|1 --use_igrf=0|1 [--igrf_coeffs=<table>]\n"
         "  extra:   --device=N | --devices=0,1,..  --chunk_rays=N  --ray_order=0|1  --timing=1 (wall clock per phase)\n"
         "           --segment_rows=N: trace in segments of N kept rows per ray and launch (rays are paused and resumed; device\n"
         "             memory for chunk_rays * N rows instead of chunk_rays * maxsteps / outputper, the same .ray file; chunks of\n"
         "             262144 rays unless --chunk_rays says otherwise; not together with --damping_out).  0 / absent: one launch per chunk\n"
         "           --first_attempt_policy=1|0: error estimate of a ray's first adaptive attempt, where the reference reads an\n"
         "             unset variable: 1 (default) = from the k term alone, as the reference's gfortran build behaves;\n"
         "             0 = NaN => accepted at dt0, dt not grown, as a flang build behaves (the goldens of this repository)\n"
         "  tools:   --grid2bin_in=<text grid> --grid2bin_out=<binary grid>   (convert and exit; --interp_interpfile\n"
         "           accepts either form);  --pts2bin_in / --pts2bin_out: the same for model-4 sample files\n"
         "           --buildgrid=1 --filename=<out> --minx .. --maxz --nx --ny --nz --compder=0|1 (the reference's regular grid\n"
         "           builder gcpm_dens_model_buildgrid with the model of --modelnum in place of GCPM; --binary=1)\n"
         "           --buildsamples=1 --filename=<out> --minx .. --maxz --n_initial_uniform ... (the reference's random grid\n"
         "           builder with the model of --modelnum in place of GCPM; --seed, --binary=1)\n"
         "           --dumpmodel=1 --filename=<out> --minx .. --maxz --nx --ny --nz (the reference's dumpmodel: qs, Ns, ms, nus, B0\n"
         "           of the model of --modelnum at every node; an axis may have one node; --mag_coords=1 with model 6 or 7: the\n"
         "           grid is in MAG coordinates)\n"
         "           --damping_out=<file>: hot-plasma damping along the kept rows (raynum, row, t, rate, magnitude, flag);\n"
         "           with --damping_in=<.ray file> instead of tracing: along the records of an existing file\n"
         "           --crossings_in=<.ray file> --crossings_surfaces=<file> --crossings_out=<file> [--device=N]: where and when the\n"
         "           rays of an existing file cross surfaces, located on the cubic Hermite curve through consecutive records;\n"
         "           the surfaces file holds one `kind p0 p1 p2 p3` per line (0 sphere: radius in m; 1 L-shell: L; 2 magnetic\n"
         "           latitude: radians; 3 plane: normal and offset; trailing values may be absent); one record per crossing:\n"
         "           raynum, surface, interval, direction (4 i10), then t, pos, vprel, vgrel, n, B0, Ns (20 es24.15e3)\n"
         "           --approach_in=<.ray file> --approach_observers=<file> --approach_out=<file> [--device=N]: each ray's closest\n"
         "           approach to observer points, located on the cubic Hermite curve through consecutive records; the observers\n"
         "           file holds one `x y z radius` per line (SM metres; an approach is reported when it comes within the radius);\n"
         "           one record per event: raynum, observer, interval, 0 (4 i10), then the distance and t, pos, vprel, vgrel, n,\n"
         "           B0, Ns (21 es24.15e3)\n"
         "           --tube_in=<.ray file> --tube_neighbours=<file> --tube_out=<file> [--device=N]: the cross-section of ray tubes\n"
         "           (geometric spreading) at every record of their centre rays; the neighbours file holds one tube per line,\n"
         "           `centre b c`, as ray numbers of the .ray file; a neighbour is taken at the centre record's time on the cubic\n"
         "           Hermite curve through its own records; one record per centre record: raynum, record, flag (3 i10), then t, the\n"
         "           area vector (m^2) and its component along the group velocity (5 es24.15e3)\n"
         "           --bin_in=<.ray file> --bin_axes=<file> --bin_out=<file> [--bin_nsub=8] [--bin_quantum=9.313225746154785e-10]\n"
         "           [--device=N]: the dwell-time map of the rays of an existing file: every interval of consecutive records is cut\n"
         "           into bin_nsub pieces on the cubic Hermite curve, each deposits its duration into the cell of its midpoint, in\n"
         "           whole ticks of bin_quantum seconds; the axes file holds one axis per line, `kind n e0 e1 .. en` (kind 0 .. 7\n"
         "           or x y z r rho L sinlat mlt; metres, L, sine of the magnetic latitude, hours; 1 .. 3 axes of 1 .. 1024 cells);\n"
         "           the output holds the grid, then per cell seconds (es24.15e3) and samples (i20)");
    return 0;
  }
  if (have_flag("grid2bin_in") || have_flag("pts2bin_in")) return mode_convert();
  if (switched_on("buildgrid")) return mode_buildgrid();
  if (switched_on("buildsamples")) return mode_buildsamples();
  if (switched_on("dumpmodel")) return mode_dumpmodel();
  if (have_flag("damping_in")) return mode_damping_in();
  // (one flag of a post-processor's three selects it; the mode then names the ones that are missing)
  if (have_flag("approach_in") || have_flag("approach_observers") || have_flag("approach_out")) return mode_approach();
  if (have_flag("tube_in") || have_flag("tube_neighbours") || have_flag("tube_out")) return mode_tube();
  if (have_flag("crossings_in") || have_flag("crossings_surfaces") || have_flag("crossings_out")) return mode_crossings();
  if (have_flag("bin_in") || have_flag("bin_axes") || have_flag("bin_out")) return mode_bin();
  return mode_trace();
}
