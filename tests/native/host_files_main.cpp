// host_files_main.cpp -- the host file formats of libsrt_hip (csrc/srt_host.cpp, csrc/srt_scattered_host.cpp) driven by a
// stand-alone program, meant to be built with the address and undefined-behaviour sanitizers:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -pthread host_files_main.cpp
//       ../../stanford_raytracer_amd/csrc/srt_host.cpp ../../stanford_raytracer_amd/csrc/srt_scattered_host.cpp
//   ./host_files DIR [none|points|grid|both]
// Every writer writes small files into DIR, every reader reads them back and is then given files cut short or spoilt.  The
// second argument chooses which of two hostile files are read as well (default both): a 136-byte binary sample file whose
// header announces 2^40 samples, and a text grid that announces 100000^3 nodes ahead of four value lines.  Both must be
// refused, not answered with an allocation of what the header asks for.  Prints "ok <checks>" and exits 0, or names the
// first check that failed.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/srt.h"
#include "../../stanford_raytracer_amd/csrc/srt_host.hpp"

// ---- what the two sources take from the rest of the library
static char g_err[1024];
int srt_set_error(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code;
}
extern "C" int32_t srt_rows_per_ray(const srt_params *p) {
  const int per = p->outputper < 1 ? 1 : p->outputper;
  return (p->maxsteps + per - 1) / per;
}

static int g_checks = 0;
#define CHECK(cond)                                                                                  \
  do {                                                                                               \
    ++g_checks;                                                                                      \
    if (!(cond)) {                                                                                   \
      printf("FAILED line %d: %s   (last error: %s)\n", __LINE__, #cond, g_err);                     \
      exit(1);                                                                                       \
    }                                                                                                \
  } while (0)

static std::string g_dir;
static std::string in_dir(const char *name) { return g_dir + "/" + name; }
static std::string put(const char *name, const std::string &bytes) {
  const std::string p = in_dir(name);
  FILE *f = fopen(p.c_str(), "wb");
  if (!f || fwrite(bytes.data(), 1, bytes.size(), f) != bytes.size() || fclose(f) != 0) {
    printf("cannot write %s\n", p.c_str());
    exit(2);
  }
  return p;
}
static std::string slurp(const std::string &p) {
  std::string s;
  FILE *f = fopen(p.c_str(), "rb");
  if (!f) return s;
  char buf[65536];
  size_t k;
  while ((k = fread(buf, 1, sizeof buf, f)) > 0) s.append(buf, k);
  fclose(f);
  return s;
}
static bool refused(int rc, int code, const char *text) { return rc == code && strstr(g_err, text) != nullptr; }
// what sixteen significant digits keep of v, NaN compared as equal
static bool kept16(double got, double v) {
  if (std::isnan(v)) return std::isnan(got);
  char b[64];
  snprintf(b, sizeof b, "%.15E", v);
  return got == strtod(b, nullptr) && std::signbit(got) == std::signbit(v);
}
static std::vector<double> values(size_t n, int salt) {
  const double inf = std::numeric_limits<double>::infinity();
  const double special[7] = {std::nan(""), inf, -inf, -0.0, 5e-324, 1.7976931348623157e308, 9.9999999999999995e22};
  std::vector<double> v(n);
  for (size_t i = 0; i < n; ++i) {
    const double x = (double)(i + (size_t)salt);
    v[i] = i < 7 ? special[i] : std::ldexp((x + 1.0) * 0.1 * ((i & 1) ? -1.0 : 1.0), (int)((3 * (i + (size_t)salt)) % 120) - 60);
  }
  return v;
}
static const double B6[6] = {-3.0e7, 3.0e7, -2.0e7, 2.0e7, -1.0e7, 1.5e7};
static const double QS[4] = {-1.602e-19, 1.602e-19, 1.602e-19, 1.602e-19};
static const double MS[4] = {9.10938188e-31, 1.6726e-27, 6.6904e-27, 2.67616e-26};

// ---- model-3 grid files
static void grids() {
  for (int nspec = 1; nspec <= 4; nspec += 3)
    for (int with_derivs = 0; with_derivs < 2; ++with_derivs)
      for (int binary = 0; binary < 2; ++binary) {
        const size_t n = (size_t)8 * nspec;
        const std::vector<double> F = values(n, 1), D = values(7 * n, 10);
        const std::string p = in_dir("grid");
        CHECK(srt_grid_file_write(p.c_str(), binary, nspec, 2, 2, 2, B6, QS, MS, F.data(), with_derivs ? D.data() : nullptr) == SRT_OK);
        CHECK(srt_grid_file_is_binary(p.c_str()) == binary);
        int32_t dims[5];
        double b[6], q[4], m[4], *f = nullptr, *d = nullptr;
        CHECK(srt_grid_file_read(p.c_str(), dims, b, q, m, &f, &d) == SRT_OK);
        CHECK(dims[0] == with_derivs && dims[1] == nspec && dims[2] == 2 && dims[3] == 2 && dims[4] == 2 && (d != nullptr) == (with_derivs == 1));
        bool same = true;
        for (size_t i = 0; i < n; ++i) same = same && (binary ? (std::isnan(F[i]) ? std::isnan(f[i]) : f[i] == F[i]) : kept16(f[i], F[i]));
        for (size_t i = 0; d && i < 7 * n; ++i) same = same && (binary ? (std::isnan(D[i]) ? std::isnan(d[i]) : d[i] == D[i]) : kept16(d[i], D[i]));
        for (int k = 0; k < 6; ++k) same = same && kept16(b[k], B6[k]);
        for (int k = 0; k < nspec; ++k) same = same && kept16(q[k], QS[k]) && kept16(m[k], MS[k]);
        CHECK(same);
        srt_free(f);
        srt_free(d);
        if (!binary) {
          const std::string c = in_dir("grid.conv");
          CHECK(srt_grid_file_convert(p.c_str(), c.c_str()) == SRT_OK && srt_grid_file_is_binary(c.c_str()) == 1);
          CHECK(slurp(c).size() == 144 + n * 8 * (with_derivs ? 8 : 1));
        }
      }
  // a text file large enough for the reader to cut it into pieces: 12 x 12 x 12 x 4 values, 172 KB
  const size_t n = 12 * 12 * 12 * 4;
  const std::vector<double> F = values(n, 9);
  const std::string big = in_dir("grid.big");
  CHECK(srt_grid_file_write(big.c_str(), 0, 4, 12, 12, 12, B6, QS, MS, F.data(), nullptr) == SRT_OK);
  int32_t dims[5];
  double b[6], q[4], m[4], *f = nullptr;
  CHECK(srt_grid_file_read(big.c_str(), dims, b, q, m, &f, nullptr) == SRT_OK);
  bool same = true;
  for (size_t i = 0; i < n; ++i) same = same && kept16(f[i], F[i]);
  CHECK(same);
  srt_free(f);
  // spoilt files
  CHECK(srt_grid_file_write(big.c_str(), 0, 1, 2, 2, 2, B6, QS, MS, F.data() + 8, F.data() + 16) == SRT_OK);
  const std::string text = slurp(big);
  CHECK(text.size() == 51 + 6 * 24 + 1 + 25 + 25 + 64 * 25);
  const size_t body = 51 + 6 * 24 + 1 + 25 + 25;
  struct { size_t keep; const char *why; } cuts[] = {{30, "size header incomplete"}, {51 + 72, "bounds incomplete"},
                                                      {51 + 145, "charges incomplete"}, {51 + 145 + 25, "masses incomplete"},
                                                      {body + 3 * 25, "grid values truncated"}, {body + 20 * 25, "derivative block truncated"}};
  for (auto &c : cuts) {
    const std::string p = put("grid.cut", text.substr(0, c.keep) + "\n");
    CHECK(refused(srt_grid_file_read(p.c_str(), dims, b, q, m, &f, nullptr), SRT_EIO, c.why));
  }
  std::string t = text;
  t.replace(body + 25, 24, "                     xyz");
  CHECK(refused(srt_grid_file_read(put("grid.token", t).c_str(), dims, b, q, m, &f, nullptr), SRT_EIO, "grid values truncated"));
  const char *heads[3] = {"         0         0         2         2         2\n", "         0         5         2         2         2\n",
                          "         0         1         2         1         2\n"};
  for (int k = 0; k < 3; ++k)
    CHECK(refused(srt_grid_file_read(put("grid.head", heads[k] + text.substr(51)).c_str(), dims, b, q, m, &f, nullptr), SRT_EIO,
                  k < 2 ? "nspec must be 1..4" : "grid needs >= 2 nodes per axis"));
  // records with a field more than their READ takes: the Fortran's record semantics
  std::string wide = "         0" + text.substr(10, body - 10);
  for (size_t i = 0; i < 8; ++i) wide += text.substr(body + i * 25, 24) + " 9.0\n";
  CHECK(srt_grid_file_read(put("grid.wide", wide).c_str(), dims, b, q, m, &f, nullptr) == SRT_OK && dims[0] == 0);
  same = true;
  for (size_t i = 0; i < 8; ++i) same = same && kept16(f[i], F[8 + i]);
  CHECK(same);
  srt_free(f);
  CHECK(srt_grid_file_write(big.c_str(), 1, 1, 2, 2, 2, B6, QS, MS, F.data() + 8, F.data() + 16) == SRT_OK);
  const std::string raw = slurp(big);
  CHECK(raw.size() == 144 + 64 * 8);
  CHECK(refused(srt_grid_file_read(put("grid.bcut", raw.substr(0, 100)).c_str(), dims, b, q, m, &f, nullptr), SRT_EIO, "binary grid: header truncated"));
  CHECK(refused(srt_grid_file_read(put("grid.bcut", raw.substr(0, 400)).c_str(), dims, b, q, m, &f, nullptr), SRT_EIO, "binary grid: value block truncated"));
  CHECK(srt_grid_file_is_binary(put("grid.magic", "SRTGRID2" + raw.substr(8)).c_str()) == 0);
  CHECK(refused(srt_grid_file_read(in_dir("grid.none").c_str(), dims, b, q, m, &f, nullptr), SRT_EIO, "cannot open"));
  CHECK(refused(srt_grid_file_write(in_dir("no/such").c_str(), 0, 1, 2, 2, 2, B6, QS, MS, F.data(), nullptr), SRT_EIO, "cannot open for writing"));
}

// ---- model-4 sample files: samples between 2 and 3 Earth radii, read back through the model's host preparation
static void points() {
  const double RE = 6371.2e3;
  for (int nspec = 1; nspec <= 4; nspec += 3) {
    const int w = 3 + nspec;
    std::vector<double> rec((size_t)5 * w);
    for (int i = 0; i < 5; ++i) {
      rec[(size_t)i * w] = (2.0 + 0.2 * i) * RE;
      rec[(size_t)i * w + 1] = 0.1 * i * RE;
      rec[(size_t)i * w + 2] = -0.3 * i * RE;
      for (int k = 0; k < nspec; ++k) rec[(size_t)i * w + 3 + k] = 20.0 + i + 0.5 * k;
    }
    const std::string txt = in_dir("pts.txt"), bin = in_dir("pts.bin"), conv = in_dir("pts.conv");
    CHECK(srt_points_file_write(txt.c_str(), 0, nspec, 5, B6, QS, MS, rec.data()) == SRT_OK && srt_points_file_is_binary(txt.c_str()) == 0);
    CHECK(srt_points_file_write(bin.c_str(), 1, nspec, 5, B6, QS, MS, rec.data()) == SRT_OK && srt_points_file_is_binary(bin.c_str()) == 1);
    CHECK(srt_points_file_convert(txt.c_str(), conv.c_str()) == SRT_OK);
    CHECK(slurp(bin).size() == 136 + (size_t)5 * w * 8 && slurp(conv).size() == slurp(bin).size());
    CHECK(refused(srt_points_file_convert(bin.c_str(), conv.c_str()), SRT_EINVAL, "is already binary"));
    std::string text = slurp(txt);
    // the same samples with a field more on every record: record semantics, one READ at a time
    std::string wide;
    for (size_t at = 0, line = 0; at < text.size(); ++line) {
      const size_t nl = text.find('\n', at);
      wide += text.substr(at, nl - at) + (line >= 4 ? " 7.0\n" : "\n");
      at = nl + 1;
    }
    const std::string files[3] = {txt, bin, put("pts.wide", wide)};
    for (const std::string &p : files) {
      srt_host::ScatteredHost h;
      std::string err;
      CHECK(srt_host::build_scattered(p.c_str(), 1.5, h, err));
      CHECK(h.nspec == nspec && h.npts == 5 && h.pts.size() == 40 && h.radius > 0.0);
      bool same = true;
      for (int k = 0; k < nspec; ++k) same = same && kept16(h.qs[k], QS[k]) && kept16(h.ms[k], MS[k]);
      double sum = 0.0, want = 0.0;
      for (int i = 0; i < 5; ++i) {
        sum += h.pts[(size_t)i * 8] + h.pts[(size_t)i * 8 + 3];
        want += rec[(size_t)i * w] + rec[(size_t)i * w + 3];
      }
      CHECK(same && std::fabs(sum - want) <= 1e-9 * want);
    }
    srt_host::ScatteredHost h;
    std::string err;
    const std::string raw = slurp(bin);
    CHECK(!srt_host::build_scattered(put("pts.cut", raw.substr(0, 100)).c_str(), 1.5, h, err) && err == "truncated or malformed binary sample file");
    CHECK(!srt_host::build_scattered(put("pts.cut", raw.substr(0, raw.size() - 8)).c_str(), 1.5, h, err) && err == "truncated or malformed binary sample file");
    std::string five = raw;
    five[8] = 5;
    CHECK(!srt_host::build_scattered(put("pts.five", five).c_str(), 1.5, h, err) && err == "truncated or malformed binary sample file");
    CHECK(!srt_host::build_scattered(put("pts.head", text.substr(0, 11 + 72) + "\n").c_str(), 1.5, h, err) && err == "header (nspec + bounds) incomplete");
    CHECK(!srt_host::build_scattered(put("pts.head", text.substr(0, 11 + 145 + 24 * nspec) + "\n").c_str(), 1.5, h, err) && err == "charges/masses incomplete");
    CHECK(!srt_host::build_scattered(put("pts.head", text.substr(0, 11 + 145 + 2 * (24 * nspec + 1))).c_str(), 1.5, h, err) && err == "no samples");
    CHECK(!srt_host::build_scattered(put("pts.head", "         9" + text.substr(10)).c_str(), 1.5, h, err) && err.compare(0, 18, "nspec must be 1..4") == 0);
    CHECK(!srt_host::build_scattered(in_dir("pts.none").c_str(), 1.5, h, err) && err == "cannot open");
    CHECK(refused(srt_points_file_convert(put("pts.short", text.substr(0, 11 + 72) + "\n").c_str(), conv.c_str()), SRT_EIO, "too short"));
    CHECK(refused(srt_points_file_convert(put("pts.short", text.substr(0, text.size() - 30) + "\n").c_str(), conv.c_str()), SRT_EIO, "not a model-4 sample file"));
    CHECK(refused(srt_points_file_convert(put("pts.tok", text + "a b\n").c_str(), conv.c_str()), SRT_EIO, "non-numeric token"));
    CHECK(srt_points_file_is_binary(put("pts.magic", "SRTPTS02" + raw.substr(8)).c_str()) == 0);
    CHECK(refused(srt_points_file_write(in_dir("no/such").c_str(), 0, nspec, 5, B6, QS, MS, rec.data()), SRT_EIO, "cannot open for writing"));
  }
}

// ---- dump files
static void dumps() {
  const int shapes[2][4] = {{1, 1, 1, 1}, {4, 2, 1, 3}};
  for (auto &s : shapes) {
    const size_t n = (size_t)(4 * s[0] + 3) * s[1] * s[2] * s[3];
    const std::vector<double> f = values(n, 3);
    const std::string p = in_dir("dump");
    CHECK(srt_dump_file_write(p.c_str(), s[0], s[1], s[2], s[3], B6, f.data()) == SRT_OK);
    int32_t dims[4];
    double b[6], *g = nullptr;
    CHECK(srt_dump_file_read(p.c_str(), dims, b, &g) == SRT_OK && dims[0] == s[0] && dims[1] == s[1] && dims[2] == s[2] && dims[3] == s[3]);
    bool same = true;
    for (size_t i = 0; i < n; ++i) same = same && kept16(g[i], f[i]);
    CHECK(same);
    srt_free(g);
    const std::string text = slurp(p);
    CHECK(refused(srt_dump_file_read(put("dump.cut", text.substr(0, 41 + 96) + "\n").c_str(), dims, b, &g), SRT_EIO, "dump file header incomplete"));
    CHECK(refused(srt_dump_file_read(put("dump.cut", text.substr(0, text.size() - 25)).c_str(), dims, b, &g), SRT_EIO, "announces"));
    CHECK(refused(srt_dump_file_read(put("dump.tok", text + "1.0x\n").c_str(), dims, b, &g), SRT_EIO, "non-numeric token"));
    CHECK(refused(srt_dump_file_read(put("dump.five", "         5" + text.substr(10)).c_str(), dims, b, &g), SRT_EIO, "nspec = 5"));
  }
  CHECK(refused(srt_dump_file_write(in_dir("no/such").c_str(), 1, 1, 1, 1, B6, B6), SRT_EIO, "cannot open for writing"));
}

// ---- crossings, approaches and tubes files
static void events_and_tubes() {
  const int64_t raynum[3] = {1, 9999999999ll, 42}, big[1] = {10000000000ll};
  const int32_t meta[12] = {0, 0, 0, 1, 1, 15, 2147483646, -1, 2, 3, 7, 0};
  const std::vector<double> rows = values(3 * SRT_ROW, 4), dist = values(3, 5);
  for (int ne = 0; ne <= 3; ++ne) {
    const std::string c = in_dir("crossings"), a = in_dir("approaches");
    CHECK(srt_crossings_file_write(c.c_str(), ne, raynum, meta, rows.data()) == SRT_OK && slurp(c).size() == (size_t)ne * (40 + 20 * 24 + 1));
    CHECK(srt_approaches_file_write(a.c_str(), ne, raynum, meta, dist.data(), rows.data()) == SRT_OK && slurp(a).size() == (size_t)ne * (40 + 21 * 24 + 1));
  }
  CHECK(slurp(in_dir("crossings")).compare(0, 64, "         1         1         1         1                     NaN") == 0);
  CHECK(refused(srt_crossings_file_write(in_dir("x").c_str(), 1, big, meta, rows.data()), SRT_EINVAL, "srt_crossings_file_write: ray number 10000000000 of event 0 does not fit"));
  CHECK(refused(srt_approaches_file_write(in_dir("no/such").c_str(), 1, raynum, meta, dist.data(), rows.data()), SRT_EIO, "cannot open for writing"));
  const int64_t offsets[3] = {0, 2, 5}, first[3] = {1, 2, 5}, down[3] = {0, 3, 2}, two[2] = {7, 9999999999ll};
  const int32_t flag[5] = {0, 1, 2, 0, 5};
  const std::vector<double> prow = values(5 * SRT_ROW, 6), section = values(20, 7);
  const std::string t = in_dir("tubes");
  CHECK(srt_tubes_file_write(t.c_str(), 2, two, offsets, prow.data(), section.data(), flag) == SRT_OK && slurp(t).size() == (size_t)4 * (30 + 5 * 24 + 1));
  CHECK(slurp(t).compare(151, 30, "9999999999         1         2") == 0);
  CHECK(refused(srt_tubes_file_write(t.c_str(), 2, two, first, prow.data(), section.data(), flag), SRT_EINVAL, "srt_tubes_file_write: offsets[0] = 1"));
  CHECK(refused(srt_tubes_file_write(t.c_str(), 2, two, down, prow.data(), section.data(), flag), SRT_EINVAL, "srt_tubes_file_write: offsets decrease at ray 1"));
  CHECK(refused(srt_tubes_file_write(t.c_str(), 1, big, offsets, prow.data(), section.data(), flag), SRT_EINVAL, "ray number 10000000000 of ray 0"));
}

// ---- bin files
static void bins() {
  const double e0[3] = {-1.0e7, 0.5, 2.0e7}, e1[2] = {-1.0, 1.0}, e2[4] = {6.4e6, 7.0e6, 1.0e7, 5.0e7};
  srt_bin_params p;
  memset(&p, 0, sizeof p);
  p.naxes = 3, p.nsub = 3, p.quantum = 0.1;
  p.axis[0] = {0, 2, e0}, p.axis[1] = {6, 1, e1}, p.axis[2] = {3, 3, e2};
  const int64_t ticks[6] = {0, 1, (int64_t)1 << 62, 3, 4, 5}, hits[6] = {0, 9, (int64_t)1 << 40, 1, 2, 3};
  const std::string path = in_dir("bin");
  for (int k = 0; k < 4; ++k) {
    CHECK(srt_bin_file_write(path.c_str(), &p, (k & 1) ? nullptr : ticks, (k & 2) ? nullptr : hits) == SRT_OK);
    srt_bin_params q;
    double *ed = nullptr, *sum = nullptr;
    int64_t nc = 0, *hh = nullptr;
    CHECK(srt_bin_file_read(path.c_str(), &q, &ed, &nc, &sum, &hh) == SRT_OK && nc == 6 && q.naxes == 3 && q.nsub == 3 && q.axis[2].n == 3);
    bool same = kept16(q.quantum, 0.1) && q.axis[2].edges[3] == 5.0e7;
    for (int c = 0; c < 6; ++c) same = same && kept16(sum[c], (k & 1) ? 0.0 : (double)ticks[c] * 0.1) && hh[c] == ((k & 2) ? 0 : hits[c]);
    CHECK(same);
    srt_free(ed), srt_free(sum), srt_free(hh);
  }
  const std::string text = slurp(path);
  srt_bin_params q;
  double *ed = nullptr, *sum = nullptr;
  int64_t nc = 0, *hh = nullptr;
  CHECK(refused(srt_bin_file_read(put("bin.cut", text.substr(0, 20) + "\n").c_str(), &q, &ed, &nc, &sum, &hh), SRT_EIO, "bin file header"));
  CHECK(refused(srt_bin_file_read(put("bin.cut", text.substr(0, 45 + 21 + 48) + "\n").c_str(), &q, &ed, &nc, &sum, &hh), SRT_EIO, "the edges of axis 0 are cut short"));
  CHECK(refused(srt_bin_file_read(put("bin.cut", text.substr(0, text.size() - 45)).c_str(), &q, &ed, &nc, &sum, &hh), SRT_EIO, "announces 6 cells of two"));
  CHECK(refused(srt_bin_file_read(put("bin.tok", text + "nope\n").c_str(), &q, &ed, &nc, &sum, &hh), SRT_EIO, "non-numeric token"));
  CHECK(refused(srt_bin_file_write(in_dir("no/such").c_str(), &p, ticks, hits), SRT_EIO, "cannot open for writing"));
}

// ---- .ray files, padded and packed, and the launch-set file
static void rays() {
  srt_params p;
  memset(&p, 0, sizeof p);
  p.maxsteps = 3, p.outputper = 1;
  std::vector<double> rows = values(2 * 3 * SRT_ROW, 8);
  for (int r = 0; r < 2; ++r)
    for (int s = 0; s < 3; ++s) rows[(size_t)(r * 3 + s) * SRT_ROW] = 1e-3 * s;
  const double w0[2] = {1.0e4, 5e-324};
  const int32_t nrows[2] = {3, 2}, none[1] = {0}, stop[2] = {0, 6};
  const int64_t offsets[3] = {0, 3, 5}, empty[2] = {0, 0};
  std::vector<double> packed(rows.begin(), rows.begin() + 5 * SRT_ROW);
  for (int nspec = 1; nspec <= 4; nspec += 3)
    for (const char *threads : {"1", "3"}) {
      setenv("SRT_IO_THREADS", threads, 1);
      const std::string a = in_dir("a.ray"), b = in_dir("b.ray");
      const size_t L = 20 + 17 * 24 + 10 + (size_t)4 * nspec * 24 + 1;
      CHECK(srt_write_ray_file(a.c_str(), 0, 1, 0, &p, nspec, QS, MS, w0, rows.data(), nrows, stop) == SRT_OK && slurp(a).empty());
      CHECK(srt_write_ray_file_packed(b.c_str(), 0, 1, 0, nspec, QS, MS, nullptr, empty, nullptr, nullptr) == SRT_OK && slurp(b).empty());
      CHECK(srt_write_ray_file(a.c_str(), 0, 1, 1, &p, nspec, QS, MS, w0, rows.data(), none, stop) == SRT_OK && slurp(a).empty());
      CHECK(srt_write_ray_file_packed(b.c_str(), 0, 1, 1, nspec, QS, MS, w0, empty, nullptr, stop) == SRT_OK && slurp(b).empty());
      for (int append = 0; append < 2; ++append) {
        CHECK(srt_write_ray_file(a.c_str(), append, 1 + 2 * append, 2, &p, nspec, QS, MS, w0, rows.data(), nrows, stop) == SRT_OK);
        CHECK(srt_write_ray_file_packed(b.c_str(), append, 1 + 2 * append, 2, nspec, QS, MS, w0, offsets, packed.data(), stop) == SRT_OK);
        CHECK(slurp(a).size() == (size_t)5 * (1 + append) * L && slurp(a) == slurp(b));
      }
      int32_t ns = 0, *sc = nullptr, *kept = nullptr;
      int64_t nrec = 0, *rn = nullptr;
      double q[4], m[4], *w = nullptr, *back = nullptr;
      CHECK(srt_read_ray_file(a.c_str(), &ns, q, m, &nrec, &rn, &sc, &kept, &w, &back) == 4 && ns == nspec && nrec == 10);
      bool same = rn[0] == 1 && rn[3] == 4 && kept[0] == 3 && kept[3] == 2 && sc[1] == 6 && kept16(w[1], 5e-324);
      for (int i = 0; i < 5 * SRT_ROW; ++i)
        if (i % SRT_ROW < 16 + nspec) same = same && kept16(back[i], packed[i]) && kept16(back[5 * SRT_ROW + i], packed[i]);
      CHECK(same);
      srt_free(rn), srt_free(sc), srt_free(kept), srt_free(w), srt_free(back);
      const std::string text = slurp(a);
      CHECK(refused((int)srt_read_ray_file(put("c.ray", text.substr(0, 300) + "\n").c_str(), &ns, q, m, &nrec, &rn, &sc, &kept, &w, &back), SRT_EIO, "truncated record"));
      CHECK(refused((int)srt_read_ray_file(put("c.ray", text.substr(0, text.size() - 49) + "\n").c_str(), &ns, q, m, &nrec, &rn, &sc, &kept, &w, &back), SRT_EIO, "are not a whole number of"));
      CHECK(refused((int)srt_read_ray_file(put("c.ray", text + "***\n").c_str(), &ns, q, m, &nrec, &rn, &sc, &kept, &w, &back), SRT_EIO, "non-numeric token"));
      CHECK(srt_read_ray_file(put("c.ray", "").c_str(), &ns, q, m, &nrec, &rn, &sc, &kept, &w, &back) == 0 && nrec == 0);
      srt_free(rn), srt_free(sc), srt_free(kept), srt_free(w), srt_free(back);
    }
  CHECK(refused(srt_write_ray_file(in_dir("x.ray").c_str(), 0, 9999999999ll, 2, &p, 1, QS, MS, w0, rows.data(), nrows, stop), SRT_EINVAL, "ray numbers 9999999999 .. 10000000000 do not fit"));
  const int64_t first[3] = {1, 3, 5}, down[3] = {0, 3, 2};
  CHECK(refused(srt_write_ray_file_packed(in_dir("x.ray").c_str(), 0, 1, 2, 1, QS, MS, w0, first, packed.data(), stop), SRT_EINVAL, "offsets[0] = 1: the first ray's rows start at 0"));
  CHECK(refused(srt_write_ray_file_packed(in_dir("x.ray").c_str(), 0, 1, 2, 1, QS, MS, w0, down, packed.data(), stop), SRT_EINVAL, "offsets decrease at ray 1") && strncmp(g_err, "offsets", 7) == 0);
  CHECK(refused(srt_write_ray_file(in_dir("no/such").c_str(), 0, 1, 2, &p, 1, QS, MS, w0, rows.data(), nrows, stop), SRT_EIO, "cannot open for writing"));
  double *pos = nullptr, *dir = nullptr, *w = nullptr;
  CHECK(srt_read_rays_file(put("rays", "1 2 3 0 0 1 5000.\n1d0,2,3 , 0 0 1 6.0D3\n 1 2 3\n").c_str(), &pos, &dir, &w) == 2 && pos[3] == 1.0 && dir[5] == 1.0 && w[1] == 6000.0);
  srt_free(pos), srt_free(dir), srt_free(w);
  CHECK(srt_read_rays_file(put("rays", "").c_str(), &pos, &dir, &w) == 0);
  srt_free(pos), srt_free(dir), srt_free(w);
  CHECK(refused((int)srt_read_rays_file(in_dir("rays.none").c_str(), &pos, &dir, &w), SRT_EIO, "cannot open"));
}

// ---- the two files whose headers ask for more than the file can hold
static void hostile_points() {
  std::string head(136, '\0');
  memcpy(&head[0], "SRTPTS01", 8);
  const int32_t nspec = 4;
  const int64_t npts = (int64_t)1 << 40;
  memcpy(&head[8], &nspec, 4);
  memcpy(&head[16], &npts, 8);
  srt_host::ScatteredHost h;
  std::string err;
  CHECK(!srt_host::build_scattered(put("pts.hostile", head).c_str(), 1.5, h, err) && err == "truncated or malformed binary sample file");
  const int64_t most = std::numeric_limits<int64_t>::max(); // (npts * (3 + nspec) * 8 wraps round 64 bits)
  memcpy(&head[16], &most, 8);
  CHECK(!srt_host::build_scattered(put("pts.hostile", head + std::string(56, '\0')).c_str(), 1.5, h, err) && err == "truncated or malformed binary sample file");
}
static void hostile_grid() {
  int32_t dims[5];
  double b[6], q[4], m[4], *f = nullptr;
  const std::string head = "0 4 100000 100000 100000\n-1 1 -1 1 -1 1\n-1 1 1 1\n1 2 3 4\n";
  const std::string four = "1 2 3 4\n1 2 3 4\n1 2 3 4\n1 2 3 4\n";
  CHECK(refused(srt_grid_file_read(put("grid.hostile", head + four).c_str(), dims, b, q, m, &f, nullptr), SRT_EIO, "grid values truncated"));
  // 2 x 2 x 2 nodes of one species whose values are there, and seven derivative blocks that are not
  CHECK(refused(srt_grid_file_read(put("grid.hostile", "1 1 2 2 2\n-1 1 -1 1 -1 1\n-1\n1\n1\n2\n3\n4\n5\n6\n7\n8\n9\n").c_str(), dims, b, q, m, &f, nullptr), SRT_EIO,
                "derivative block truncated"));
}

int main(int argc, char **argv) {
  if (argc < 2) {
    printf("usage: %s DIR [none|points|grid|both]\n", argv[0]);
    return 2;
  }
  g_dir = argv[1];
  const std::string hostile = argc > 2 ? argv[2] : "both";
  grids();
  points();
  dumps();
  events_and_tubes();
  bins();
  rays();
  if (hostile == "points" || hostile == "both") hostile_points();
  if (hostile == "grid" || hostile == "both") hostile_grid();
  printf("ok %d\n", g_checks);
  return 0;
}
