// srt_host.cpp -- host-side file formats of the drop-in boundary (no device code).
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <thread>

#include "srt_host.hpp"
#include "srt_xform.hpp"
#define SRT_BINNING_NO_KERNELS
#include "srt_binning.hpp"

#include <charconv>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/srt.h"

int srt_set_error(int code, const char *fmt, ...);

namespace srt_host {

// ---------------------------------------------------------------------------------------------
// xform_double: get_q_c_d (Get_q_c.f95:4-30) -> t1_d inverse (T1.f95) -> t2_d (T2.f95) -> mu (T4.f95): the angles of the
// whole chain T1 .. T5 are computed in one place, srt_xform.hpp
double dipole_tilt(int yearday, int msec) { return srt::xform::angles(yearday, msec).mu; }

// ---------------------------------------------------------------------------------------------
// IGRF set-up for one date (host, once per model): what RECALC_08 leaves in COMMON /GEOPACK1/ and /GEOPACK2/ that
// IGRF_GSW_08 reads.  Everything is default REAL in the Fortran, so everything is float here; SUN_08's two DOUBLE
// PRECISION variables are double (geopack2008.for:333-381, :486-1196).
namespace {
struct SunAngles {
  float gst = 0.f, srasn = 0.f, sdec = 0.f;
};
SunAngles sun_angles(int iyear, int iday, int ihour, int min, int isec) {
  SunAngles o;
  const float RAD = 57.295779513f;
  if (iyear < 1901 || iyear > 2099) return o;
  const double fday = (double)(ihour * 3600 + min * 60 + isec) / 86400.0;
  const double dj = 365 * (iyear - 1900) + (iyear - 1901) / 4 + iday - 0.5 + fday;
  const float t = (float)(dj / (double)36525.f);
  const float vl = (float)std::fmod((double)279.696678f + (double)0.9856473354f * dj, 360.0);
  o.gst = (float)(std::fmod((double)279.690983f + (double).9856473354f * dj + (double)360.f * fday + (double)180.f, 360.0) / (double)RAD);
  const float g = (float)(std::fmod((double)358.475845f + (double)0.985600267f * dj, 360.0) / (double)RAD);
  float slong = (vl + (1.91946f - 0.004789f * t) * sinf(g) + 0.020094f * sinf(2.f * g)) / RAD;
  if (slong > 6.2831853f) slong = slong - 6.2831853f;
  if (slong < 0.f) slong = slong + 6.2831853f;
  const float obliq = (23.45229f - 0.0130125f * t) / RAD;
  const float sob = sinf(obliq), slp = slong - 9.924e-5f;
  const float sind = sob * sinf(slp);
  const float cosd = sqrtf(1.f - sind * sind);
  const float sc = sind / cosd;
  o.sdec = atanf(sc);
  o.srasn = 3.141592654f - atan2f(cosf(obliq) / sob * sc, -cosf(slp) / cosd);
  return o;
}
} // namespace

bool igrf_setup(const char *coeff_file, int yearday, int msec, float G[105], float H[105], float REC[105], float A[9],
                float *psi, std::string &err, float *geopack_psi) {
  // table: "g|h mn v1965 v1970 ... v2020 sv"
  static const int NEP = 12;
  std::vector<float> tg(13 * 105, 0.f), th(13 * 105, 0.f);
  FILE *f = fopen(coeff_file, "r");
  if (!f) {
    err = std::string("cannot open IGRF coefficient table ") + coeff_file;
    return false;
  }
  char line[2048];
  int seen = 0;
  while (fgets(line, sizeof line, f)) {
    if (line[0] != 'g' && line[0] != 'h') continue;
    char *s = line + 1;
    const long mn = strtol(s, &s, 10);
    if (mn < 1 || mn > 105) continue;
    for (int e = 0; e <= NEP; ++e) {
      char *end = s;
      (line[0] == 'g' ? tg : th)[e * 105 + (mn - 1)] = strtof(s, &end);
      if (end == s) { // a row cut short (a truncated file): never a silent zero
        fclose(f);
        err = std::string("IGRF coefficient table has a row with fewer than 13 values: ") + coeff_file;
        return false;
      }
      s = end;
    }
    ++seen;
  }
  fclose(f);
  if (seen != 210) {
    err = std::string("IGRF coefficient table has the wrong number of rows: ") + coeff_file;
    return false;
  }
  // itime -> calendar fields as the adapters do (interp_dens_model_adapter.f95:217-221)
  const int iyear = yearday / 1000, iday = yearday % 1000;
  const int ihour = msec / (1000 * 60 * 60);
  const int min = (msec - ihour * (1000 * 60 * 60)) / (1000 * 60);
  const int isec = (msec - ihour * (1000 * 60 * 60) - min * (1000 * 60)) / 1000;
  int iy = iyear < 1965 ? 1965 : iyear > 2025 ? 2025 : iyear;
  for (int n = 1; n <= 14; ++n) {
    const int n2 = (2 * n - 1) * (2 * n - 3);
    for (int m = 1; m <= n; ++m) REC[n * (n - 1) / 2 + m - 1] = (float)((n - m) * (n + m - 2)) / (float)n2;
  }
  const float yfrac = (float)iy + (float)(iday - 1) / 365.25f;
  if (iy >= 2020) { // extrapolate: secular variation for degrees <= 8 (the first 45 entries)
    const float dt = yfrac - 2020.f;
    for (int n = 0; n < 105; ++n) {
      G[n] = tg[11 * 105 + n];
      H[n] = th[11 * 105 + n];
      if (n < 45) {
        G[n] = G[n] + tg[12 * 105 + n] * dt;
        H[n] = H[n] + th[12 * 105 + n] * dt;
      }
    }
  } else { // interpolate between the two bracketing epochs
    const int e = (iy - 1965) / 5;
    const float f2 = (yfrac - (float)(1965 + 5 * e)) / 5.f, f1 = 1.f - f2;
    for (int n = 0; n < 105; ++n) {
      G[n] = tg[e * 105 + n] * f1 + tg[(e + 1) * 105 + n] * f2;
      H[n] = th[e * 105 + n] * f1 + th[(e + 1) * 105 + n] * f2;
    }
  }
  // Gauss -> Schmidt quasi-normalised
  float s = 1.f;
  for (int n = 2; n <= 14; ++n) {
    const int mn = n * (n - 1) / 2 + 1;
    s = s * (float)(2 * n - 3) / (float)(n - 1);
    G[mn - 1] = G[mn - 1] * s;
    H[mn - 1] = H[mn - 1] * s;
    float p = s;
    for (int m = 2; m <= n; ++m) {
      const float aa = m == 2 ? 2.f : 1.f;
      p = p * sqrtf(aa * (float)(n - m + 1) / (float)(n + m - 2));
      G[mn + m - 2] = G[mn + m - 2] * p;
      H[mn + m - 2] = H[mn + m - 2] * p;
    }
  }
  // dipole axis in GEO, Sun direction, GSE/GSW axes, GEO -> GSW rotation
  const float g10 = -G[1], g11 = G[2], h11 = H[2];
  const float sq = g11 * g11 + h11 * h11, sqq = sqrtf(sq), sqr = sqrtf(g10 * g10 + sq);
  const float sl0 = -h11 / sqq, cl0 = -g11 / sqq, st0 = sqq / sqr, ct0 = g10 / sqr;
  const float stcl = st0 * cl0, stsl = st0 * sl0;
  const SunAngles sun = sun_angles(iy, iday, ihour, min, isec);
  const float s1 = cosf(sun.srasn) * cosf(sun.sdec), s2 = sinf(sun.srasn) * cosf(sun.sdec), s3 = sinf(sun.sdec);
  const float dj = (float)(365 * (iy - 1900) + (iy - 1901) / 4 + iday) - 0.5f + (float)(ihour * 3600 + min * 60 + isec) / 86400.f;
  const float t = dj / 36525.f;
  const float obliq = (23.45229f - 0.0130125f * t) / 57.2957795f;
  const float dz1 = 0.f, dz2 = -sinf(obliq), dz3 = cosf(obliq);
  const float dy1 = dz2 * s3 - dz3 * s2, dy2 = dz3 * s1 - dz1 * s3, dy3 = dz1 * s2 - dz2 * s1;
  const float vx = -400.f, vy = 0.f, vz = 0.f; // tsy_recalc's solar wind: GSW coincides with GSM
  const float v = sqrtf(vx * vx + vy * vy + vz * vz);
  const float dx1 = -vx / v, dx2 = -vy / v, dx3 = -vz / v;
  const float x1 = dx1 * s1 + dx2 * dy1 + dx3 * dz1, x2 = dx1 * s2 + dx2 * dy2 + dx3 * dz2, x3 = dx1 * s3 + dx2 * dy3 + dx3 * dz3;
  const float cgst = cosf(sun.gst), sgst = sinf(sun.gst);
  const float dip1 = stcl * cgst - stsl * sgst, dip2 = stcl * sgst + stsl * cgst, dip3 = ct0;
  float y1 = dip2 * x3 - dip3 * x2, y2 = dip3 * x1 - dip1 * x3, y3 = dip1 * x2 - dip2 * x1;
  const float y = sqrtf(y1 * y1 + y2 * y2 + y3 * y3);
  y1 = y1 / y;
  y2 = y2 / y;
  y3 = y3 / y;
  const float z1 = x2 * y3 - x3 * y2, z2 = x3 * y1 - x1 * y3, z3 = x1 * y2 - x2 * y1;
  A[0] = x1 * cgst + x2 * sgst;
  A[1] = -x1 * sgst + x2 * cgst;
  A[2] = x3;
  A[3] = y1 * cgst + y2 * sgst;
  A[4] = -y1 * sgst + y2 * cgst;
  A[5] = y3;
  A[6] = z1 * cgst + z2 * sgst;
  A[7] = -z1 * sgst + z2 * cgst;
  A[8] = z3;
  if (psi) {
    // What the adapters pass to T04_s as the tilt angle: they declare `real(kind=SP) :: PSI; COMMON /GEOPACK1/ PSI`
    // (interp_dens_model_adapter.f95:45-46), i.e. PSI is the FIRST word of geopack's block -- and that word is ST0, the
    // sine of the dipole axis' colatitude (geopack2008.for:569), not RECALC_08's PSI (16th word).  The reference
    // therefore runs T04_s with PS = ST0 (~0.17 in 2010) whatever the date and hour; parity means doing the same.
    *psi = st0;
  }
  if (geopack_psi) { // geopack2008.for:1138-1142: PSI = ASIN(SPS), SPS = (DIP, EXGSW)
    const float sps = dip1 * x1 + dip2 * x2 + dip3 * x3;
    *geopack_psi = asinf(sps);
  }
  return true;
}

// ---------------------------------------------------------------------------------------------
ListReader::ListReader(const char *path) : f_(fopen(path, "r")), line_(1 << 16) {}
ListReader::~ListReader() {
  if (f_) fclose((FILE *)f_);
}
int64_t ListReader::read(int64_t n, double *out) {
  int64_t got = 0;
  FILE *f = (FILE *)f_;
  while (got < n) {
    if (!fgets(line_.data(), (int)line_.size(), f)) return got;
    char *s = line_.data();
    while (got < n) {
      while (*s == ' ' || *s == '\t' || *s == ',' || *s == '\r' || *s == '\n') ++s;
      if (!*s) break;
      char *e = s;
      // accept Fortran 'd' exponents
      char tok[64];
      int k = 0;
      while (*e && *e != ' ' && *e != '\t' && *e != ',' && *e != '\r' && *e != '\n' && k < 63) {
        char ch = *e++;
        tok[k++] = (ch == 'd' || ch == 'D') ? 'e' : ch;
      }
      tok[k] = 0;
      char *endp = nullptr;
      double v = strtod(tok, &endp);
      if (endp == tok) return got; // not a number
      out[got++] = v;
      s = e;
    }
  }
  return got;
}

bool read_newray(const char *path, NgoConfig &c, std::string &err) {
  ListReader r(path);
  if (!r.ok()) {
    err = "cannot open";
    return false;
  }
  double v[16];
  if (r.read(4, v) != 4) { err = "card 1 (intera numres nsuppr spelat) incomplete"; return false; }
  for (;;) { // satellite coordinates until distre <= -1 (:64-80)
    if (r.read(2, v) != 2) { err = "unterminated satellite-coordinate list"; return false; }
    c.last_latitu = v[1];
    if (v[0] <= -1.0) break;
  }
  if (r.read(10, v) != 10) { err = "model card (num kskip mode kount kducts ktape refalt dsrrng dsrlat dsdens) incomplete"; return false; }
  c.num = (int)v[0];
  c.kducts = (int)v[4];
  c.dsrrng = v[7]; c.dsrlat = v[8]; c.dsdens = v[9];
  if (c.num < 2 || c.num > 4) { err = "num must be 2..4"; return false; }
  if (c.kducts < 0 || c.kducts > 9) { err = "kducts must be 0..9"; return false; }
  if (r.read(5, v) != 5) { err = "card egfeq therm hm absb relb incomplete"; return false; }
  c.therm = v[1];
  if (r.read(5, v) != 5) { err = "card rbase ane0 alpha0(2:4) incomplete"; return false; }
  c.rbase = v[0]; c.ane0 = v[1]; c.alpha0[2] = v[2]; c.alpha0[3] = v[3]; c.alpha0[4] = v[4];
  if (r.read(5, v) != 5) { err = "card rzero scbot rstop rdiv hmin incomplete"; return false; }
  c.rzero = v[0]; c.scbot = v[1];
  if (c.kducts >= 1) {
    if (r.read(5, v) != 5) { err = "plasmapause card (lk expk ddk rconsn scr) incomplete"; return false; }
    c.lk = v[0]; c.expk = v[1]; c.ddk = v[2]; c.rconsn = v[3]; c.scr = v[4];
    for (int k = 2; k <= c.kducts; ++k) {
      if (r.read(12, v) != 12) { err = "duct card incomplete"; return false; }
      c.l0[k] = v[0]; c.def[k] = v[1]; c.dd[k] = v[2];
      c.rducln[k] = v[3]; c.hducln[k] = v[4]; c.rducun[k] = v[5]; c.hducun[k] = v[6];
      c.rducls[k] = v[7]; c.hducls[k] = v[8]; c.rducus[k] = v[9]; c.hducus[k] = v[10];
      c.sidedu[k] = v[11];
    }
  }
  return true;
}

static const char NSPEC_REFUSED[] = "nspec must be 1..4 (SRT_MAXSPEC: this library carries at most four species; see INTEGRATION.md section 1)";
// the shape a grid header announces, refused in the words of every grid reader
static bool grid_shape_ok(const GridFile &g, std::string &err) {
  if (g.nspec < 1 || g.nspec > 4) { err = NSPEC_REFUSED; return false; }
  if (g.nx < 2 || g.ny < 2 || g.nz < 2) { err = "grid needs >= 2 nodes per axis"; return false; }
  return true;
}

// --- the record-by-record reader (exactly the Fortran's READ semantics; slow: one strtod at a time)
static bool read_grid_file_records(const char *path, GridFile &g, std::string &err) {
  ListReader r(path);
  struct stat st;
  if (!r.ok() || stat(path, &st) != 0) { err = "cannot open"; return false; }
  double v[8];
  if (r.read(5, v) != 5) { err = "size header incomplete"; return false; }
  g.compder = (int)v[0]; g.nspec = (int)v[1]; g.nx = (int)v[2]; g.ny = (int)v[3]; g.nz = (int)v[4];
  if (!grid_shape_ok(g, err)) return false;
  if (r.read(6, g.bounds) != 6) { err = "bounds incomplete"; return false; }
  if (r.read(g.nspec, g.qs) != g.nspec) { err = "charges incomplete"; return false; }
  if (r.read(g.nspec, g.ms) != g.nspec) { err = "masses incomplete"; return false; }
  // a value takes two bytes of text at the least (a digit and its separator): a header that announces more values than the
  // file has room for is refused before anything of that size is allocated (in double: three int axes cannot overflow it)
  const double announced = (double)g.nx * g.ny * g.nz * g.nspec, room = (double)st.st_size / 2.0;
  if (announced > room) { err = "grid values truncated"; return false; }
  size_t nnode = (size_t)g.nx * g.ny * g.nz, n = nnode * g.nspec;
  g.F.resize(n);
  for (size_t c = 0; c < nnode; ++c) // one record per node (:100-106)
    if (r.read(g.nspec, g.F.data() + c * g.nspec) != g.nspec) { err = "grid values truncated"; return false; }
  g.have_derivs = (g.compder == 1);
  if (g.have_derivs) {
    if (8.0 * announced > room) { err = "derivative block truncated"; return false; }
    for (int a = 0; a < 7; ++a) {
      g.derivs[a].resize(n);
      if (r.read((int64_t)n, g.derivs[a].data()) != (int64_t)n) { err = "derivative block truncated"; return false; }
    }
  }
  return true;
}

// --- whole-file tokeniser, value block parsed by all host cores (a 256^3 x 4 grid is 67 M numbers, 1.7 GB of text)
namespace {
inline bool is_sep(char c) { return c == ' ' || c == '\t' || c == ',' || c == '\r' || c == '\n'; }
// parse every token of [b, e) as a double ('d' exponents accepted); false on a non-numeric token
bool parse_tokens(const char *b, const char *e, std::vector<double> &out) {
  char tok[72];
  while (b < e) {
    while (b < e && is_sep(*b)) ++b;
    if (b >= e) break;
    int k = 0;
    while (b < e && !is_sep(*b) && k < 70) {
      char ch = *b++;
      tok[k++] = (ch == 'd' || ch == 'D') ? 'e' : ch;
    }
    tok[k] = 0;
    char *endp = nullptr;
    double v = strtod(tok, &endp);
    if (endp == tok || *endp) return false;
    out.push_back(v);
  }
  return true;
}
struct MappedFile {
  const char *p = nullptr;
  size_t n = 0;
  int fd = -1;
  explicit MappedFile(const char *path) {
    fd = open(path, O_RDONLY);
    if (fd < 0) return;
    struct stat st;
    if (fstat(fd, &st) != 0 || st.st_size == 0) return;
    void *m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
    if (m == MAP_FAILED) return;
    p = (const char *)m;
    n = (size_t)st.st_size;
  }
  ~MappedFile() {
    if (p) munmap((void *)p, n);
    if (fd >= 0) close(fd);
  }
};
// every numeric token of [b, e), parsed by all host cores: the pieces hold them in order; false on a non-numeric token
bool parse_numbers(const char *b, const char *e, std::vector<std::vector<double>> &part) {
  unsigned nt = std::thread::hardware_concurrency();
  nt = nt ? (nt > 32 ? 32 : nt) : 1;
  if ((size_t)(e - b) < (size_t)nt * 4096) nt = 1;
  std::vector<const char *> cut(nt + 1); // cut at record boundaries, one piece per thread
  cut[0] = b;
  cut[nt] = e;
  for (unsigned t = 1; t < nt; ++t) {
    const char *c = b + (size_t)(e - b) * t / nt;
    const char *nl = (const char *)memchr(c, '\n', (size_t)(e - c));
    cut[t] = nl ? nl + 1 : e;
  }
  part.assign(nt, std::vector<double>());
  std::vector<char> good(nt, 1);
  std::vector<std::thread> th;
  for (unsigned t = 0; t < nt; ++t)
    th.emplace_back([&, t] {
      part[t].reserve((size_t)(cut[t + 1] - cut[t]) / 16 + 16);
      good[t] = parse_tokens(cut[t], cut[t + 1], part[t]) ? 1 : 0;
    });
  for (auto &x : th) x.join();
  for (unsigned t = 0; t < nt; ++t)
    if (!good[t]) return false;
  return true;
}
size_t count_numbers(const std::vector<std::vector<double>> &part) {
  size_t total = 0;
  for (const auto &p : part) total += p.size();
  return total;
}
// a binary side-format is known by the eight bytes it starts with
bool has_magic(const char *path, const char magic[8]) {
  FILE *f = fopen(path, "rb");
  if (!f) return false;
  char m[8];
  const bool ok = fread(m, 1, 8, f) == 8 && memcmp(m, magic, 8) == 0;
  fclose(f);
  return ok;
}
// a malloc'd array of n values for the caller (srt_free), a copy of src[n] where src is given; null: out of memory
template <class T> T *copy_out(size_t n, const T *src = nullptr) {
  T *p = (T *)malloc(sizeof(T) * (n ? n : 1));
  if (p && src && n) memcpy(p, src, sizeof(T) * n);
  return p;
}
const char GRID_MAGIC[8] = {'S', 'R', 'T', 'G', 'R', 'I', 'D', '1'};
struct GridBinHeader { // 8 + 5*4 + 4 (pad) + 14*8 = 144 bytes, then F, then 7 derivative blocks if compder == 1
  char magic[8];
  int32_t compder, nspec, nx, ny, nz, pad;
  double bounds[6], qs[4], ms[4];
};
} // namespace

static bool read_grid_binary(const char *path, GridFile &g, std::string &err) {
  MappedFile mf(path);
  if (!mf.p) { err = "cannot open"; return false; }
  if (mf.n < sizeof(GridBinHeader)) { err = "binary grid: header truncated"; return false; }
  GridBinHeader h;
  memcpy(&h, mf.p, sizeof h);
  g.compder = h.compder; g.nspec = h.nspec; g.nx = h.nx; g.ny = h.ny; g.nz = h.nz;
  if (!grid_shape_ok(g, err)) return false;
  memcpy(g.bounds, h.bounds, sizeof g.bounds);
  memcpy(g.qs, h.qs, sizeof g.qs);
  memcpy(g.ms, h.ms, sizeof g.ms);
  size_t n = (size_t)g.nx * g.ny * g.nz * g.nspec;
  g.have_derivs = (g.compder == 1);
  size_t need = sizeof h + n * sizeof(double) * (g.have_derivs ? 8 : 1);
  if (mf.n < need) { err = "binary grid: value block truncated"; return false; }
  const char *q = mf.p + sizeof h;
  g.F.resize(n);
  memcpy(g.F.data(), q, n * sizeof(double));
  if (g.have_derivs)
    for (int a = 0; a < 7; ++a) {
      g.derivs[a].resize(n);
      memcpy(g.derivs[a].data(), q + (size_t)(a + 1) * n * sizeof(double), n * sizeof(double));
    }
  return true;
}

// binary side-format: the 144-byte header followed by the value blocks of the text format as raw little-endian doubles in
// the same order
static bool write_grid_binary(const char *path, const GridFile &g, std::string &err) {
  FILE *f = fopen(path, "wb");
  if (!f) { err = "cannot open for writing"; return false; }
  GridBinHeader h;
  memset(&h, 0, sizeof h);
  memcpy(h.magic, GRID_MAGIC, 8);
  h.compder = g.have_derivs ? 1 : 0; h.nspec = g.nspec; h.nx = g.nx; h.ny = g.ny; h.nz = g.nz;
  memcpy(h.bounds, g.bounds, sizeof h.bounds);
  memcpy(h.qs, g.qs, sizeof h.qs);
  memcpy(h.ms, g.ms, sizeof h.ms);
  bool ok = fwrite(&h, sizeof h, 1, f) == 1 && fwrite(g.F.data(), sizeof(double), g.F.size(), f) == g.F.size();
  if (g.have_derivs)
    for (int a = 0; a < 7 && ok; ++a) ok = fwrite(g.derivs[a].data(), sizeof(double), g.derivs[a].size(), f) == g.derivs[a].size();
  ok = (fclose(f) == 0) && ok;
  if (!ok) err = "write failed";
  return ok;
}

// every numeric token of a text file, in order, parsed by all host cores; false if the file cannot be opened or holds
// a non-numeric token
static bool read_all_numbers(const char *path, std::vector<double> &all, std::string &err) {
  MappedFile mf(path);
  if (!mf.p) { err = "cannot open"; return false; }
  std::vector<std::vector<double>> part;
  if (!parse_numbers(mf.p, mf.p + mf.n, part)) { err = "non-numeric token"; return false; }
  all.clear();
  all.reserve(count_numbers(part));
  for (const auto &p : part) all.insert(all.end(), p.begin(), p.end());
  return true;
}

bool read_grid_file(const char *path, GridFile &g, std::string &err) {
  if (has_magic(path, GRID_MAGIC)) return read_grid_binary(path, g, err);
  MappedFile mf(path);
  if (!mf.p) { err = "cannot open"; return false; }
  // header: the first four records (sizes; bounds; charges; masses)
  const char *b = mf.p, *e = mf.p + mf.n;
  std::vector<double> hv;
  auto record = [&](int want) -> bool { // one READ: starts on a new record, may continue over following ones
    size_t got0 = hv.size();
    while ((int)(hv.size() - got0) < want && b < e) {
      const char *nl = (const char *)memchr(b, '\n', (size_t)(e - b));
      const char *le = nl ? nl : e;
      std::vector<double> t;
      if (!parse_tokens(b, le, t)) return false;
      for (double v : t)
        if ((int)(hv.size() - got0) < want) hv.push_back(v);
      b = nl ? nl + 1 : e;
    }
    return (int)(hv.size() - got0) == want;
  };
  if (!record(5)) { err = "size header incomplete"; return false; }
  g.compder = (int)hv[0]; g.nspec = (int)hv[1]; g.nx = (int)hv[2]; g.ny = (int)hv[3]; g.nz = (int)hv[4];
  if (!grid_shape_ok(g, err)) return false;
  if (!record(6)) { err = "bounds incomplete"; return false; }
  if (!record(g.nspec)) { err = "charges incomplete"; return false; }
  if (!record(g.nspec)) { err = "masses incomplete"; return false; }
  for (int k = 0; k < 6; ++k) g.bounds[k] = hv[5 + k];
  for (int k = 0; k < g.nspec; ++k) { g.qs[k] = hv[11 + k]; g.ms[k] = hv[11 + g.nspec + k]; }
  const size_t nnode = (size_t)g.nx * g.ny * g.nz, n = nnode * g.nspec;
  g.have_derivs = (g.compder == 1);
  // the value block; the count is compared in double, which the product of three int axes cannot overflow
  std::vector<std::vector<double>> part;
  if (!parse_numbers(b, e, part) || (double)count_numbers(part) != (double)g.nx * g.ny * g.nz * g.nspec * (g.have_derivs ? 8 : 1)) {
    // not the plain one-record-per-node layout (extra fields on a line, a stray token, ...): re-read with the
    // Fortran's record semantics
    g = GridFile();
    return read_grid_file_records(path, g, err);
  }
  g.F.resize(n);
  if (g.have_derivs)
    for (int a = 0; a < 7; ++a) g.derivs[a].resize(n);
  size_t pos = 0; // the pieces, end to end, are F and then the seven derivative blocks
  for (auto &p : part) {
    for (size_t i = 0; i < p.size();) {
      const size_t blk = pos / n, off = pos % n, m = std::min(p.size() - i, n - off);
      memcpy((blk == 0 ? g.F : g.derivs[blk - 1]).data() + off, p.data() + i, m * sizeof(double));
      i += m;
      pos += m;
    }
    std::vector<double>().swap(p);
  }
  return true;
}

// ---------------------------------------------------------------------------------------------
// the es24.15e3 edit descriptor into exactly 24 characters (no terminator), the exponent widened to three digits by hand;
// NaN, Inf and -Inf right-aligned as the Fortran writes them
static void put_es24(double v, char *out) {
  char tmp[40];
  if (!std::isfinite(v)) {
    const char *s = std::isnan(v) ? "NaN" : v > 0 ? "Inf" : "-Inf";
    const size_t n = strlen(s);
    memset(out, ' ', 24 - n);
    memcpy(out + 24 - n, s, n);
    return;
  }
  // [-]d.ddddddddddddddde+XX[X]: std::to_chars with a precision is correctly rounded like printf's %.15E (and 5x faster)
  const std::to_chars_result tr = std::to_chars(tmp, tmp + sizeof tmp - 1, v, std::chars_format::scientific, 15);
  const int n = (int)(tr.ptr - tmp);
  tmp[n] = 0;
  const char *e = (const char *)memchr(tmp, 'e', (size_t)n);
  const int mant = (int)(e - tmp);
  int ex = atoi(e + 2);
  const int len = mant + 5;
  char *q = out;
  for (int k = len; k < 24; ++k) *q++ = ' ';
  memcpy(q, tmp, (size_t)mant);
  q += mant;
  *q++ = 'E';
  *q++ = e[1];
  *q++ = (char)('0' + (ex / 100) % 10);
  *q++ = (char)('0' + (ex / 10) % 10);
  *q++ = (char)('0' + ex % 10);
}

// A text file of Fortran-formatted records being written.  It owns the FILE and its 4 MB buffer; a record is put together
// field by field and goes out at end(); what went wrong, at the opening or at any write, is said once, by close().
namespace {
class TextWriter {
public:
  explicit TextWriter(const char *path) : path_(path), f_(fopen(path, "w")), buf_(f_ ? (size_t)1 << 22 : 0) {
    if (f_) setvbuf(f_, buf_.data(), _IOFBF, buf_.size());
  }
  ~TextWriter() {
    if (f_) fclose(f_);
  }
  TextWriter(const TextWriter &) = delete;
  TextWriter &operator=(const TextWriter &) = delete;
  bool ok() const { return f_ != nullptr; }
  TextWriter &i10(long long v) { return integer("%10lld", v); }
  TextWriter &i20(long long v) { return integer("%20lld", v); }
  TextWriter &es24(double v) {
    rec_.resize(rec_.size() + 24);
    put_es24(v, &rec_[rec_.size() - 24]);
    return *this;
  }
  TextWriter &es24(const double *v, size_t n) {
    for (size_t k = 0; k < n; ++k) es24(v[k]);
    return *this;
  }
  void end() {
    rec_ += '\n';
    if (f_) fwrite(rec_.data(), 1, rec_.size(), f_);
    rec_.clear();
  }
  int close() { // SRT_OK, or SRT_EIO and its text
    if (!f_) return srt_set_error(SRT_EIO, "%s: cannot open for writing", path_);
    const bool failed = ferror(f_) != 0;
    const bool closed = fclose(f_) == 0;
    f_ = nullptr;
    return failed || !closed ? srt_set_error(SRT_EIO, "%s: write failed", path_) : SRT_OK;
  }

private:
  TextWriter &integer(const char *fmt, long long v) {
    char b[24];
    rec_.append(b, (size_t)snprintf(b, sizeof b, fmt, v));
    return *this;
  }
  const char *path_;
  FILE *f_;
  std::vector<char> buf_;
  std::string rec_;
};
// one text file: opened, written by body(TextWriter &) if it could be opened, closed -> SRT_OK, or SRT_EIO and its text
template <class Body> int write_text(const char *path, Body body) {
  TextWriter t(path);
  if (t.ok()) body(t);
  return t.close();
}

// an i10 field holds a ray number of at most ten digits: beyond, Fortran prints asterisks, and a fixed-length record could not
// hold the number -- every writer refuses rather than shifts or truncates
bool fits_i10(long long first, long long last) { return first >= 0 && last <= 9999999999ll; }
int refuse_beyond_i10(const char *who, const char *what, int64_t n, const int64_t *raynum) {
  for (int64_t k = 0; k < n; ++k)
    if (!fits_i10(raynum[k], raynum[k]))
      return srt_set_error(SRT_EINVAL, "%s: ray number %lld of %s %lld does not fit the record's i10 field", who, (long long)raynum[k], what,
                           (long long)k);
  return SRT_OK;
}
// the offsets of a packed row set start at 0 and do not decrease; `who` is "" or the caller's name and ": "
int refuse_bad_offsets(const char *who, int64_t nrays, const int64_t *offsets) {
  if (offsets[0] != 0) return srt_set_error(SRT_EINVAL, "%soffsets[0] = %lld: the first ray's rows start at 0", who, (long long)offsets[0]);
  for (int64_t r = 0; r < nrays; ++r)
    if (offsets[r + 1] < offsets[r]) return srt_set_error(SRT_EINVAL, "%soffsets decrease at ray %lld", who, (long long)r);
  return SRT_OK;
}
} // namespace

// ---- model-4 sample files: the reference builder's text (gcpm_dens_model_buildgrid_random.f95:196-208 for the
// header, helpermod :37-43 for one sample per record, es24.15e3) and the binary side-format "SRTPTS01": int32 nspec, int32 0,
// int64 npts, bounds[6], qs[4], ms[4] (a 136-byte header), then npts records of 3 + nspec little-endian doubles ----
namespace {
const char PTS_MAGIC[8] = {'S', 'R', 'T', 'P', 'T', 'S', '0', '1'};
struct PtsHeader {
  char magic[8];
  int32_t nspec, zero;
  int64_t npts;
  double bounds[6], qs[4], ms[4];
};
// a text sample file taken as one run of numbers -- nspec, 6 bounds, nspec charges, nspec masses, then 3 + nspec per sample --
// which it is when every record holds exactly what its READ takes
struct PointsText {
  int nspec = 0;
  int64_t npts = 0;
  const double *bounds = nullptr, *qs = nullptr, *ms = nullptr, *rec = nullptr;
};
bool split_points_text(const std::vector<double> &all, PointsText &p) {
  if (all.size() < 7) return false;
  p.nspec = (int)all[0];
  if (p.nspec < 1 || p.nspec > 4 || all.size() < (size_t)(7 + 2 * p.nspec) || (all.size() - 7 - 2 * p.nspec) % (size_t)(3 + p.nspec) != 0)
    return false;
  p.npts = (int64_t)((all.size() - 7 - 2 * p.nspec) / (size_t)(3 + p.nspec));
  p.bounds = &all[1];
  p.qs = &all[7];
  p.ms = p.qs + p.nspec;
  p.rec = p.ms + p.nspec;
  return true;
}
bool read_points_binary(const char *path, int &nspec, double qs[4], double ms[4], std::vector<double> &rec, std::string &err) {
  MappedFile mf(path);
  if (!mf.p) { err = "cannot open"; return false; }
  err = "truncated or malformed binary sample file";
  PtsHeader h;
  if (mf.n < sizeof h) return false;
  memcpy(&h, mf.p, sizeof h);
  if (memcmp(h.magic, PTS_MAGIC, 8) != 0 || h.nspec < 1 || h.nspec > 4 || h.npts < 0) return false;
  // the records the file has room for against the count its header announces: a division, which cannot overflow
  const size_t w = (size_t)(3 + h.nspec);
  if ((mf.n - sizeof h) / (w * sizeof(double)) < (uint64_t)h.npts) return false;
  nspec = h.nspec;
  for (int k = 0; k < nspec; ++k) { qs[k] = h.qs[k]; ms[k] = h.ms[k]; }
  rec.resize((size_t)h.npts * w);
  if (!rec.empty()) memcpy(rec.data(), mf.p + sizeof h, rec.size() * sizeof(double));
  err.clear();
  return true;
}
int write_points_file(const char *path, bool binary, int nspec, int64_t npts, const double bounds[6], const double *qs, const double *ms,
                      const double *rec) {
  const size_t w = (size_t)(3 + nspec);
  if (binary) {
    FILE *f = fopen(path, "wb");
    if (!f) return srt_set_error(SRT_EIO, "%s: cannot open for writing", path);
    PtsHeader h;
    memset(&h, 0, sizeof h);
    memcpy(h.magic, PTS_MAGIC, 8);
    h.nspec = nspec;
    h.npts = npts;
    for (int k = 0; k < 6; ++k) h.bounds[k] = bounds[k];
    for (int k = 0; k < nspec; ++k) { h.qs[k] = qs[k]; h.ms[k] = ms[k]; }
    bool ok = fwrite(&h, sizeof h, 1, f) == 1 && fwrite(rec, sizeof(double), (size_t)npts * w, f) == (size_t)npts * w;
    ok = (fclose(f) == 0) && ok;
    return ok ? SRT_OK : srt_set_error(SRT_EIO, "%s: write failed", path);
  }
  return write_text(path, [&](TextWriter &t) {
    t.i10(nspec).end();
    t.es24(bounds, 6).end();
    t.es24(qs, (size_t)nspec).end();
    t.es24(ms, (size_t)nspec).end();
    for (int64_t i = 0; i < npts; ++i) t.es24(rec + (size_t)i * w, w).end();
  });
}
} // namespace

bool read_points_file(const char *path, int &nspec, double qs[4], double ms[4], std::vector<double> &rec, std::string &err) {
  if (has_magic(path, PTS_MAGIC)) return read_points_binary(path, nspec, qs, ms, rec, err);
  // fast path: the whole file tokenised by all cores
  std::vector<double> all;
  std::string unused;
  PointsText p;
  if (read_all_numbers(path, all, unused) && split_points_text(all, p)) {
    nspec = p.nspec;
    for (int k = 0; k < nspec; ++k) { qs[k] = p.qs[k]; ms[k] = p.ms[k]; }
    rec.assign(p.rec, p.rec + (size_t)p.npts * (size_t)(3 + nspec));
    return true;
  }
  // the Fortran's record semantics, one READ at a time
  ListReader r(path);
  if (!r.ok()) {
    err = "cannot open";
    return false;
  }
  double hdr[7];
  if (r.read(7, hdr) != 7) { err = "header (nspec + bounds) incomplete"; return false; }
  nspec = (int)hdr[0];
  if (nspec < 1 || nspec > 4) { err = NSPEC_REFUSED; return false; }
  if (r.read(nspec, qs) != nspec || r.read(nspec, ms) != nspec) { err = "charges/masses incomplete"; return false; }
  double row[8];
  while (r.read(3 + nspec, row) == 3 + nspec) rec.insert(rec.end(), row, row + 3 + nspec);
  return true;
}

} // namespace srt_host

// ================================================================================ C ABI (file I/O)
using srt_host::copy_out;
using srt_host::put_es24;
using srt_host::TextWriter;

extern "C" void srt_free(void *p) { free(p); }

// ---- model-3 grid files: text of gcpm_dens_model_buildgrid.f95:302-327 <-> binary side-format
extern "C" int srt_grid_file_read(const char *path, int32_t dims[5], double bounds[6], double qs[4], double ms[4],
                                  double **F, double **derivs) {
  if (!path || !dims || !bounds || !qs || !ms || !F) return srt_set_error(SRT_EINVAL, "null argument");
  srt_host::GridFile g;
  std::string err;
  if (!srt_host::read_grid_file(path, g, err)) return srt_set_error(SRT_EIO, "%s: %s", path, err.c_str());
  dims[0] = g.have_derivs ? 1 : 0; dims[1] = g.nspec; dims[2] = g.nx; dims[3] = g.ny; dims[4] = g.nz;
  memcpy(bounds, g.bounds, 6 * sizeof(double));
  memcpy(qs, g.qs, 4 * sizeof(double));
  memcpy(ms, g.ms, 4 * sizeof(double));
  const size_t n = g.F.size();
  *F = copy_out(n, g.F.data());
  if (!*F) return srt_set_error(SRT_ENOMEM, "grid of %zu values", n);
  if (derivs) {
    *derivs = nullptr;
    if (g.have_derivs) {
      *derivs = copy_out<double>(7 * n);
      if (!*derivs) return srt_set_error(SRT_ENOMEM, "derivative blocks of %zu values", 7 * n);
      for (int a = 0; a < 7; ++a) memcpy(*derivs + (size_t)a * n, g.derivs[a].data(), n * sizeof(double));
    }
  }
  return SRT_OK;
}

extern "C" int srt_grid_file_write(const char *path, int binary, int nspec, int nx, int ny, int nz,
                                   const double bounds[6], const double *qs, const double *ms, const double *F,
                                   const double *derivs) {
  if (!path || !bounds || !qs || !ms || !F) return srt_set_error(SRT_EINVAL, "null argument");
  if (nspec < 1 || nspec > SRT_MAXSPEC || nx < 2 || ny < 2 || nz < 2) return srt_set_error(SRT_EINVAL, "bad grid shape");
  const size_t n = (size_t)nx * ny * nz * nspec;
  if (binary) {
    srt_host::GridFile g;
    g.nspec = nspec; g.nx = nx; g.ny = ny; g.nz = nz;
    g.have_derivs = derivs != nullptr;
    memcpy(g.bounds, bounds, sizeof g.bounds);
    for (int k = 0; k < nspec; ++k) { g.qs[k] = qs[k]; g.ms[k] = ms[k]; }
    g.F.assign(F, F + n);
    if (derivs)
      for (int a = 0; a < 7; ++a) g.derivs[a].assign(derivs + (size_t)a * n, derivs + (size_t)(a + 1) * n);
    std::string err;
    if (!srt_host::write_grid_binary(path, g, err)) return srt_set_error(SRT_EIO, "%s: %s", path, err.c_str());
    return SRT_OK;
  }
  // text, byte for byte what gcpm_dens_model_buildgrid.f95:302-327 writes: (5i10); (6es24.15e3); charges; masses;
  // then every value on its own record in es24.15e3 (16 significant digits -- the format's, not ours: use the
  // binary form where the last bit matters)
  return srt_host::write_text(path, [&](TextWriter &t) {
    t.i10(derivs ? 1 : 0).i10(nspec).i10(nx).i10(ny).i10(nz).end();
    t.es24(bounds, 6).end();
    t.es24(qs, (size_t)nspec).end();
    t.es24(ms, (size_t)nspec).end();
    for (size_t c = 0; c < n; ++c) t.es24(F[c]).end();
    for (size_t c = 0; derivs && c < 7 * n; ++c) t.es24(derivs[c]).end();
  });
}

extern "C" int srt_grid_file_convert(const char *in, const char *out_binary) {
  if (!in || !out_binary) return srt_set_error(SRT_EINVAL, "null argument");
  srt_host::GridFile g;
  std::string err;
  if (!srt_host::read_grid_file(in, g, err)) return srt_set_error(SRT_EIO, "%s: %s", in, err.c_str());
  if (!srt_host::write_grid_binary(out_binary, g, err)) return srt_set_error(SRT_EIO, "%s: %s", out_binary, err.c_str());
  return SRT_OK;
}

extern "C" int srt_grid_file_is_binary(const char *path) { return path && srt_host::has_magic(path, srt_host::GRID_MAGIC) ? 1 : 0; }

extern "C" int64_t srt_read_rays_file(const char *path, double **pos0, double **dir0, double **w0) {
  if (!path || !pos0 || !dir0 || !w0) return srt_set_error(SRT_EINVAL, "null argument");
  srt_host::ListReader r(path);
  if (!r.ok()) return srt_set_error(SRT_EIO, "%s: cannot open", path);
  std::vector<double> all;
  double v[7];
  while (r.read(7, v) == 7) all.insert(all.end(), v, v + 7); // read(infile,*) pos0, dir0, w ; EOF ends (driver:1146)
  int64_t n = (int64_t)(all.size() / 7);
  *pos0 = copy_out<double>(3 * (size_t)n);
  *dir0 = copy_out<double>(3 * (size_t)n);
  *w0 = copy_out<double>((size_t)n);
  if (!*pos0 || !*dir0 || !*w0) {
    free(*pos0), free(*dir0), free(*w0);
    *pos0 = *dir0 = *w0 = nullptr;
    return srt_set_error(SRT_ENOMEM, "%s: %lld rays", path, (long long)n);
  }
  for (int64_t i = 0; i < n; ++i) {
    for (int c = 0; c < 3; ++c) {
      (*pos0)[3 * i + c] = all[7 * i + c];
      (*dir0)[3 * i + c] = all[7 * i + 3 + c];
    }
    (*w0)[i] = all[7 * i + 6];
  }
  return n;
}

// .ray reader: the inverse of srt_write_ray_file (what matlab/readrayoutput.m does for the damping scripts).  Every record
// is a run of blank-separated numbers -- 2 + 17 + 1 + 4 nspec of them -- so the whole file is parsed as one token stream by
// all host cores and cut into records; the records of a ray are consecutive.
extern "C" int64_t srt_read_ray_file(const char *path, int32_t *nspec_out, double qs[4], double ms[4], int64_t *nrecords,
                                     int64_t **raynum, int32_t **stopcond, int32_t **kept, double **w0, double **rows) {
  if (!path || !nspec_out || !qs || !ms || !nrecords || !raynum || !stopcond || !kept || !w0 || !rows)
    return srt_set_error(SRT_EINVAL, "null argument");
  *nspec_out = 0;
  *nrecords = 0;
  *raynum = nullptr, *stopcond = nullptr, *kept = nullptr, *w0 = nullptr, *rows = nullptr;
  struct stat st;
  if (stat(path, &st) != 0) return srt_set_error(SRT_EIO, "%s: cannot open", path);
  std::vector<double> all;
  std::string err;
  if (st.st_size > 0 && !srt_host::read_all_numbers(path, all, err)) return srt_set_error(SRT_EIO, "%s: %s", path, err.c_str());
  int64_t nrec = 0, nray = 0;
  int nspec = 0;
  if (!all.empty()) {
    if (all.size() < 20) return srt_set_error(SRT_EIO, "%s: truncated record", path);
    nspec = (int)all[19];
    if (nspec < 1 || nspec > SRT_MAXSPEC || (double)nspec != all[19]) return srt_set_error(SRT_EIO, "%s: nspec = %g in the first record", path, all[19]);
    const size_t per = 20 + (size_t)4 * nspec;
    if (all.size() % per) return srt_set_error(SRT_EIO, "%s: %zu numbers are not a whole number of %zu-number records", path, all.size(), per);
    nrec = (int64_t)(all.size() / per);
    for (int64_t r = 0; r < nrec; ++r) {
      const double *v = all.data() + (size_t)r * per;
      if ((int)v[19] != nspec) return srt_set_error(SRT_EIO, "%s: record %lld has nspec %g", path, (long long)r + 1, v[19]);
      if (r == 0 || v[0] != all[(size_t)(r - 1) * per] || v[2] == 0.0) ++nray; // (a ray's first record is its row 0: t = 0)
    }
  }
  *raynum = copy_out<int64_t>((size_t)nray);
  *stopcond = copy_out<int32_t>((size_t)nray);
  *kept = copy_out<int32_t>((size_t)nray);
  *w0 = copy_out<double>((size_t)nray);
  *rows = copy_out<double>((size_t)SRT_ROW * (size_t)nrec);
  if (!*raynum || !*stopcond || !*kept || !*w0 || !*rows) {
    free(*raynum), free(*stopcond), free(*kept), free(*w0), free(*rows);
    *raynum = nullptr, *stopcond = nullptr, *kept = nullptr, *w0 = nullptr, *rows = nullptr;
    return srt_set_error(SRT_ENOMEM, "%s: %lld records", path, (long long)nrec);
  }
  for (int s = 0; s < 4; ++s) qs[s] = ms[s] = 0.0;
  const size_t per = 20 + (size_t)4 * (nspec ? nspec : 1);
  int64_t ray = -1;
  for (int64_t r = 0; r < nrec; ++r) {
    const double *v = all.data() + (size_t)r * per;
    if (r == 0 || v[0] != all[(size_t)(r - 1) * per] || v[2] == 0.0) { // (so files appended to, which repeat ray numbers, keep their rays apart)
      ++ray;
      (*raynum)[ray] = (int64_t)v[0];
      (*stopcond)[ray] = (int32_t)v[1];
      (*kept)[ray] = 0;
      (*w0)[ray] = v[18];
    }
    (*kept)[ray] += 1;
    double *row = *rows + (size_t)r * SRT_ROW;
    for (int c = 0; c < 16; ++c) row[c] = v[2 + c]; // t, pos, vprel, vgrel, n, B0
    for (int k = 0; k < 4; ++k) row[16 + k] = k < nspec ? v[20 + 2 * nspec + k] : 0.0; // Ns
    if (r == 0)
      for (int k = 0; k < nspec; ++k) {
        qs[k] = v[20 + k];
        ms[k] = v[20 + nspec + k];
      }
  }
  *nspec_out = nspec;
  *nrecords = nrec;
  return nray;
}

// record format of raytracer_driver.f95:1197-1217:
//   (i10, i10, 17es24.15e3, i10) raynum, stopcond, t, pos, vprel, vgrel, n, B0, w, nspec
//   then nspec x es24.15e3 for each of qs, ms, Ns, nus
// Records are fixed-length (raytracer_driver.f95:1197-1217: i10, i10, 17 es24.15e3, i10, 4 nspec es24.15e3, newline), so a
// ray's file offset is known from the kept-row counts before it: all host cores format disjoint ray ranges and pwrite them
// in place (SRT_IO_THREADS=1: one thread).  At BASELINE config[2] (1 M rays, 13 kept rows each) the file is 10.7 GB of text.
// The one formatting routine of both writers: prefix[r] = records before ray r (prefix[nrays] = all of them), and record s
// of ray r is the row at rows + (r * stride + prefix[r] * packed + s) * SRT_ROW -- stride = slots, packed = 0 for the padded
// layout [nrays][slots][SRT_ROW]; stride = 0, packed = 1 for rows that lie back to back.
static int write_ray_records(const char *path, int append, int64_t raynum0, int64_t nrays, int nspec, const double *qs,
                             const double *ms, const double *w0, const double *rows, const int32_t *stopcond,
                             const std::vector<int64_t> &prefix, size_t stride, size_t packed) {
  if (nspec < 1 || nspec > SRT_MAXSPEC) return srt_set_error(SRT_EINVAL, "nspec out of range");
  // the record's ray number is an i10 field (raytracer_driver.f95:1197)
  if (nrays < 0 || !srt_host::fits_i10(raynum0, raynum0 + nrays - 1))
    return srt_set_error(SRT_EINVAL, "ray numbers %lld .. %lld do not fit the record's i10 field", (long long)raynum0, (long long)(raynum0 + nrays - 1));
  const size_t L = 20 + 17 * 24 + 10 + (size_t)4 * nspec * 24 + 1;
  const int fd = open(path, O_WRONLY | O_CREAT | (append ? 0 : O_TRUNC), 0644);
  if (fd < 0) return srt_set_error(SRT_EIO, "%s: cannot open for writing", path);
  off_t base = 0;
  if (append) {
    struct stat st;
    if (fstat(fd, &st) == 0) base = st.st_size;
  }
  int nth = (int)std::thread::hardware_concurrency();
  if (const char *e = getenv("SRT_IO_THREADS")) nth = atoi(e);
  if (nth < 1) nth = 1;
  if (nth > 64) nth = 64;
  if ((int64_t)nth > nrays) nth = nrays > 0 ? (int)nrays : 1;
  // contiguous ray ranges, one per thread
  std::vector<int64_t> first(nth + 1);
  for (int t = 0; t <= nth; ++t) first[t] = (nrays * t) / nth;
  std::vector<char> consts((size_t)8 * 24); // qs and ms of the record, formatted once
  for (int s = 0; s < nspec; ++s) {
    put_es24(qs[s], consts.data() + 24 * s);
    put_es24(ms[s], consts.data() + 24 * (nspec + s));
  }
  char zero[24];
  put_es24(0.0, zero);
  std::vector<int> fail(nth, 0);
  auto work = [&](int t) {
    const size_t CH = (size_t)1 << 22;
    std::vector<char> buf(CH + L);
    size_t fill = 0;
    off_t off = base + (off_t)((size_t)prefix[first[t]] * L);
    auto flush = [&]() {
      size_t done = 0;
      while (done < fill) {
        ssize_t w = pwrite(fd, buf.data() + done, fill - done, off + (off_t)done);
        if (w < 0 && errno == EINTR) continue; // interrupted before anything was written: again
        if (w <= 0) {
          fail[t] = 1;
          return;
        }
        done += (size_t)w;
      }
      off += (off_t)fill;
      fill = 0;
    };
    for (int64_t r = first[t]; r < first[t + 1] && !fail[t]; ++r) {
      const int64_t kept = prefix[r + 1] - prefix[r];
      char head[24], wbuf[24];
      snprintf(head, sizeof head, "%10lld%10d", (long long)(raynum0 + r), (int)stopcond[r]);
      put_es24(w0[r], wbuf);
      for (int64_t s = 0; s < kept; ++s) {
        const double *row = rows + ((size_t)r * stride + (size_t)prefix[r] * packed + (size_t)s) * SRT_ROW;
        char *q = buf.data() + fill;
        memcpy(q, head, 20);
        q += 20;
        for (int c = 0; c < 16; ++c, q += 24) put_es24(row[c], q);
        memcpy(q, wbuf, 24);
        q += 24;
        char ns[12];
        snprintf(ns, sizeof ns, "%10d", nspec);
        memcpy(q, ns, 10);
        q += 10;
        memcpy(q, consts.data(), (size_t)2 * nspec * 24);
        q += (size_t)2 * nspec * 24;
        for (int k = 0; k < nspec; ++k, q += 24) put_es24(row[16 + k], q);
        for (int k = 0; k < nspec; ++k, q += 24) memcpy(q, zero, 24);
        *q++ = '\n';
        fill += L;
        if (fill >= CH) flush();
      }
    }
    if (fill && !fail[t]) flush();
  };
  if (nth == 1) work(0);
  else {
    std::vector<std::thread> th;
    for (int t = 0; t < nth; ++t) th.emplace_back(work, t);
    for (auto &x : th) x.join();
  }
  const int rc = close(fd);
  for (int t = 0; t < nth; ++t)
    if (fail[t]) return srt_set_error(SRT_EIO, "%s: write failed", path);
  if (rc != 0) return srt_set_error(SRT_EIO, "%s: close failed", path);
  return SRT_OK;
}

extern "C" int srt_write_ray_file(const char *path, int append, int64_t raynum0, int64_t nrays, const srt_params *p,
                                  int nspec, const double *qs, const double *ms, const double *w0,
                                  const double *rows, const int32_t *nrows, const int32_t *stopcond) {
  if (!path || !p || !qs || !ms || !w0 || !rows || !nrows || !stopcond) return srt_set_error(SRT_EINVAL, "null argument");
  const int slots = srt_rows_per_ray(p);
  const int per = p->outputper < 1 ? 1 : p->outputper;
  std::vector<int64_t> prefix(nrays > 0 ? (size_t)nrays + 1 : 1, 0); // (nrays < 0 is refused by the shared routine)
  for (int64_t r = 0; r < nrays; ++r) {
    const int k = (nrows[r] + per - 1) / per;
    prefix[r + 1] = prefix[r] + (k > slots ? slots : (k < 0 ? 0 : k));
  }
  return write_ray_records(path, append, raynum0, nrays, nspec, qs, ms, w0, rows, stopcond, prefix, (size_t)slots, 0);
}

// the same file from the packed layout srt_read_ray_file returns: offsets[nrays + 1], rows[offsets[nrays]][SRT_ROW]
extern "C" int srt_write_ray_file_packed(const char *path, int append, int64_t raynum0, int64_t nrays, int nspec, const double *qs,
                                         const double *ms, const double *w0, const int64_t *offsets, const double *rows,
                                         const int32_t *stopcond) {
  if (!path || !qs || !ms || !offsets || nrays < 0 || (nrays > 0 && (!w0 || !stopcond))) return srt_set_error(SRT_EINVAL, "null argument");
  if (const int rc = srt_host::refuse_bad_offsets("", nrays, offsets)) return rc;
  if (offsets[nrays] > 0 && !rows) return srt_set_error(SRT_EINVAL, "null argument");
  const std::vector<int64_t> prefix(offsets, offsets + nrays + 1);
  return write_ray_records(path, append, raynum0, nrays, nspec, qs, ms, w0, rows, stopcond, prefix, 0, 1);
}

// ---- event files: one record per event, (4 i10, then es24.15e3 fields): raynum, index + 1, interval + 1, meta[3], [distance,] the row ----
static int write_event_records(const char *who, const char *path, int64_t nevents, const int64_t *raynum, const int32_t *event_meta,
                               const double *event_dist, const double *event_rows) {
  if (const int rc = srt_host::refuse_beyond_i10(who, "event", nevents, raynum)) return rc;
  return srt_host::write_text(path, [&](TextWriter &t) {
    for (int64_t e = 0; e < nevents; ++e) {
      const int32_t *m = event_meta + 4 * e;
      t.i10(raynum[e]).i10((long long)m[1] + 1).i10((long long)m[2] + 1).i10(m[3]);
      if (event_dist) t.es24(event_dist[e]);
      t.es24(event_rows + (size_t)e * SRT_ROW, SRT_ROW).end();
    }
  });
}

// crossings file: (4 i10, 20 es24.15e3): raynum, surface + 1, interval + 1, direction, the row
extern "C" int srt_crossings_file_write(const char *path, int64_t nevents, const int64_t *raynum, const int32_t *event_meta,
                                        const double *event_rows) {
  if (!path || nevents < 0 || (nevents > 0 && (!raynum || !event_meta || !event_rows)))
    return srt_set_error(SRT_EINVAL, "srt_crossings_file_write: null argument");
  return write_event_records("srt_crossings_file_write", path, nevents, raynum, event_meta, nullptr, event_rows);
}

// approaches file: (4 i10, 21 es24.15e3): raynum, observer + 1, interval + 1, 0, distance, the row
extern "C" int srt_approaches_file_write(const char *path, int64_t nevents, const int64_t *raynum, const int32_t *event_meta,
                                         const double *event_dist, const double *event_rows) {
  if (!path || nevents < 0 || (nevents > 0 && (!raynum || !event_meta || !event_dist || !event_rows)))
    return srt_set_error(SRT_EINVAL, "srt_approaches_file_write: null argument");
  return write_event_records("srt_approaches_file_write", path, nevents, raynum, event_meta, event_dist, event_rows);
}

// tubes file: one record per packed row whose flag is not 1, (3 i10, 5 es24.15e3): raynum, row + 1 (among the ray's kept rows),
// flag, t, the section
extern "C" int srt_tubes_file_write(const char *path, int64_t nrays, const int64_t *raynum, const int64_t *offsets, const double *rows,
                                    const double *section, const int32_t *flag) {
  if (!path || nrays < 0 || !offsets || (nrays > 0 && !raynum)) return srt_set_error(SRT_EINVAL, "srt_tubes_file_write: null argument");
  if (const int rc = srt_host::refuse_bad_offsets("srt_tubes_file_write: ", nrays, offsets)) return rc;
  if (offsets[nrays] > 0 && (!rows || !section || !flag)) return srt_set_error(SRT_EINVAL, "srt_tubes_file_write: null argument");
  if (const int rc = srt_host::refuse_beyond_i10("srt_tubes_file_write", "ray", nrays, raynum)) return rc;
  return srt_host::write_text(path, [&](TextWriter &t) {
    for (int64_t r = 0; r < nrays; ++r)
      for (int64_t j = offsets[r]; j < offsets[r + 1]; ++j) {
        if (flag[j] == 1) continue;
        t.i10(raynum[r]).i10(j - offsets[r] + 1).i10(flag[j]);
        t.es24(rows[(size_t)j * SRT_ROW]).es24(section + (size_t)j * 4, 4).end();
      }
  });
}

// ---- bin file: a map of srt_bin_rays as text (include/srt.h) ----
// the grid's soundness is srt_binning.hpp's prepare(), the host half of that header; -> 0 and *ncells, or -1 and `why`
static int bin_file_cells(const srt_bin_params *params, int64_t *ncells, char *why, size_t whylen) {
  srt::binning::Grid G;
  std::vector<double> edges(3 * (srt::binning::MAXN + 1));
  if (srt::binning::prepare(params, &G, edges.data(), why, whylen)) return -1;
  *ncells = G.ncells;
  return 0;
}
extern "C" int srt_bin_file_write(const char *path, const srt_bin_params *params, const int64_t *ticks, const int64_t *hits) {
  if (!path) return srt_set_error(SRT_EINVAL, "srt_bin_file_write: null path");
  int64_t ncells = 0;
  char why[200];
  if (bin_file_cells(params, &ncells, why, sizeof why)) return srt_set_error(SRT_EINVAL, "srt_bin_file_write: %s", why);
  return srt_host::write_text(path, [&](TextWriter &t) {
    t.i10(params->naxes).i10(params->nsub).es24(params->quantum).end();
    for (int a = 0; a < params->naxes; ++a) {
      t.i10(params->axis[a].kind).i10(params->axis[a].n).end();
      t.es24(params->axis[a].edges, (size_t)params->axis[a].n + 1).end();
    }
    for (int64_t c = 0; c < ncells; ++c) t.es24(ticks ? (double)ticks[c] * params->quantum : 0.0).i20(hits ? hits[c] : 0).end();
  });
}

extern "C" int srt_bin_file_read(const char *path, srt_bin_params *params, double **edges, int64_t *ncells, double **sum, int64_t **hits) {
  if (!path || !params || !edges || !ncells || !sum || !hits) return srt_set_error(SRT_EINVAL, "srt_bin_file_read: null argument");
  *edges = nullptr, *sum = nullptr, *hits = nullptr, *ncells = 0;
  std::vector<double> all;
  std::string err;
  if (!srt_host::read_all_numbers(path, all, err)) return srt_set_error(SRT_EIO, "%s: %s", path, err.c_str());
  if (all.size() < 3 || !(all[0] >= 1.0 && all[0] <= 3.0) || all[0] != std::floor(all[0]) || all[1] != std::floor(all[1]) ||
      !(all[1] >= 1.0 && all[1] <= 64.0))
    return srt_set_error(SRT_EIO, "%s: bin file header (naxes nsub quantum) incomplete or out of range", path);
  memset(params, 0, sizeof *params);
  params->naxes = (int32_t)all[0];
  params->nsub = (int32_t)all[1];
  params->quantum = all[2];
  size_t at = 3, eoff[3] = {0, 0, 0}, nedges = 0;
  for (int a = 0; a < params->naxes; ++a) {
    if (at + 2 > all.size() || all[at + 1] != std::floor(all[at + 1]) || !(all[at + 1] >= 1.0 && all[at + 1] <= 1024.0) ||
        all[at] != std::floor(all[at]) || !(all[at] >= 0.0 && all[at] <= 7.0))
      return srt_set_error(SRT_EIO, "%s: bin file: the header of axis %d (kind n) is cut short or out of range", path, a);
    params->axis[a].kind = (int32_t)all[at];
    params->axis[a].n = (int32_t)all[at + 1];
    at += 2;
    if (at + (size_t)params->axis[a].n + 1 > all.size())
      return srt_set_error(SRT_EIO, "%s: bin file: the edges of axis %d are cut short", path, a);
    eoff[a] = at;
    at += (size_t)params->axis[a].n + 1;
    nedges += (size_t)params->axis[a].n + 1;
  }
  double *ed = copy_out<double>(nedges);
  if (!ed) return srt_set_error(SRT_ENOMEM, "bin file of %zu edges", nedges);
  size_t k = 0;
  for (int a = 0; a < params->naxes; ++a) {
    params->axis[a].edges = ed + k;
    for (int i = 0; i <= params->axis[a].n; ++i) ed[k++] = all[eoff[a] + i];
  }
  int64_t nc = 0;
  char why[200];
  if (bin_file_cells(params, &nc, why, sizeof why)) {
    free(ed);
    memset(params, 0, sizeof *params);
    return srt_set_error(SRT_EIO, "%s: bin file: %s", path, why);
  }
  if ((double)(all.size() - at) != 2.0 * (double)nc) {
    free(ed);
    memset(params, 0, sizeof *params);
    return srt_set_error(SRT_EIO, "%s: bin file holds %zu values after its axes, its header announces %lld cells of two", path,
                         all.size() - at, (long long)nc);
  }
  double *sm = copy_out<double>((size_t)nc);
  int64_t *hh = copy_out<int64_t>((size_t)nc);
  if (!sm || !hh) {
    free(ed), free(sm), free(hh);
    memset(params, 0, sizeof *params);
    return srt_set_error(SRT_ENOMEM, "bin file of %lld cells", (long long)nc);
  }
  for (int64_t c = 0; c < nc; ++c) {
    sm[c] = all[at + 2 * (size_t)c];
    hh[c] = (int64_t)all[at + 2 * (size_t)c + 1];
  }
  *edges = ed, *ncells = nc, *sum = sm, *hits = hh;
  return SRT_OK;
}

// ---- frame rotation SM <-> MAG (xform_double's sm_to_mag_d / mag_to_sm_d; srt_xform.hpp) ----
extern "C" int srt_sm_to_mag(int yearday, int msec, int inverse, int64_t n, const double *x, double *out) {
  if (inverse != 0 && inverse != 1) return srt_set_error(SRT_EINVAL, "srt_sm_to_mag: inverse = %d is neither 0 (SM -> MAG) nor 1 (MAG -> SM)", inverse);
  if (n < 0 || (n > 0 && (!x || !out))) return srt_set_error(SRT_EINVAL, "srt_sm_to_mag: bad argument");
  const srt::xform::Chain ch = srt::xform::chain(yearday, msec, inverse == 1);
  for (int64_t i = 0; i < n; ++i) srt::xform::apply(ch, x + 3 * i, out + 3 * i);
  return SRT_OK;
}

// ---- dump files: the last lines of dumpmodel.f95 (:1284-1292): (5i10) nspec nx ny nz; (6es24.15e3) the bounds; then every
// value of f(4 nspec + 3, nx, ny, nz) in array order, one (es24.15e3) record each
extern "C" int srt_dump_file_write(const char *path, int nspec, int nx, int ny, int nz, const double bounds[6], const double *f) {
  if (!path || !bounds || !f) return srt_set_error(SRT_EINVAL, "null argument");
  if (nspec < 1 || nspec > SRT_MAXSPEC || nx < 1 || ny < 1 || nz < 1) return srt_set_error(SRT_EINVAL, "bad dump shape");
  const size_t n = (size_t)nx * ny * nz * (4 * (size_t)nspec + 3);
  return srt_host::write_text(path, [&](TextWriter &t) {
    t.i10(nspec).i10(nx).i10(ny).i10(nz).end();
    t.es24(bounds, 6).end();
    for (size_t c = 0; c < n; ++c) t.es24(f[c]).end();
  });
}

extern "C" int srt_dump_file_read(const char *path, int32_t dims[4], double bounds[6], double **f) {
  if (!path || !dims || !bounds || !f) return srt_set_error(SRT_EINVAL, "null argument");
  *f = nullptr;
  std::vector<double> all;
  std::string err;
  if (!srt_host::read_all_numbers(path, all, err)) return srt_set_error(SRT_EIO, "%s: %s", path, err.c_str());
  if (all.size() < 10) return srt_set_error(SRT_EIO, "%s: dump file header incomplete", path);
  for (int k = 0; k < 4; ++k) {
    if (!(all[k] >= 1.0 && all[k] <= 2147483647.0) || all[k] != std::floor(all[k]) || (k == 0 && all[k] > SRT_MAXSPEC))
      return srt_set_error(SRT_EIO, "%s: dump file header: %s = %g", path, k == 0 ? "nspec" : k == 1 ? "nx" : k == 2 ? "ny" : "nz", all[k]);
    dims[k] = (int32_t)all[k];
  }
  const double want = (4.0 * dims[0] + 3.0) * dims[1] * dims[2] * dims[3];
  if ((double)(all.size() - 10) != want)
    return srt_set_error(SRT_EIO, "%s: dump file holds %zu values, its header (nspec nx ny nz = %d %d %d %d) announces %.0f", path,
                         all.size() - 10, dims[0], dims[1], dims[2], dims[3], want);
  for (int k = 0; k < 6; ++k) bounds[k] = all[4 + k];
  const size_t n = all.size() - 10;
  *f = copy_out(n, all.data() + 10);
  if (!*f) return srt_set_error(SRT_ENOMEM, "dump of %zu values", n);
  return SRT_OK;
}

// ---- model-4 sample files (include/srt.h) ----
extern "C" int srt_points_file_write(const char *path, int binary, int nspec, int64_t npts, const double bounds[6], const double *qs,
                                     const double *ms, const double *records) {
  if (!path || !bounds || !qs || !ms || (npts > 0 && !records) || npts < 0) return srt_set_error(SRT_EINVAL, "bad argument");
  if (nspec < 1 || nspec > SRT_MAXSPEC) return srt_set_error(SRT_EINVAL, "nspec=%d unsupported", nspec);
  return srt_host::write_points_file(path, binary != 0, nspec, npts, bounds, qs, ms, records);
}
extern "C" int srt_points_file_is_binary(const char *path) { return path && srt_host::has_magic(path, srt_host::PTS_MAGIC) ? 1 : 0; }
extern "C" int srt_points_file_convert(const char *in, const char *out_binary) {
  if (!in || !out_binary) return srt_set_error(SRT_EINVAL, "null argument");
  std::vector<double> all;
  std::string err;
  if (srt_host::has_magic(in, srt_host::PTS_MAGIC)) return srt_set_error(SRT_EINVAL, "%s is already binary", in);
  if (!srt_host::read_all_numbers(in, all, err) || all.size() < 7) return srt_set_error(SRT_EIO, "%s: %s", in, err.empty() ? "too short" : err.c_str());
  srt_host::PointsText p;
  if (!srt_host::split_points_text(all, p))
    return srt_set_error(SRT_EIO, "%s: not a model-4 sample file (or records do not match their READs)", in);
  return srt_host::write_points_file(out_binary, true, p.nspec, p.npts, p.bounds, p.qs, p.ms, p.rec);
}
