// srt_binning.hpp -- traced rays binned onto a grid (include/srt.h, "dwell time and power maps"): the coordinate functions of
// an axis, the half-open edge search, the midpoint samples of an interval on srt_rows.hpp's Hermite curve, their
// weights and deposits in integer ticks, the whole routine of one packed row, and the kernel over packed rows.
//
// Two halves, as srt_crossings.hpp.  The POINT FUNCTIONS are __host__ __device__ and spell out every operation with contraction
// off, so that a host build (tests/native/binning_host.cpp) and the device give the same integers wherever sqrt and atan2 give
// the same bits.  The KERNEL has one work item per packed row j: the interval that starts there.  A lane merges consecutive
// samples that fall into the same cell and hands each run over once; where the runs go is the only thing the two accumulation
// paths differ in, and since cells hold integers every path gives the same map:
//   ncells <= LDS_CELLS (4096): a block-private copy of the grid in LDS (ticks 8 B, hits 4 B a cell), LDS atomics, and one
//                               flush of the cells that are not zero per block with global atomics;
//   larger grids:               global atomics on unsigned long long, one per run.
// The path is chosen from the cell count alone.  The edges of all axes (at most 3 x 1025 doubles) are staged in LDS by every
// block on both paths: with LDS_CELLS cells the axes hold at most 1032 edges, 8256 B + 49152 B + 32 B of counters < 64 KiB.
//
// Compiles for the device (hipcc) and for the host.
#pragma once
#include "srt_rows.hpp"

namespace srt {
namespace binning {

constexpr int MAXN = 1024;                // cells per axis
constexpr int MAXSUB = 64;                // samples per interval
constexpr int NKINDS = 8;                 // x y z r rho L sinlat mlt
constexpr long long MAXCELLS = 2147483647ll;
constexpr long long LDS_CELLS = 4096;     // the threshold between the two accumulation paths
constexpr double TICK_LIMIT = 4611686018427387904.0; // 2^62
constexpr double PI = 3.141592653589793;

// the grid as the passes read it; the edges of axis a are edges[eoff[a] .. eoff[a] + n[a]] of one array beside it
struct Grid {
  int32_t naxes, nsub;
  int32_t kind[3], n[3], eoff[3];
  int32_t nedges;
  long long ncells;
  double quantum, C;
};

// Host: the refusals of include/srt.h, by name.  0 = fine, *G is ready and edges[G->nedges] (room for 3 * (MAXN + 1)) holds
// the axes' edges one after another; otherwise `why` says what is wrong.
inline int prepare(const srt_bin_params *p, Grid *G, double *edges, char *why, size_t whylen) {
  if (!p) {
    snprintf(why, whylen, "null params");
    return -1;
  }
  if (p->naxes < 1 || p->naxes > 3) {
    snprintf(why, whylen, "naxes = %d is outside 1 .. 3", (int)p->naxes);
    return -1;
  }
  if (p->nsub < 1 || p->nsub > MAXSUB) {
    snprintf(why, whylen, "nsub = %d is outside 1 .. %d", (int)p->nsub, MAXSUB);
    return -1;
  }
  if (!__builtin_isfinite(p->quantum) || !(p->quantum > 0.0)) {
    snprintf(why, whylen, "quantum = %g is not a finite number > 0", p->quantum);
    return -1;
  }
  G->naxes = p->naxes;
  G->nsub = p->nsub;
  G->quantum = p->quantum;
  G->C = rows::light_speed();
  G->ncells = 1;
  G->nedges = 0;
  for (int a = 0; a < 3; ++a) G->kind[a] = 0, G->n[a] = 1, G->eoff[a] = 0;
  for (int a = 0; a < p->naxes; ++a) {
    const srt_bin_axis &x = p->axis[a];
    if (x.kind < 0 || x.kind >= NKINDS) {
      snprintf(why, whylen, "axis %d: unknown kind %d (0 x, 1 y, 2 z, 3 r, 4 rho, 5 L, 6 sinlat, 7 mlt)", a, (int)x.kind);
      return -1;
    }
    if (x.n < 1 || x.n > MAXN) {
      snprintf(why, whylen, "axis %d: n = %d is outside 1 .. %d", a, (int)x.n, MAXN);
      return -1;
    }
    if (!x.edges) {
      snprintf(why, whylen, "axis %d: null edges", a);
      return -1;
    }
    for (int i = 0; i <= x.n; ++i) {
      const double e = x.edges[i];
      if (!__builtin_isfinite(e)) {
        snprintf(why, whylen, "axis %d: edge %d is not finite", a, i);
        return -1;
      }
      if (i > 0 && !(e > x.edges[i - 1])) {
        snprintf(why, whylen, "axis %d: edges do not increase at edge %d", a, i);
        return -1;
      }
      if (x.kind == 6 && !(e >= -1.0 && e <= 1.0)) {
        snprintf(why, whylen, "axis %d: edge %d = %g of a sine of latitude is outside [-1, 1]", a, i, e);
        return -1;
      }
      if (x.kind == 7 && !(e >= 0.0 && e <= 24.0)) {
        snprintf(why, whylen, "axis %d: edge %d = %g of an MLT axis is outside [0, 24]", a, i, e);
        return -1;
      }
    }
  }
  // (all axes are known to be sound before anything is copied or multiplied)
  for (int a = 0; a < p->naxes; ++a) {
    const srt_bin_axis &x = p->axis[a];
    G->kind[a] = x.kind;
    G->n[a] = x.n;
    G->eoff[a] = G->nedges;
    for (int i = 0; i <= x.n; ++i) edges[G->nedges++] = x.edges[i];
    G->ncells *= x.n;
    if (G->ncells > MAXCELLS) { // (three axes of MAXN cells hold 2^30: out of reach until either cap moves)
      snprintf(why, whylen, "the grid has too many cells (more than 2^31 - 1)");
      return -1;
    }
  }
  return 0;
}

// the coordinate of kind k at x (SM metres); not finite where it is not defined (L on the z axis, sinlat at the origin)
ROWS_HD inline double coordinate(int kind, const double x[3]) {
  ROWS_NOCONTRACT
  if (kind < 3) return x[kind];
  if (kind == 7) return fmod(24.0 * atan2(x[1], x[0]) / (2.0 * PI) + 12.0, 24.0);
  const double rho2 = x[0] * x[0] + x[1] * x[1];
  if (kind == 4) return sqrt(rho2);
  const double r2 = rho2 + x[2] * x[2];
  const double r = sqrt(r2);
  if (kind == 3) return r;
  if (kind == 5) return r2 * r / (rows::EARTH_RADIUS * rho2);
  return x[2] / r;
}

// the cell of c on an axis of n cells: i with e[i] <= c < e[i + 1]; -1 when c is outside [e[0], e[n]) or not a number
ROWS_HD inline int find_cell(const double *e, int n, double c) {
  if (!(c >= e[0]) || !(c < e[n])) return -1;
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (c >= e[mid]) lo = mid;
    else hi = mid;
  }
  return lo;
}

// the cell index of x, (i2 n1 + i1) n0 + i0; -1 = outside
ROWS_HD inline long long cell_of(const Grid &G, const double *edges, const double x[3]) {
  long long cell = 0, mul = 1;
  for (int a = 0; a < G.naxes; ++a) {
    const int i = find_cell(edges + G.eoff[a], G.n[a], coordinate(G.kind[a], x));
    if (i < 0) return -1;
    cell += mul * i;
    mul *= G.n[a];
  }
  return cell;
}

// sample k of nsub: sigma = (k + 1/2) / nsub
ROWS_HD inline double sample_sigma(int k, int nsub) {
  ROWS_NOCONTRACT
  return ((double)k + 0.5) / (double)nsub;
}
// W = rayweight (w0 + sigma (w1 - w0))
ROWS_HD inline double sample_weight(double rayw, double w0, double w1, double sigma) {
  ROWS_NOCONTRACT
  return rayw * (w0 + sigma * (w1 - w0));
}
// d / quantum of a sample, d = W hsub, hsub = h / nsub
ROWS_HD inline double sample_ticks(double W, double hsub, double quantum) {
  ROWS_NOCONTRACT
  return W * hsub / quantum;
}

// The whole routine of packed row j: decides whether the interval (j, j + 1) is used, and hands its samples to `acc` as runs
// of consecutive samples in one cell: acc(cell, ticks, hits), ticks summed modulo 2^64.  c[4] (the caller's, added to) =
// intervals used, intervals skipped, samples deposited, samples outside.  The pair of rows either side of a ray boundary is no
// interval: it is neither used nor skipped.
template <class Acc>
ROWS_HD inline void bin_row(const Grid &G, const double *edges, long long nrays, const long long *offsets, long long total,
                            const double *rows, const double *rowweight, const double *rayweight, long long j, Acc &acc,
                            unsigned long long c[4]) {
  if (j + 1 >= total) return;
  const long long r = rows::ray_of_row(offsets, nrays, j);
  if (r < 0 || j + 1 >= offsets[r + 1]) return;
  const double *r0 = rows + j * SRT_ROW, *r1 = r0 + SRT_ROW;
  const bool weighted = rowweight || rayweight;
  const double w0 = rowweight ? rowweight[j] : 1.0, w1 = rowweight ? rowweight[j + 1] : 1.0, rayw = rayweight ? rayweight[r] : 1.0;
  if (!rows::interval_usable(r0, r1) || !__builtin_isfinite(w0) || !__builtin_isfinite(w1) || !__builtin_isfinite(rayw)) {
    c[1] += 1;
    return;
  }
  rows::Interval iv;
  rows::interval_setup(r0, r1, G.C, iv);
  double hsub;
  {
    ROWS_NOCONTRACT
    hsub = iv.h / (double)G.nsub;
  }
  // a deposit of 2^62 ticks or more (or none that is a number) at ANY sample skips the interval whole: looked at first
  const int ncheck = weighted ? G.nsub : 1; // (without weights every sample deposits the same)
  for (int k = 0; k < ncheck; ++k) {
    const double q = sample_ticks(sample_weight(rayw, w0, w1, sample_sigma(k, G.nsub)), hsub, G.quantum);
    if (!(fabs(q) < TICK_LIMIT)) {
      c[1] += 1;
      return;
    }
  }
  c[0] += 1;
  long long run_cell = -1;
  unsigned long long run_ticks = 0, run_hits = 0;
  for (int k = 0; k < G.nsub; ++k) {
    const double sigma = sample_sigma(k, G.nsub);
    double x[3];
    rows::hermite(iv, sigma, x);
    const long long cell = cell_of(G, edges, x);
    if (cell < 0) {
      c[3] += 1;
      continue;
    }
    const long long t = llrint(sample_ticks(sample_weight(rayw, w0, w1, sigma), hsub, G.quantum));
    if (cell != run_cell) {
      if (run_hits) acc(run_cell, run_ticks, run_hits);
      run_cell = cell;
      run_ticks = 0;
      run_hits = 0;
    }
    run_ticks += (unsigned long long)t;
    run_hits += 1;
    c[2] += 1;
  }
  if (run_hits) acc(run_cell, run_ticks, run_hits);
}

#if defined(__HIPCC__) && !defined(SRT_BINNING_NO_KERNELS) // (a host-only build has no code object for kernels to live in)
constexpr int BLOCK = 256;

// LDS a block asks for: the edges, four counters, and on the LDS path the block's copy of the grid
inline size_t lds_bytes(const Grid &G) {
  size_t b = ((size_t)G.nedges + 4) * 8;
  if (G.ncells <= LDS_CELLS) b += (size_t)G.ncells * 12;
  return b;
}

struct AccLds {
  unsigned long long *ticks;
  unsigned int *hits;
  __device__ void operator()(long long cell, unsigned long long t, unsigned long long h) const {
    atomicAdd(ticks + cell, t);
    atomicAdd(hits + cell, (unsigned int)h);
  }
};
struct AccGlobal {
  unsigned long long *ticks, *hits;
  __device__ void operator()(long long cell, unsigned long long t, unsigned long long h) const {
    if (ticks) atomicAdd(ticks + cell, t);
    if (hits) atomicAdd(hits + cell, h);
  }
};

// A block sees at most 64 samples per row; the launch gives a block of the LDS path fewer than 2^22 rows (launch_blocks: 2^31
// rows at most over LDS_BLOCKS blocks), so a cell's 32-bit hit count in LDS cannot wrap.
constexpr long long LDS_BLOCKS = 1024, GLOBAL_BLOCKS = 65536;
inline unsigned launch_blocks(const Grid &G, long long total) {
  const long long want = (total + BLOCK - 1) / BLOCK, cap = G.ncells <= LDS_CELLS ? LDS_BLOCKS : GLOBAL_BLOCKS;
  return (unsigned)(want < cap ? want : cap);
}
template <bool LDSGRID>
__global__ __launch_bounds__(BLOCK) void bin_kernel(Grid G, const double *__restrict__ g_edges, long long nrays,
                                                    const long long *__restrict__ offsets, long long total,
                                                    const double *__restrict__ rows, const double *__restrict__ rowweight,
                                                    const double *__restrict__ rayweight, unsigned long long *__restrict__ ticks,
                                                    unsigned long long *__restrict__ hits, unsigned long long *__restrict__ counters) {
  extern __shared__ double smem[];
  double *s_edges = smem;
  unsigned long long *s_count = (unsigned long long *)(smem + G.nedges);
  unsigned long long *s_ticks = s_count + 4;
  unsigned int *s_hits = (unsigned int *)(s_ticks + (LDSGRID ? G.ncells : 0));
  const int ncells = LDSGRID ? (int)G.ncells : 0;
  for (int i = threadIdx.x; i < G.nedges; i += BLOCK) s_edges[i] = g_edges[i];
  if (threadIdx.x < 4) s_count[threadIdx.x] = 0ull;
  for (int i = threadIdx.x; i < ncells; i += BLOCK) {
    s_ticks[i] = 0ull;
    s_hits[i] = 0u;
  }
  __syncthreads();
  unsigned long long c[4] = {0ull, 0ull, 0ull, 0ull};
  const long long stride = (long long)gridDim.x * BLOCK;
  if (LDSGRID) {
    AccLds acc{s_ticks, s_hits};
    for (long long j = (long long)blockIdx.x * BLOCK + threadIdx.x; j < total; j += stride)
      bin_row(G, s_edges, nrays, offsets, total, rows, rowweight, rayweight, j, acc, c);
  } else {
    AccGlobal acc{ticks, hits};
    for (long long j = (long long)blockIdx.x * BLOCK + threadIdx.x; j < total; j += stride)
      bin_row(G, s_edges, nrays, offsets, total, rows, rowweight, rayweight, j, acc, c);
  }
  for (int k = 0; k < 4; ++k)
    if (c[k]) atomicAdd(s_count + k, c[k]);
  __syncthreads();
  if (threadIdx.x < 4 && s_count[threadIdx.x]) atomicAdd(counters + threadIdx.x, s_count[threadIdx.x]);
  for (int i = threadIdx.x; i < ncells; i += BLOCK) {
    const unsigned int h = s_hits[i];
    if (!h) continue; // (a cell without hits has no ticks)
    if (ticks && s_ticks[i]) atomicAdd(ticks + i, s_ticks[i]);
    if (hits) atomicAdd(hits + i, (unsigned long long)h);
  }
}
#endif

} // namespace binning
} // namespace srt
