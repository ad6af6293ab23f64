"""Traced rays binned onto a grid (include/srt.h, "dwell time and power maps"): the numpy restatement the tests hold the library
against, and the case builders B1 .. B7 shared by the CPU tests (tests/test_binning_host.py, the host build of
csrc/srt_binning.hpp) and the GPU tests (tests/test_gpu_binning.py).

The restatement has the header's definition in the header's order of operations and nothing of its code: the Delta form of the
cubic, plain np.searchsorted(side="right") - 1, np.rint, np.add.at on int64.  Cells hold integers, so the library is held to
EQUALITY with it, under one precondition on the inputs (assert_clear_of_edges): no sample's coordinate lies within
1e-9 max(|c|, edge spacing) of an edge (1e-9 rad for MLT), so that a last-bit difference of sqrt or atan2 between two builds
cannot move a sample across an edge.  It is a condition on the cases, not a tolerance on the result.

Where a truth exists that owes nothing to either (B1: a ray of constant velocity spends in a cell the length of a clipped
interval of time) the bar is derived, not measured: per cell
    |ticks quantum - true dwell time| <= (crossings of the cell's boundary) h_max / (2 nsub) + deposits quantum / 2 + 1e-12 T:
a piece that straddles a boundary misplaces at most half of itself, a deposit is rounded by at most half a quantum."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

import crossings_cases as cc

ROW = 20
R_E = cc.R_E
C_LIGHT = cc.C_LIGHT
QUANTUM = 2.0 ** -30
X, Y, Z, R, RHO, L, SINLAT, MLT = range(8)
TICK_LIMIT = 2.0 ** 62


# ---------------------------------------------------------------------------------------------- the restatement
def coordinate(kind, x):
    """x[..., 3] in SM metres -> the coordinate of `kind`"""
    with np.errstate(all="ignore"):
        if kind < 3:
            return x[..., kind]
        if kind == MLT:
            return np.fmod(24.0 * np.arctan2(x[..., 1], x[..., 0]) / (2.0 * np.pi) + 12.0, 24.0)
        rho2 = x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1]
        if kind == RHO:
            return np.sqrt(rho2)
        r2 = rho2 + x[..., 2] * x[..., 2]
        r = np.sqrt(r2)
        if kind == R:
            return r
        if kind == L:
            return r2 * r / (R_E * rho2)
        return x[..., 2] / r


def shape_of(axes):
    return tuple(len(e) - 1 for _, e in axes)[::-1]


def zeros(axes):
    """-> (ticks, hits, counters) to accumulate into"""
    n = int(np.prod([len(e) - 1 for _, e in axes]))
    return np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(4, dtype=np.int64)


def reference(offsets, rows, axes, nsub, quantum=QUANTUM, row_weight=None, ray_weight=None, into=None, samples=None):
    """The definition.  axes = [(kind, edges)]; ACCUMULATES into `into` = (ticks, hits, counters) (flat, int64) or starts from
    zeros; -> (ticks, hits, counters).  `samples`, a list, receives (axis index, coordinates of all samples of used intervals)."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, ROW)
    offsets = np.asarray(offsets, dtype=np.int64)
    ticks, hits, counters = into if into is not None else zeros(axes)
    nrays = len(offsets) - 1
    lens = np.maximum(np.diff(offsets) - 1, 0)
    if lens.sum() == 0:
        return ticks, hits, counters
    j = np.concatenate([np.arange(offsets[r], offsets[r] + lens[r]) for r in range(nrays)]).astype(np.int64)
    ray = np.repeat(np.arange(nrays), lens)
    r0, r1 = rows[j], rows[j + 1]
    one = np.ones(len(j))
    w0 = one if row_weight is None else np.asarray(row_weight, dtype=np.float64)[j]
    w1 = one if row_weight is None else np.asarray(row_weight, dtype=np.float64)[j + 1]
    yw = one if ray_weight is None else np.asarray(ray_weight, dtype=np.float64)[ray]
    cols = [0, 1, 2, 3, 7, 8, 9]
    ok = np.isfinite(r0[:, cols]).all(1) & np.isfinite(r1[:, cols]).all(1) & (r1[:, 0] != r0[:, 0])
    ok &= np.isfinite(w0) & np.isfinite(w1) & np.isfinite(yw)
    sigma = (np.arange(nsub, dtype=np.float64) + 0.5) / float(nsub)
    with np.errstate(all="ignore"):
        h = r1[:, 0] - r0[:, 0]
        hsub = h / float(nsub)
        W = yw[:, None] * (w0[:, None] + sigma[None, :] * (w1 - w0)[:, None])
        q = W * hsub[:, None] / quantum
        used = ok & (np.abs(q) < TICK_LIMIT).all(1)
    counters[0] += int(used.sum())
    counters[1] += int((~used).sum())
    if not used.any():
        return ticks, hits, counters
    r0, r1, h, q = r0[used], r1[used], h[used], q[used]
    d = r1[:, 1:4] - r0[:, 1:4]
    m0, m1 = C_LIGHT * r0[:, 7:10] * h[:, None], C_LIGHT * r1[:, 7:10] * h[:, None]
    c2, c3 = 3.0 * d - 2.0 * m0 - m1, m0 + m1 - 2.0 * d
    s = sigma[None, :, None]
    p = r0[:, None, 1:4] + s * (m0[:, None, :] + s * (c2[:, None, :] + s * c3[:, None, :]))
    cell = np.zeros(p.shape[:2], dtype=np.int64)
    inside = np.ones(p.shape[:2], dtype=bool)
    mul = 1
    for a, (kind, edges) in enumerate(axes):
        edges = np.asarray(edges, dtype=np.float64)
        c = coordinate(kind, p)
        if samples is not None:
            samples.append((a, c.copy()))
        i = np.searchsorted(edges, c, side="right") - 1
        inside &= (i >= 0) & (i < len(edges) - 1) & np.isfinite(c)
        cell += mul * np.clip(i, 0, len(edges) - 2)
        mul *= len(edges) - 1
    t = np.rint(q).astype(np.int64)
    np.add.at(ticks, cell[inside], t[inside])
    np.add.at(hits, cell[inside], 1)
    counters[2] += int(inside.sum())
    counters[3] += int((~inside).sum())
    return ticks, hits, counters


def assert_clear_of_edges(offsets, rows, axes, nsub, row_weight=None, ray_weight=None):
    """The precondition of integer equality (module docstring), asserted on the reference's own samples."""
    samples = []
    reference(offsets, rows, axes, nsub, QUANTUM, row_weight, ray_weight, samples=samples)
    for a, c in samples:
        kind, edges = axes[a]
        edges = np.asarray(edges, dtype=np.float64)
        c = c[np.isfinite(c)]
        if not c.size:
            continue
        gap = np.abs(c[:, None] - edges[None, :]).min(1)
        tol = 1e-9 * 24.0 / (2.0 * np.pi) if kind == MLT else 1e-9 * np.maximum(np.abs(c), np.diff(edges).max())
        assert np.all(gap > tol), ("a sample within 1e-9 of an edge", a, kind, float((gap / tol).min()))


def check_identities(ticks, hits, counters, nsub, offsets):
    used, skipped, deposited, outside = (int(v) for v in counters)
    assert deposited + outside == nsub * used
    assert int(np.sum(hits)) == deposited
    assert used + skipped == int(np.maximum(np.diff(offsets) - 1, 0).sum())
    assert np.all(np.asarray(hits) >= 0) and np.all(np.asarray(ticks)[np.asarray(hits) == 0] == 0)


# ---------------------------------------------------------------------------------------------- B1: known answers
def line_rows(a, v, times):
    """Rows at `times` on p(t) = a + v t, vgrel = v / C: the Hermite curve is the line to rounding."""
    t = np.asarray(times, dtype=np.float64)
    rows = np.zeros((len(t), ROW))
    rows[:, 0] = t
    rows[:, 1:4] = np.asarray(a)[None, :] + t[:, None] * np.asarray(v)[None, :]
    rows[:, 7:10] = np.asarray(v)[None, :] / C_LIGHT
    rows[:, 16:20] = 1e9
    return rows


B1_EDGES = (np.linspace(-4.0, 4.0, 9) * R_E, np.linspace(-3.0, 5.0, 9) * R_E)  # 8 x 8 cells of 1 R_E in (x, y)


def b1_cartesian(seed=3, nlines=12):
    """-> offsets, rows, axes, lines = [(a, v, t0, t1, hmax)]: rays of constant velocity through the 8 x 8 (x, y) grid, some
    starting or ending inside it, rows at uneven times."""
    rng = np.random.default_rng(seed)
    rays, lines = [], []
    for _ in range(nlines):
        a = np.array([rng.uniform(-5, 5), rng.uniform(-4, 6), rng.uniform(-1, 1)]) * R_E
        b = np.array([rng.uniform(-5, 5), rng.uniform(-4, 6), rng.uniform(-1, 1)]) * R_E
        T = rng.uniform(0.5, 2.0)
        t = np.sort(np.concatenate([[0.0, T], rng.uniform(0.0, T, rng.integers(3, 12))]))
        t = t[np.concatenate([[True], np.diff(t) > 1e-3])]
        v = (b - a) / T
        rays.append(line_rows(a, v, t))
        lines.append((a, v, t[0], t[-1], float(np.diff(t).max())))
    offsets, rows = cc.pack(rays)
    return offsets, rows, [(X, B1_EDGES[0]), (Y, B1_EDGES[1])], lines


def b1_cartesian_truth(lines, axes):
    """-> (dwell[ncells], crossings[ncells] weighted by h_max of the ray that crosses): the time each line spends in each cell by
    clipping its interval of time against the cell's two slabs."""
    (_, ex), (_, ey) = axes
    nx, ny = len(ex) - 1, len(ey) - 1
    dwell, slack = np.zeros(nx * ny), np.zeros(nx * ny)
    for a, v, t0, t1, hmax in lines:
        for iy in range(ny):
            for ix in range(nx):
                lo, hi = t0, t1
                for c, (e0, e1) in ((0, (ex[ix], ex[ix + 1])), (1, (ey[iy], ey[iy + 1]))):
                    if v[c] == 0.0:
                        if not (e0 <= a[c] < e1):
                            lo, hi = 1.0, 0.0
                        continue
                    ta, tb = sorted(((e0 - a[c]) / v[c], (e1 - a[c]) / v[c]))
                    lo, hi = max(lo, ta), min(hi, tb)
                if hi > lo:  # the line is in the cell during (lo, hi): a sample is a point of the line, so no other cell of
                    dwell[iy * nx + ix] += hi - lo  # this ray receives one; an end that is not the ray's own is a crossing
                    slack[iy * nx + ix] += (int(lo > t0) + int(hi < t1)) * hmax
    return dwell, slack


def b1_radial(nsub_dummy=None):
    """-> offsets, rows, axes, (dwell per cell): one ray straight out along a fixed direction at constant speed through an
    (r, sinlat) grid; sinlat is constant along it, r = r_a + speed t."""
    u = np.array([0.6, 0.3, 0.5])
    u = u / np.linalg.norm(u)
    ra, speed, T = 1.2 * R_E, 2.9 * R_E, 1.0
    t = np.array([0.0, 0.11, 0.19, 0.4, 0.47, 0.7, 0.93, 1.0])
    rows = line_rows(ra * u, speed * u, t)
    er = np.array([1.0, 1.5, 2.0, 2.35, 3.0, 3.7, 4.5]) * R_E
    es = np.array([-1.0, 0.0, 0.5, 0.75, 1.0])
    offsets, rows = cc.pack([rows])
    s = u[2]
    js = int(np.searchsorted(es, s, side="right") - 1)
    nr = len(er) - 1
    dwell, slack = np.zeros(nr * (len(es) - 1)), np.zeros(nr * (len(es) - 1))
    hmax = float(np.diff(t).max())
    for i in range(nr):
        lo, hi = max(0.0, (er[i] - ra) / speed), min(T, (er[i + 1] - ra) / speed)
        if hi > lo:
            dwell[js * nr + i] = hi - lo
            slack[js * nr + i] = (int(lo > 0.0) + int(hi < T)) * hmax
    return offsets, rows, [(R, er), (SINLAT, es)], dwell, slack, T


def b1_check(ticks, hits, dwell, slack, nsub, total_time, quantum=QUANTUM, label=""):
    got = np.asarray(ticks, dtype=np.float64).ravel() * quantum
    bound = slack / (2.0 * nsub) + np.asarray(hits).ravel() * quantum / 2.0 + 1e-12 * total_time
    err = np.abs(got - dwell)
    worst = float((err / bound).max())
    print("%s nsub %d: worst |ticks quantum - dwell| / bound = %.3f, max error %.3g s of %.3g s" % (label, nsub, worst, err.max(), dwell.sum()))
    assert np.all(err <= bound), (label, nsub, worst)
    return worst


# ---------------------------------------------------------------------------------------------- B2: the definition
# edges per kind, chosen to hold most of the C1 arcs (1.15 R_E at -35 degrees to 3.4 R_E at +30 degrees, near the x-z plane) and
# leave some of them outside; uneven on purpose
def _edges(kind, n):
    lo, hi = {X: (0.52, 3.47), Y: (0.011, 0.066), Z: (-0.83, 1.91), R: (1.03, 3.21), RHO: (0.47, 3.13), L: (1.21, 5.93),
              SINLAT: (-0.71, 0.47), MLT: (12.07, 12.125)}[kind]
    e = lo + (hi - lo) * (np.arange(n + 1) / n) ** 1.3
    return e * R_E if kind < L else e


def b2_axes(kind, naxes):
    """kind, kind + 1, kind + 2 (mod 8) with 4, 3 and 2 cells"""
    return [((kind + a) % 8, _edges((kind + a) % 8, (4, 3, 2)[a])) for a in range(naxes)]


def b2_rows():
    offsets, rows, _ = cc.c1_case()
    return offsets, rows


def b2_log_l():
    """uneven edges: log-spaced L, 12 cells, over a 5-cell sine of latitude"""
    return [(L, np.geomspace(1.07, 7.3, 13)), (SINLAT, np.array([-0.9, -0.33, -0.05, 0.21, 0.4, 0.93]))]


# ---------------------------------------------------------------------------------------------- B3: edges
def b3_rows(points):
    """One ray per point pair (p0, p1): two rows with vgrel = 0, t = 0 and 1; with nsub = 1 the one sample is p0 + D / 2 exactly
    when the coordinates are representable (the cubic's terms are 3 D / 4 - 2 D / 8 exactly)."""
    rays = []
    for p0, p1 in points:
        r = np.zeros((2, ROW))
        r[:, 0] = [0.0, 1.0]
        r[0, 1:4], r[1, 1:4] = p0, p1
        r[:, 16:20] = 1e9
        rays.append(r)
    return cc.pack(rays)


# ---------------------------------------------------------------------------------------------- B4 .. B6
def b4_base():
    """two rays of five rows on the C1 arcs and a grid that holds them"""
    rays = [cc.rows_on_cubic(cc.C1_COEF, np.linspace(0.0, 1.0, 5)), cc.rows_on_cubic(cc.reversed_cubic(cc.C1_COEF), np.linspace(0.0, 1.0, 5))]
    return rays, [(R, _edges(R, 6)), (SINLAT, _edges(SINLAT, 5))]


def b5_weights(offsets, seed=11):
    """-> name -> (row_weight | None, ray_weight | None)"""
    rng = np.random.default_rng(seed)
    total, nrays = int(offsets[-1]), len(offsets) - 1
    rw = rng.uniform(0.0, 1.0, total) ** 2
    yw = rng.uniform(0.5, 3.0, nrays)
    neg = rng.normal(size=total)
    neg[::3] = 0.0
    return {"row": (rw, None), "ray": (None, yw), "both": (rw, yw), "negative_and_zero": (neg, None),
            "ones": (np.ones(total), np.ones(nrays)), "none": (None, None)}


def split_rays(offsets, rows, first):
    """the rays [0, first) and [first, n) as two packed sets"""
    k = int(offsets[first])
    return (offsets[:first + 1].copy(), rows[:k]), (offsets[first:] - k, rows[k:])


def permute_rays(offsets, rows, perm, row_weight=None, ray_weight=None):
    rays = [rows[int(offsets[r]):int(offsets[r + 1])] for r in perm]
    o, r = cc.pack(rays)
    rw = None if row_weight is None else np.concatenate([row_weight[int(offsets[q]):int(offsets[q + 1])] for q in perm])
    yw = None if ray_weight is None else np.asarray(ray_weight)[list(perm)]
    return o, r, rw, yw


# ---------------------------------------------------------------------------------------------- B7: real rows
def b7_r_axis():
    return [(R, np.linspace(0.0, 100.0, 41) * R_E)]


def b7_map_axes():
    """(L, magnetic latitude) 16 x 12; the latitude edges in radians, as api.axis_maglat takes them"""
    return np.geomspace(1.02, 9.7, 17), np.deg2rad(np.linspace(-61.3, 58.9, 13))


# ---------------------------------------------------------------------------------------------- the host build
HOST_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "binning_host.cpp")
HOST_FLAGS = ["-x", "hip", "--cuda-host-only", "-ffp-contract=off", "-O2", "-std=c++17"]


class CBinAxis(C.Structure):  # the tests' own mirror of srt_bin_axis (api.BinAxis is checked against gcc in B8)
    _fields_ = [("kind", C.c_int32), ("n", C.c_int32), ("edges", C.POINTER(C.c_double))]


class CBinParams(C.Structure):
    _fields_ = [("naxes", C.c_int32), ("nsub", C.c_int32), ("quantum", C.c_double), ("axis", CBinAxis * 3)]


def build_host(directory):
    """tests/native/binning_host.cpp as a shared library in `directory` -> the loaded library"""
    so = os.path.join(str(directory), "libbnh.so")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    subprocess.check_call([hipcc] + HOST_FLAGS + ["-shared", "-fPIC", "-o", so, HOST_SRC])
    lib = C.CDLL(so)
    lib.bnh_bin.argtypes = [C.POINTER(CBinParams), C.c_longlong] + [C.c_void_p] * 7 + [C.c_char_p, C.c_int]
    lib.bnh_cells.argtypes = [C.POINTER(CBinParams), C.c_char_p, C.c_int]
    lib.bnh_cells.restype = C.c_longlong
    lib.bnh_coordinate.argtypes = [C.c_int, C.c_void_p]
    lib.bnh_coordinate.restype = C.c_double
    lib.bnh_find_cell.argtypes = [C.c_void_p, C.c_int, C.c_double]
    return lib


def c_params(axes, nsub, quantum):
    p = CBinParams()
    p.naxes, p.nsub, p.quantum = len(axes), nsub, quantum
    keep = []
    for a, (kind, edges) in enumerate(axes[:3]):
        e = np.ascontiguousarray(edges, dtype=np.float64)
        keep.append(e)
        p.axis[a] = CBinAxis(kind, len(e) - 1, e.ctypes.data_as(C.POINTER(C.c_double)))
    return p, keep


def host_bin(lib, offsets, rows, axes, nsub, quantum=QUANTUM, row_weight=None, ray_weight=None, into=None):
    """The host build on a case; ACCUMULATES into `into` = (ticks, hits, counters) or starts from zeros -> the three."""
    p, keep = c_params(axes, nsub, quantum)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    rw = None if row_weight is None else np.ascontiguousarray(row_weight, dtype=np.float64)
    yw = None if ray_weight is None else np.ascontiguousarray(ray_weight, dtype=np.float64)
    ticks, hits, counters = into if into is not None else zeros(axes)
    why = C.create_string_buffer(200)
    rc = lib.bnh_bin(C.byref(p), len(offsets) - 1, offsets.ctypes.data, rows.ctypes.data, None if rw is None else rw.ctypes.data,
                     None if yw is None else yw.ctypes.data, ticks.ctypes.data, hits.ctypes.data, counters.ctypes.data, why, 200)
    assert rc == 0, why.value
    return ticks, hits, counters


def assert_same(got, want, label=""):
    """ticks, hits and counters equal as integers"""
    for name, g, w in zip(("ticks", "hits", "counters"), got, want):
        g, w = np.asarray(g).ravel(), np.asarray(w).ravel()
        assert g.dtype == np.int64 and w.dtype == np.int64 and np.array_equal(g, w), (label, name, int(np.sum(g != w)))
