#!/usr/bin/env python3
"""Golden outputs for the interp lookup's cell test of the points around a centre (srt_models.hpp: Axis::in_cell in
InterpModel::density_stencil -- the offset points and the free point are no longer searched for, they are compared against the
nodes of the centre's cell and divided by a reciprocal the axis shares; Axis::locate itself is written with selects).  No output
bit may move.  The cases aim at what make_lookup_overlap_golden.py and make_ring_residency_golden.py do not reach:

  * centres exactly ON grid nodes and one ulp either side, on each axis in turn: launch points of traces and the states handed
    to srt_rk_step / srt_gradients are snapped there (a centre on a node has its minus point in the neighbouring cell: the
    straddle path runs for every snapped state; half of the layered states are snapped);
  * centres OUTSIDE the grid on every face: the table covers +-3 R_E only while the launch set reaches 5 R_E, so a good share
    of the lookups sit in the clamped cells 0 and n with their zeroed local coordinate;
  * del_ = 0.2: the offset max(del |x_c|, del) is up to 3.8 cells long, so offset points skip whole cells;
  * adaptive traces with maxerr = 0.3 and long steps: the free point (the 4th-order end point) lies cells away from the centre;
  * nspec 1 and 4.

main() prints, per case, the share of the evaluated centres with a straddling stencil and the share in clamped cells, counted on
the host from the positions and the grid; each must be at least 1 % (the test asserts the same).  Outputs are kept as sha256
digests of their bytes (plus a few sums to read when a digest differs).  Recorded with the library from before the change, on an
MI355X:

    SRT_LIB_OVERRIDE=<pre-change libsrt_hip.so> python tests/golden/make_cell_from_centre_golden.py OUT.npz
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NRAYS = 6000
NSTATES = 3072
GRID = 24
HALF_WIDTH_RE = 3.0
DELS = (1e-3, 0.2)
WAVES_PER_CU = "1"  # SRT_WAVES_PER_CU: fewer lanes than rays -> refills
C_LIGHT = 2.99792458e8  # (k = n w / c: only makes the inputs; any constant would do)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def grid_nodes(bounds, n, a):
    lo, hi = bounds[2 * a], bounds[2 * a + 1]
    return np.arange(n) * ((hi - lo) / (n - 1.0)) + lo  # as the model computes them: i * del + min


def shares(pos, del_, bounds, n):
    """(straddle share, clamped share) of the stencils centred at pos[m, 3]: an offset point x_c +- max(del |x_c|, del) in
    another cell than the centre's; the centre in cell 0 or n of an axis (cell = number of grid nodes <= the coordinate)."""
    straddle = np.zeros(pos.shape[0], dtype=bool)
    clamped = np.zeros(pos.shape[0], dtype=bool)
    for a in range(3):
        nodes = grid_nodes(bounds, n, a)
        x = pos[:, a]
        d = np.maximum(del_ * np.abs(x), del_)
        c0 = np.searchsorted(nodes, x, side="right")
        straddle |= (np.searchsorted(nodes, x + d, side="right") != c0) | (np.searchsorted(nodes, x - d, side="right") != c0)
        clamped |= (c0 == 0) | (c0 == n)
    return float(straddle.mean()), float(clamped.mean())


def snap_to_nodes(pos, bounds, n):
    """Point i: coordinate i % 3 moved onto the nearest grid node (i // 3 % 3 == 0), one ulp above it (1) or one ulp below (2)."""
    pos = pos.copy()
    i = np.arange(pos.shape[0])
    for a in range(3):
        nodes = grid_nodes(bounds, n, a)
        sel = i % 3 == a
        x = pos[sel, a]
        near = nodes[np.clip(np.rint((x - nodes[0]) / (nodes[1] - nodes[0])).astype(np.int64), 0, n - 1)]
        how = (i[sel] // 3) % 3
        pos[sel, a] = np.where(how == 0, near, np.where(how == 1, np.nextafter(near, np.inf), np.nextafter(near, -np.inf)))
    return pos


def compute(report=None):
    """-> {name: str digest or float64 array} for every case; needs the GPU.  report: a dict that receives (straddle share,
    clamped share) per case."""
    from stanford_raytracer_amd import api, workloads as wl

    api.init(0)
    os.environ["SRT_WAVES_PER_CU"] = WAVES_PER_CU
    F4, b = wl.make_grid(GRID, half_width=HALF_WIDTH_RE * wl.R_E)
    pos, d, w = wl.launch_set(NRAYS, 23)
    pos_free, pos = pos, snap_to_nodes(pos, b, GRID)
    out = {}
    try:
        for ns in (1, 4):
            m = api.Model.interp(np.ascontiguousarray(F4[..., :ns]), b, wl.QS[:ns], wl.MS[:ns])
            for del_ in DELS:
                dtag = "ns%d_del%g" % (ns, del_)
                for fixed in (0, 1):
                    kw = dict(fixedstep=fixed, dt0=1e-3 if not fixed else 2e-3, dtmax=0.5, tmax=1.0, maxerr=0.3,
                              maxsteps=64, del_=del_, outputper=2)
                    rows, nrows, stop, steps = m.trace(pos, d, w, **kw)
                    tag = dtag + ("_rk4" if fixed else "_rkf45")
                    out[tag + "_rows"] = digest(rows)
                    out[tag + "_nrows"] = digest(nrows)
                    out[tag + "_stop"] = digest(stop)
                    out[tag + "_sums"] = np.array([float(steps), float(nrows.sum()), float(np.nansum(rows[:, :, 1:4]))])
                    if report is not None:
                        keep = np.arange(rows.shape[1])[None, :] < nrows[:, None]
                        p = rows[keep][:, 1:4]
                        report[tag] = shares(p[np.isfinite(p).all(axis=1)], del_, b, GRID)
                # the layered kernels: snapped states and, for the second half, the launch points as they were (wave vectors
                # along the launch directions, |n| = 20)
                x = np.concatenate([pos[:NSTATES // 2], pos_free[NSTATES // 2:NSTATES]])
                k = d[:NSTATES] * (20.0 * w[:NSTATES] / C_LIGHT)[:, None]
                args = np.concatenate([x, k, w[:NSTATES, None]], axis=1)
                rk = m.rk_step(args, np.full(NSTATES, 0.05), del_)
                gr = m.gradients(x, k, w[:NSTATES], del_)
                out[dtag + "_rkstep"] = digest(rk)
                out[dtag + "_gradients"] = digest(gr)
                out[dtag + "_layered_sums"] = np.array([float(NSTATES), float(np.nansum(rk)), float(np.nansum(gr))])
                if report is not None:
                    report[dtag + "_layered"] = shares(x, del_, b, GRID)
            m.close()
    finally:
        os.environ.pop("SRT_WAVES_PER_CU", None)
    return out


def low_shares(report):
    return ["%s: straddle %.4f clamped %.4f" % (k, v[0], v[1]) for k, v in sorted(report.items()) if min(v) < 0.01]


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "cell_from_centre_golden.npz")
    report = {}
    out = compute(report)
    for k in sorted(report):
        print("%-28s straddle share %.4f  clamped share %.4f" % (k, report[k][0], report[k][1]))
    if low_shares(report):
        raise SystemExit("a share below 1 %%: the cases do not exercise the path: %s" % low_shares(report))
    for k in sorted(out):
        if k.endswith("_sums"):
            print(k, out[k])
    np.savez_compressed(path, **{k: (np.array(v) if isinstance(v, str) else v) for k, v in out.items()})
    print("wrote", path, len(out), "entries")


if __name__ == "__main__":
    main()
