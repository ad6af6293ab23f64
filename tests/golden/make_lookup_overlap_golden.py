#!/usr/bin/env python3
"""Golden outputs for the interp lookup's reordering (srt_models.hpp, InterpModel::density_stencil): exp is applied species by
species inside the species loop, the cell searches of the offset points and of the free point run after the re-stage has been
issued, and a stencil point in another cell than the centre's gets its exp in the out-of-line direct evaluation.  No output
bit may move.  The cases aim at what tests/golden/make_ring_residency_golden.py does not:

  * nspec = 2 and 3: the species a model does not have stay exactly 0.0;
  * del_ = 1e-3 on the coarse 40^3 grid over +-5 R_E (cells of 1.63e6 m): the offset max(del |x_c|, del) is a few km, so a
    stencil point leaves the centre's cell in a few per cent of the lookups (the straddle path).  main() prints the share,
    counted on the host from the kept rows' positions and the grid; it must be at least 1 %;
  * adaptive traces with a loose tolerance (maxerr = 1e-2) and long steps: the free point est1 (the 4th-order end point) lies
    up to ~1e-2 |x| ~ 1e5 m from est2, a sixteenth of a cell, so that it lands in another cell in several per cent of the
    attempts (rejected attempts, further apart still, are evaluated as well);
  * srt_gradients / srt_rk_step on states taken from those traces' rows, with the same del_.

Outputs are kept as sha256 digests of their bytes (plus a few sums to read when a digest differs).  Recorded with the library
from before the change, on an MI355X:

    SRT_LIB_OVERRIDE=<pre-change libsrt_hip.so> python tests/golden/make_lookup_overlap_golden.py OUT.npz
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NRAYS = 12000
GRID = 40
HALF_WIDTH_RE = 5.0
DEL = 1e-3
WAVES_PER_CU = "1"  # SRT_WAVES_PER_CU: fewer lanes than rays -> refills
C_LIGHT = 2.99792458e8  # (k = n w / c: only makes the inputs; any constant would do)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def straddle_share(pos, del_, bounds, n):
    """Share of the stencils centred at pos[m, 3] with an offset point x_c +- max(del |x_c|, del) in another cell than the
    centre's (cell = number of grid nodes <= the coordinate, per axis; nodes as the model computes them: i * del + min)."""
    out = np.zeros(pos.shape[0], dtype=bool)
    for a in range(3):
        lo, hi = bounds[2 * a], bounds[2 * a + 1]
        nodes = np.arange(n) * ((hi - lo) / (n - 1.0)) + lo
        x = pos[:, a]
        d = np.maximum(del_ * np.abs(x), del_)
        c0 = np.searchsorted(nodes, x, side="right")
        out |= (np.searchsorted(nodes, x + d, side="right") != c0) | (np.searchsorted(nodes, x - d, side="right") != c0)
    return float(out.mean())


def compute(report=None):
    """-> {name: str digest or float64 array} for every case; needs the GPU.  report: a dict that receives the straddle
    shares per case."""
    from stanford_raytracer_amd import api, workloads as wl

    api.init(0)
    os.environ["SRT_WAVES_PER_CU"] = WAVES_PER_CU
    F4, b = wl.make_grid(GRID, half_width=HALF_WIDTH_RE * wl.R_E)
    pos, d, w = wl.launch_set(NRAYS, 17)
    out = {}
    try:
        for ns in (2, 3, 4):
            m = api.Model.interp(np.ascontiguousarray(F4[..., :ns]), b, wl.QS[:ns], wl.MS[:ns])
            for fixed in (0, 1):
                # adaptive: a loose tolerance and a large dtmax, so that est1 and est2 of an attempt are far enough apart to
                # fall into different cells at times
                kw = dict(fixedstep=fixed, dt0=1e-3 if not fixed else 2e-3, dtmax=0.2, tmax=0.8, maxerr=1e-2,
                          maxsteps=96, del_=DEL, outputper=4)
                rows, nrows, stop, steps = m.trace(pos, d, w, **kw)
                tag = "ns%d_%s" % (ns, "rk4" if fixed else "rkf45")
                out[tag + "_rows"] = digest(rows)
                out[tag + "_nrows"] = digest(nrows)
                out[tag + "_stop"] = digest(stop)
                out[tag + "_sums"] = np.array([float(steps), float(nrows.sum()), float(np.nansum(rows[:, :, 1:4]))])
                # N_s of the species the model does not have (columns 16 + ns .. 19 of a row): exactly 0.0
                out[tag + "_absent_species_absmax"] = np.array([float(np.abs(rows[:, :, 16 + ns:]).max()) if ns < 4 else 0.0])
                keep = rows[:, :, 0] > 0
                if report is not None:
                    report[tag] = straddle_share(rows[keep][:, 1:4], DEL, b, GRID)
                if fixed == 0:
                    # states for the layered kernels: every kept row of the first 512 rays that has one
                    sel = rows[:512, 1:, :]
                    keep = sel[:, :, 0] > 0
                    st = sel[keep][:2048]
                    ww = w[:512, None].repeat(sel.shape[1], 1)[keep][:2048]
                    k = st[:, 10:13] * (ww / C_LIGHT)[:, None]
                    args = np.concatenate([st[:, 1:4], k, ww[:, None]], axis=1)
                    dt = np.full(args.shape[0], 0.08)
                    rk = m.rk_step(args, dt, DEL)
                    gr = m.gradients(args[:, :3], args[:, 3:6], args[:, 6], DEL)
                    out["ns%d_rkstep" % ns] = digest(rk)
                    out["ns%d_gradients" % ns] = digest(gr)
                    out["ns%d_layered_sums" % ns] = np.array([float(args.shape[0]), float(np.nansum(rk)), float(np.nansum(gr))])
                    if report is not None:
                        report["ns%d_layered_straddle" % ns] = straddle_share(args[:, :3], DEL, b, GRID)
            m.close()
    finally:
        os.environ.pop("SRT_WAVES_PER_CU", None)
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "lookup_overlap_golden.npz")
    report = {}
    out = compute(report)
    for k in sorted(report):
        print("straddle share %-24s %.4f" % (k, report[k]))
    low = [k for k, v in report.items() if v < 0.01]
    if low:
        raise SystemExit("straddle share below 1 %% in %s: the cases do not exercise the straddle path" % low)
    for k in sorted(out):
        if k.endswith("_sums"):
            print(k, out[k])
    np.savez_compressed(path, **{k: (np.array(v) if isinstance(v, str) else v) for k, v in out.items()})
    print("wrote", path, len(out), "entries")


if __name__ == "__main__":
    main()
