#!/usr/bin/env python3
"""Golden outputs for the interp model's ring residency (srt_models.hpp, InterpModel::density_stencil): a lookup reuses the
species its wave's LDS ring still holds for the lanes whose cell did not change and re-stages only the other lanes' rows.
The cases here make that re-staging frequent, and their outputs must not move by a bit:

  * a coarse 40^3 grid (cells of ~1.6e6 m, a few adaptive steps each), nspec = 4 and nspec = 1 (one species: the whole block
    stays resident);
  * more rays than the launch has lanes (one wave per CU), so that lanes are refilled with new rays mid-launch;
  * adaptive RKF45 and fixed-step RK4 traces;
  * srt_rk_step / srt_gradients at states taken from the traces' rows, with steps long enough that the RK stages of one
    lane land in other cells (the layered kernels: one lookup per stage, the ring shared by the wave's 64 items).

Outputs are kept as sha256 digests of their bytes (plus a few sums to read when a digest differs).  Recorded with the
library from before the residency change, on an MI355X:

    SRT_LIB_OVERRIDE=<pre-change libsrt_hip.so> python tests/golden/make_ring_residency_golden.py OUT.npz
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NRAYS = 20000
GRID = 40
WAVES_PER_CU = "1"  # SRT_WAVES_PER_CU: fewer lanes than rays -> refills
C_LIGHT = 2.99792458e8  # (k = n w / c: only makes the inputs; any constant would do)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def compute():
    """-> {name: str digest or float64 array} for every case; needs the GPU."""
    from stanford_raytracer_amd import api, workloads as wl

    api.init(0)
    os.environ["SRT_WAVES_PER_CU"] = WAVES_PER_CU
    F4, b = wl.make_grid(GRID, half_width=5 * wl.R_E)
    pos, d, w = wl.launch_set(NRAYS, 11)
    out = {}
    try:
        for ns in (4, 1):
            m = api.Model.interp(np.ascontiguousarray(F4[..., :ns]), b, wl.QS[:ns], wl.MS[:ns])
            for fixed in (0, 1):
                kw = dict(fixedstep=fixed, dt0=1e-3 if not fixed else 2e-3, dtmax=0.1, tmax=0.6, maxerr=5e-4,
                          maxsteps=96, del_=1e-6, outputper=8)
                rows, nrows, stop, steps = m.trace(pos, d, w, **kw)
                tag = "ns%d_%s" % (ns, "rk4" if fixed else "rkf45")
                out[tag + "_rows"] = digest(rows)
                out[tag + "_nrows"] = digest(nrows)
                out[tag + "_stop"] = digest(stop)
                out[tag + "_sums"] = np.array([float(steps), float(nrows.sum()), float(np.nansum(rows[:, :, 1:4]))])
                if fixed == 0:
                    # states for the layered kernels: every kept row of the first 512 rays that has one
                    sel = rows[:512, 1:, :]
                    keep = sel[:, :, 0] > 0
                    st = sel[keep][:2048]
                    k = st[:, 10:13] * (w[:512, None].repeat(sel.shape[1], 1)[keep][:2048] / C_LIGHT)[:, None]
                    ww = w[:512, None].repeat(sel.shape[1], 1)[keep][:2048]
                    args = np.concatenate([st[:, 1:4], k, ww[:, None]], axis=1)
                    dt = np.full(args.shape[0], 0.08)
                    rk = m.rk_step(args, dt, 1e-6)
                    gr = m.gradients(args[:, :3], args[:, 3:6], args[:, 6], 1e-6)
                    out["ns%d_rkstep" % ns] = digest(rk)
                    out["ns%d_gradients" % ns] = digest(gr)
                    out["ns%d_layered_sums" % ns] = np.array([float(args.shape[0]), float(np.nansum(rk)), float(np.nansum(gr))])
            m.close()
    finally:
        os.environ.pop("SRT_WAVES_PER_CU", None)
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "ring_residency_golden.npz")
    out = compute()
    np.savez_compressed(path, **{k: (np.array(v) if isinstance(v, str) else v) for k, v in out.items()})
    print("wrote", path, len(out), "entries")


if __name__ == "__main__":
    main()
