#!/usr/bin/env python3
"""Golden outputs for the first terms of the interp lookup's Horner sums (srt_models.hpp: InterpModel::plane_stencil).

plane_stencil started every partial sum at 0.0, so the first step of each was fma(0.0, y, v).  The local coordinates y are finite
and >= +0, so that is v for every v but -0.0 (which it turns into +0.0), and the lookup now assigns v instead.  A zero of either
sign is absorbed by the next non-zero term, and if every later term is zero too the sum reaches exp, where exp(+-0) = 1: no
output bit may move.  The cases aim at the sums in which zeros of either sign can travel furthest:

  * flat:      ln N = 0.0 on every node (every coefficient is a zero);
  * negzero:   ln N = -0.0 on every node;
  * negblock:  the smooth plasmasphere with a block of -0.0 nodes in it (cells with zero and non-zero coefficients mixed);
  * zeroplane: the smooth plasmasphere with one z plane and one x plane of nodes at 0.0;

each on a coarse grid (12 nodes over +-3 R_E under a launch set that reaches 5 R_E: many centres in the clamped cells 0 / n, whose
local coordinate is zeroed), with nspec 4 and 2, and with a third of the states snapped onto grid nodes on all three axes (local
coordinates exactly 0: only a(0,0,0) of a cell is left, and the minus points of the stencil lie in the neighbouring cells -- the
straddle path), a third snapped on one axis, the rest as launched.  srt_plasma_params, srt_gradients and srt_rk_step on those
states and short RKF45 and RK4 traces from them, del_ = 1e-6 and 1e-3.  Outputs are kept as sha256 digests of their bytes (plus a
few sums to read when a digest differs).  Recorded with the library from before the change, on an MI355X:

    SRT_LIB_OVERRIDE=<pre-change libsrt_hip.so> python tests/golden/make_horner_first_terms_golden.py OUT.npz
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from make_cell_from_centre_golden import C_LIGHT, digest, grid_nodes, shares, snap_to_nodes  # noqa: E402

NRAYS = 1536
GRID = 12
HALF_WIDTH_RE = 3.0
DELS = (1e-6, 1e-3)
WAVES_PER_CU = "1"  # SRT_WAVES_PER_CU: fewer lanes than rays -> refills


def grids(wl):
    F, b = wl.make_grid(GRID, half_width=HALF_WIDTH_RE * wl.R_E)
    flat = np.zeros_like(F)
    negzero = np.full_like(F, -0.0)
    negblock = F.copy()
    negblock[3:8, 2:9, 4:10, :] = -0.0
    zeroplane = F.copy()
    zeroplane[5, :, :, :] = 0.0
    zeroplane[:, :, 7, :] = 0.0
    return b, {"flat": flat, "negzero": negzero, "negblock": negblock, "zeroplane": zeroplane}


def states(wl, b):
    """-> x[n,3], d[n,3], w[n]: a third on nodes on every axis, a third on a node (or one ulp beside it) on one axis, a third free"""
    pos, d, w = wl.launch_set(NRAYS, 31)
    n = pos.shape[0]
    x = pos.copy()
    third = n // 3
    for a in range(3):
        nodes = grid_nodes(b, GRID, a)
        i = np.clip(np.rint((x[:third, a] - nodes[0]) / (nodes[1] - nodes[0])).astype(np.int64), -1, GRID)
        # (nodes one step outside the grid as well: centres on the continued lattice, in the clamped cells)
        x[:third, a] = np.where((i >= 0) & (i < GRID), nodes[np.clip(i, 0, GRID - 1)], i * (nodes[1] - nodes[0]) + nodes[0])
    x[third:2 * third] = snap_to_nodes(pos[third:2 * third], b, GRID)
    return np.ascontiguousarray(x), d, w


def coverage(x, b):
    """shares of the states with all three local coordinates exactly 0 on interior nodes, in clamped cells, and with a stencil
    that straddles cells at the smaller del_"""
    on_node = np.ones(x.shape[0], dtype=bool)
    for a in range(3):
        on_node &= np.isin(x[:, a], grid_nodes(b, GRID, a))
    straddle, clamped = shares(x, DELS[0], b, GRID)
    return {"on_node": float(on_node.mean()), "clamped": clamped, "straddle": straddle}


def low_coverage(cov):
    return ["%s %.4f" % (k, v) for k, v in sorted(cov.items()) if v < 0.01]


def compute(report=None):
    """-> {name: str digest or float64 array} for every case; needs the GPU.  report: a dict that receives coverage()."""
    from stanford_raytracer_amd import api, workloads as wl

    api.init(0)
    os.environ["SRT_WAVES_PER_CU"] = WAVES_PER_CU
    b, Fs = grids(wl)
    x, d, w = states(wl, b)
    if report is not None:
        report.update(coverage(x, b))
    k = d * (20.0 * w / C_LIGHT)[:, None]
    args = np.concatenate([x, k, w[:, None]], axis=1)
    out = {}
    try:
        for gname in sorted(Fs):
            for ns in (4, 2):
                m = api.Model.interp(np.ascontiguousarray(Fs[gname][..., :ns]), b, wl.QS[:ns], wl.MS[:ns])
                tag = "%s_ns%d" % (gname, ns)
                pp = m.plasma_params(x)
                out[tag + "_params"] = digest(pp)
                out[tag + "_params_sums"] = np.array([float(np.nansum(pp[:, 4:8])), float(np.isnan(pp).sum())])
                for del_ in DELS:
                    dtag = "%s_del%g" % (tag, del_)
                    rk = m.rk_step(args, np.full(x.shape[0], 0.05), del_)
                    gr = m.gradients(x, k, w, del_)
                    out[dtag + "_rkstep"] = digest(rk)
                    out[dtag + "_gradients"] = digest(gr)
                    out[dtag + "_layered_sums"] = np.array([float(np.nansum(rk)), float(np.nansum(gr))])
                    for fixed in (0, 1):
                        kw = dict(fixedstep=fixed, dt0=1e-3 if not fixed else 2e-3, dtmax=0.1, tmax=0.2, maxerr=5e-4,
                                  maxsteps=24, del_=del_, outputper=2)
                        rows, nrows, stop, steps = m.trace(x, d, w, **kw)
                        ttag = dtag + ("_rk4" if fixed else "_rkf45")
                        out[ttag + "_rows"] = digest(rows)
                        out[ttag + "_nrows"] = digest(nrows)
                        out[ttag + "_stop"] = digest(stop)
                        out[ttag + "_sums"] = np.array([float(steps), float(nrows.sum()), float(np.nansum(rows[:, :, 1:4]))])
                m.close()
    finally:
        os.environ.pop("SRT_WAVES_PER_CU", None)
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "horner_first_terms_golden.npz")
    report = {}
    out = compute(report)
    print("coverage of the states:", report)
    if low_coverage(report):
        raise SystemExit("a share below 1 %%: the cases do not exercise the path: %s" % low_coverage(report))
    for name in sorted(out):
        if name.endswith("_sums"):
            print(name, out[name])
    np.savez_compressed(path, **{name: (np.array(v) if isinstance(v, str) else v) for name, v in out.items()})
    print("wrote", path, len(out), "entries")


if __name__ == "__main__":
    main()
