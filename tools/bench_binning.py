#!/usr/bin/env python3
"""What binning traced rays onto a grid costs on the device (include/srt.h, srt_bin_rays_device).  config[2]'s launch set
(bench.py's interp256: 1 M rays, 256^3 grid, maxsteps 256, outputper 16) is traced once and packed (srt_pack_rows_device); then
the packed rows are binned onto
    a 64 x 48 (L, magnetic latitude) map     3072 cells: the block-private LDS copy, flushed once per block;
    the same map with a third axis of two z cells whose upper one holds nothing
                                             6144 cells: the SAME deposits through global atomics, the other accumulation path;
    a 128^3 (x, y, z) volume                 2 M cells: global atomics spread over many addresses,
with nsub 1 and 8, with and without row weights.  Timed with HIP events on the stream, one warm-up, then the median of
`--repeats`.  The call reads offsets[nrays] back once; that round trip is inside every figure.  The two forms of the map are
checked to hold the same integers.  A first measurement: it sets no bar.

    python tools/bench_binning.py [--repeats 5] [--rays 1000000] [--grid 256] [--out FILE]
"""
import numpy as np

import bench_rows_common as common


def main():
    a = common.parser().parse_args()
    s = common.traced_and_packed(a, "bench_binning.py")
    torch, api, parallel, wl, dev, st = s.torch, s.api, s.parallel, s.wl, s.dev, s.st
    packed, offsets, trace_ms, n, total = s.packed, s.offsets, s.trace_ms, s.n, s.total
    roww = torch.rand(max(total, 1), dtype=torch.float64, device=dev)

    le, lat = np.geomspace(1.0, 10.0, 65), np.deg2rad(np.linspace(-72.0, 72.0, 49))
    half = 10.0 * wl.R_E
    cube = np.linspace(-half, half, 129)
    grids = {"map 64x48 (L, maglat), LDS path": [api.axis("L", le), api.axis_maglat(lat)],
             "map 64x48x2 (L, maglat, z: upper cell empty), global atomics": [api.axis("L", le), api.axis_maglat(lat),
                                                                              api.axis("z", [-1e12, 1e12, 2e12])],
             "volume 128^3 (x, y, z), global atomics": [api.axis("x", cube), api.axis("y", cube), api.axis("z", cube)]}

    def timed(axes, nsub, weights):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(st)
        out = parallel.bin_rays_device(packed, offsets, axes, nsub, row_weight=roww if weights else None, stream=st)
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1), out

    runs, maps = [], {}
    for name, axes in grids.items():
        for nsub in (1, 8):
            for weights in (False, True):
                ms = []
                for _ in range(a.repeats + 1):
                    t, out = timed(axes, nsub, weights)
                    ms.append(t)
                ms = ms[1:]  # (the first call is the warm-up; its zeroing of the outputs is inside every figure)
                med = float(np.median(ms))
                ticks, hits, counters = (t_.cpu().numpy() for t_ in out)
                maps[(name, nsub, weights)] = (ticks, hits, counters)
                runs.append({"grid": name, "cells": int(ticks.size), "nsub": nsub, "row_weights": weights, "ms_median": round(med, 4),
                             "ms": [round(v, 4) for v in ms], "GBs_of_whole_rows": round(total * 160 / (med * 1e-3) / 1e9, 1),
                             "counters": counters.tolist(), "cells_hit": int(np.count_nonzero(hits)),
                             "seconds_binned": float(ticks.sum()) * 2.0 ** -30})
    names = list(grids)
    for nsub in (1, 8):
        for weights in (False, True):
            a2, b3 = maps[(names[0], nsub, weights)], maps[(names[1], nsub, weights)]
            assert np.array_equal(b3[0][0], a2[0]) and np.array_equal(b3[1][0], a2[1]) and np.array_equal(b3[2], a2[2]), "the two paths differ"
            assert not b3[0][1].any() and not b3[1][1].any()
    res = {"device": api.device_info()["name"], "repeats": a.repeats, "rays": n, "grid": a.grid, "maxsteps": 256, "outputper": 16,
           "packed_rows": total, "trace_kernel_ms": round(trace_ms, 3), "quantum": 2.0 ** -30, "runs": runs,
           "the_two_paths_hold_the_same_integers": True,
           "bytes": {"rows_whole": total * 160, "rows_t_pos_vgrel_only": total * 56, "offsets": (n + 1) * 8, "row_weights": total * 8},
           "note": "HIP-event time around parallel.bin_rays_device on the stream: the zeroing of the two maps and the counters, "
                   "srt_bin_rays_device with its 8-byte read of offsets[nrays] and its upload of the edges; a first measurement, no bar"}
    common.emit(res, a.out)


if __name__ == "__main__":
    main()
