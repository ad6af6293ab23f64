#!/usr/bin/env python3
"""What the ray-tube sections cost on the device (include/srt.h, srt_tubes_device).  config[2]'s launch set (bench.py's interp256:
1 M rays, 256^3 grid, maxsteps 256, outputper 16) is traced once and packed (srt_pack_rows_device); the neighbours of ray r are
r + 1 and r + 2, the last two rays without a tube.  The call -- its copy of the neighbours, its 8-byte read of offsets[nrays], its
one pass over the packed rows, two searches in the neighbours' times per row -- is timed with HIP events on the stream, one
warm-up, then the median of `--repeats`.  Beside it, in the same run on the same rows: the crossings' count-only call on the four
surfaces of bench_crossings.py.  A first measurement: it sets no bar.

    python tools/bench_tubes.py [--repeats 5] [--rays 1000000] [--grid 256] [--out FILE]
"""
import ctypes as C

import numpy as np

import bench_rows_common as common


def main():
    a = common.parser().parse_args()
    s = common.traced_and_packed(a, "bench_tubes.py")
    torch, api, L, dev, st = s.torch, s.api, s.L, s.dev, s.st
    packed, offsets, trace_ms, n, total = s.packed, s.offsets, s.trace_ms, s.n, s.total
    count = torch.zeros(1, dtype=torch.int64, device=dev)

    def timed(call):
        return common.timed(s, call)

    # the crossings' count pass on the same rows, in the same run
    surf, ns = api.surface_array(common.c5_surfaces(s))
    cx_ms = [timed(lambda: L.srt_crossings_device(ns, surf, n, offsets.data_ptr(), packed.data_ptr(), None, None, C.c_int64(0),
                                                  count.data_ptr(), st.cuda_stream)) for _ in range(a.repeats + 1)][1:]
    nb = np.full((n, 2), -1, dtype=np.int64)
    if n >= 3:
        nb[:n - 2, 0] = np.arange(n - 2) + 1
        nb[:n - 2, 1] = np.arange(n - 2) + 2
    pnb = nb.ctypes.data_as(C.POINTER(C.c_int64))
    section = torch.full((max(total, 1), 4), float("nan"), dtype=torch.float64, device=dev)
    flag = torch.ones(max(total, 1), dtype=torch.int32, device=dev)
    tb_ms = [timed(lambda: L.srt_tubes_device(n, pnb, offsets.data_ptr(), packed.data_ptr(), section.data_ptr(), flag.data_ptr(),
                                              st.cuda_stream)) for _ in range(a.repeats + 1)][1:]
    flags = torch.bincount(flag[:total].to(torch.int64), minlength=6).cpu().numpy()
    ok = flag[:total] == 0
    assert bool(torch.isfinite(section[:total][ok]).all()) and int(flags[0]) > 0
    # the rows of the last two rays have no tube; every other row has a flag of its own
    off_h = offsets.cpu().numpy()
    assert int(flags[1]) == int(off_h[n] - off_h[max(n - 2, 0)])
    med = float(np.median(tb_ms))
    res = {"device": api.device_info()["name"], "repeats": a.repeats, "rays": n, "grid": a.grid, "maxsteps": 256, "outputper": 16,
           "packed_rows": total, "neighbours": "ray r: r + 1 and r + 2; the last two rays have no tube",
           "trace_kernel_ms": round(trace_ms, 3),
           "tubes_ms_median": round(med, 4), "tubes_ms": [round(v, 4) for v in tb_ms],
           "tubes_ns_per_row": round(med * 1e6 / max(total, 1), 4),
           "flags": {str(k): int(v) for k, v in enumerate(flags[:6])},
           "crossings_count_only_ms_median": round(float(np.median(cx_ms)), 4), "crossings_count_only_ms": [round(v, 4) for v in cx_ms],
           "note": "HIP-event time around srt_tubes_device on the stream, including its copy of the neighbours and its 8-byte read "
                   "of offsets[nrays]; a first measurement, no bar"}
    common.emit(res, a.out)


if __name__ == "__main__":
    main()
