#!/usr/bin/env python3
"""What locating surface crossings on the device costs (include/srt.h, srt_crossings_device).  config[2]'s launch set (bench.py's
interp256: 1 M rays, 256^3 grid, maxsteps 256, outputper 16) is traced once and packed (srt_pack_rows_device); then the four
surfaces of the tests' case C5 (sphere 1.3 R_E, magnetic equator, latitude 20 degrees, L = 2) are located on the packed rows.
Timed with HIP events on the stream, one warm-up, then the median of `--repeats`: the count-only call (count pass + scan) and the
full call (count pass + scan + fill pass) with room for every event.  The call reads offsets[nrays] back once to size its
launches; that round trip is inside both figures.  A first measurement: it sets no bar.

    python tools/bench_crossings.py [--repeats 5] [--rays 1000000] [--grid 256] [--out FILE]
"""
import ctypes as C

import numpy as np

import bench_rows_common as common


def main():
    a = common.parser().parse_args()
    s = common.traced_and_packed(a, "bench_crossings.py")
    torch, api, L, dev, st = s.torch, s.api, s.L, s.dev, s.st
    packed, offsets, trace_ms, n, total = s.packed, s.offsets, s.trace_ms, s.n, s.total
    arr, ns = api.surface_array(common.c5_surfaces(s))
    count = torch.zeros(1, dtype=torch.int64, device=dev)

    def timed(ev, meta, cap):
        return common.timed(s, lambda: L.srt_crossings_device(ns, arr, n, offsets.data_ptr(), packed.data_ptr(), ev.data_ptr() if cap else None,
                                                              meta.data_ptr() if cap else None, C.c_int64(cap), count.data_ptr(), st.cuda_stream))

    count_ms = [timed(None, None, 0) for _ in range(a.repeats + 1)][1:]
    nev = int(count.item())
    ev = torch.zeros((max(nev, 1), api.ROW), dtype=torch.float64, device=dev)
    meta = torch.zeros((max(nev, 1), 4), dtype=torch.int32, device=dev)
    full_ms = [timed(ev, meta, max(nev, 1)) for _ in range(a.repeats + 1)][1:]
    assert int(count.item()) == nev
    mh = meta[:nev].cpu().numpy()
    per_surface = [int(np.sum(mh[:, 1] == s)) for s in range(ns)]
    key = mh[:, 0].astype(np.int64) * (1 << 32) + mh[:, 2].astype(np.int64) * 16 + mh[:, 1]
    assert np.all(np.diff(key) > 0), "events are not in (ray, interval, surface) order"
    assert bool(torch.isfinite(ev[:nev]).all())
    res = {"device": api.device_info()["name"], "repeats": a.repeats, "rays": n, "grid": a.grid, "maxsteps": 256, "outputper": 16,
           "packed_rows": total, "surfaces": ["sphere 1.3 R_E", "maglat 0", "maglat 20 deg", "L = 2"], "events": nev,
           "events_per_surface": per_surface, "trace_kernel_ms": round(trace_ms, 3),
           "count_only_ms_median": round(float(np.median(count_ms)), 4), "count_only_ms": [round(v, 4) for v in count_ms],
           "count_and_fill_ms_median": round(float(np.median(full_ms)), 4), "count_and_fill_ms": [round(v, 4) for v in full_ms],
           "bytes": {"rows_whole": total * 160, "rows_t_pos_vgrel_only": total * 56, "offsets": (n + 1) * 8,
                     "mask_written_then_read_twice": total * 2, "event_offsets_written_then_read": (total + 1) * 8,
                     "fill_reads_rows_with_events": "two whole rows per row whose mask is not zero: at most %d" % (2 * 160 * nev),
                     "events_written": nev * (160 + 16)},
           "note": "HIP-event time around srt_crossings_device on the stream, including its 8-byte read of offsets[nrays]; "
                   "a first measurement, no bar"}
    res["count_only_GBs_of_whole_rows"] = round(total * 160 / (res["count_only_ms_median"] * 1e-3) / 1e9, 1)
    common.emit(res, a.out)


if __name__ == "__main__":
    main()
