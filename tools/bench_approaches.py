#!/usr/bin/env python3
"""What finding closest approaches to observer points costs on the device (include/srt.h, srt_approaches_device).  config[2]'s
launch set (bench.py's interp256: 1 M rays, 256^3 grid, maxsteps 256, outputper 16) is traced once and packed
(srt_pack_rows_device); the observers lie evenly on a circular track of radius 2.5 R_E, inclined 30 degrees to the SM equator,
each with a detection radius of 500 km.  For 1, 64, 1 024 and 16 384 observers: the count-only call (count pass + scan) and the
full call (count pass + scan + fill pass, which recounts the rows that have events) with room for every event, timed with HIP
events on the stream, one warm-up, then the median of `--repeats`.  The call copies the observers up and reads offsets[nrays] back
once; both are inside the figures.  Beside them, in the same run on the same rows: the crossings' count-only call on the four
surfaces of bench_crossings.py, which reads the same bytes as the one-observer call.  A first measurement: it sets no bar.

    python tools/bench_approaches.py [--repeats 5] [--rays 1000000] [--grid 256] [--observers 1,64,1024,16384] [--out FILE]
"""
import ctypes as C

import numpy as np

import bench_rows_common as common

MAX_EVENTS = 100_000_000  # room is made for at most this many events (18.4 GB)


def track(n, r_e):
    """n observers evenly on a circle of radius 2.5 R_E whose plane is the SM equator tilted by 30 degrees about the x axis"""
    a = 2.0 * np.pi * (np.arange(n) + 0.5) / n
    inc = np.deg2rad(30.0)
    r = 2.5 * r_e
    return np.stack([r * np.cos(a), r * np.sin(a) * np.cos(inc), r * np.sin(a) * np.sin(inc), np.full(n, 500e3)], axis=1)


def main():
    ap = common.parser()
    ap.add_argument("--observers", default="1,64,1024,16384")
    a = ap.parse_args()
    s = common.traced_and_packed(a, "bench_approaches.py")
    torch, api, wl, L, dev, st = s.torch, s.api, s.wl, s.L, s.dev, s.st
    packed, offsets, trace_ms, n, total = s.packed, s.offsets, s.trace_ms, s.n, s.total
    count = torch.zeros(1, dtype=torch.int64, device=dev)

    def timed(call):
        return common.timed(s, call)

    # the crossings' count pass on the same rows, in the same run
    surf, ns = api.surface_array(common.c5_surfaces(s))
    cx_ms = [timed(lambda: L.srt_crossings_device(ns, surf, n, offsets.data_ptr(), packed.data_ptr(), None, None, C.c_int64(0),
                                                  count.data_ptr(), st.cuda_stream)) for _ in range(a.repeats + 1)][1:]
    runs = []
    for nobs in [int(v) for v in a.observers.split(",")]:
        arr, no = api.observer_array(track(nobs, wl.R_E))

        def call(ev=None, meta=None, dist=None, cap=0):
            return L.srt_approaches_device(no, arr, n, offsets.data_ptr(), packed.data_ptr(), ev.data_ptr() if cap else None,
                                           meta.data_ptr() if cap else None, dist.data_ptr() if cap else None, C.c_int64(cap),
                                           count.data_ptr(), st.cuda_stream)

        count_ms = [timed(call) for _ in range(a.repeats + 1)][1:]
        nev = int(count.item())
        cap = max(min(nev, MAX_EVENTS), 1)
        ev = torch.zeros((cap, api.ROW), dtype=torch.float64, device=dev)
        meta = torch.zeros((cap, 4), dtype=torch.int32, device=dev)
        dist = torch.zeros(cap, dtype=torch.float64, device=dev)
        full_ms = [timed(lambda: call(ev, meta, dist, cap)) for _ in range(a.repeats + 1)][1:]
        assert int(count.item()) == nev
        k = min(nev, cap)
        mh = meta[:k].cpu().numpy().astype(np.int64)
        if k:
            key = (mh[:, 0] * (1 << 20) + mh[:, 2]) * (1 << 17) + mh[:, 1]
            assert np.all(np.diff(key) > 0), "events are not in (ray, interval, observer) order"
            assert bool(torch.isfinite(ev[:k]).all()) and bool((dist[:k] <= 500e3).all())
        runs.append({"observers": nobs, "pairs": (total - n) * nobs, "events": nev, "events_written": k,
                     "rays_with_events": int(len(np.unique(mh[:, 0]))), "observers_with_events": int(len(np.unique(mh[:, 1]))),
                     "count_only_ms_median": round(float(np.median(count_ms)), 4), "count_only_ms": [round(v, 4) for v in count_ms],
                     "count_and_fill_ms_median": round(float(np.median(full_ms)), 4), "count_and_fill_ms": [round(v, 4) for v in full_ms],
                     "count_only_ns_per_pair": round(float(np.median(count_ms)) * 1e6 / max((total - n) * nobs, 1), 5)})
        del ev, meta, dist
    res = {"device": api.device_info()["name"], "repeats": a.repeats, "rays": n, "grid": a.grid, "maxsteps": 256, "outputper": 16,
           "packed_rows": total, "track": "circle of 2.5 R_E inclined 30 deg, observers evenly spaced, radius 500 km",
           "trace_kernel_ms": round(trace_ms, 3), "runs": runs,
           "crossings_count_only_ms_median": round(float(np.median(cx_ms)), 4), "crossings_count_only_ms": [round(v, 4) for v in cx_ms],
           "note": "HIP-event time around srt_approaches_device on the stream, including its copy of the observers and its 8-byte "
                   "read of offsets[nrays]; pairs = intervals x observers; a first measurement, no bar"}
    common.emit(res, a.out)


if __name__ == "__main__":
    main()
