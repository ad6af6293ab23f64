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
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

MAX_EVENTS = 100_000_000  # room is made for at most this many events (18.4 GB)


def track(n, r_e):
    """n observers evenly on a circle of radius 2.5 R_E whose plane is the SM equator tilted by 30 degrees about the x axis"""
    a = 2.0 * np.pi * (np.arange(n) + 0.5) / n
    inc = np.deg2rad(30.0)
    r = 2.5 * r_e
    return np.stack([r * np.cos(a), r * np.sin(a) * np.cos(inc), r * np.sin(a) * np.sin(inc), np.full(n, 500e3)], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--observers", default="1,64,1024,16384")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch  # before the library, as in bench.py

    if not torch.cuda.is_available():
        raise SystemExit("bench_approaches.py needs an MI355X (no CPU fallback)")
    from stanford_raytracer_amd import api, parallel, workloads as wl
    from stanford_raytracer_amd.device_batch import DeviceBatch

    api.init(0)
    dev = torch.device("cuda:0")
    F, bounds = wl.make_grid(a.grid, half_width=10.0 * wl.R_E)
    m = api.Model.interp(F, bounds, wl.QS, wl.MS)
    del F
    p = api.make_params(fixedstep=0, dt0=1e-3, dtmax=0.1, maxerr=5e-4, tmax=0.5, root=2, minalt=wl.MINALT, maxsteps=256,
                        outputper=16, del_=1e-6, ray_order=1)
    pos, d, w = wl.launch_set(a.rays, 3)
    batch = DeviceBatch(m, p, pos, d, w, dev)
    o = batch.launch()
    packed, offsets = parallel.pack_rows_device(o["rows"], o["nrows"], p.outputper)
    torch.cuda.synchronize()
    trace_ms = m.last_kernel_ms()
    n = len(w)
    total = int(offsets[-1].item())
    L = api.lib()
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream(dev)

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        api._check(call())
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1)

    # the crossings' count pass on the same rows, in the same run
    surf, ns = api.surface_array([api.sphere(1.3 * wl.R_E), api.maglat(0.0), api.maglat(np.deg2rad(20.0)), api.lshell(2.0)])
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
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
