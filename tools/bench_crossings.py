#!/usr/bin/env python3
"""What locating surface crossings on the device costs (include/srt.h, srt_crossings_device).  config[2]'s launch set (bench.py's
interp256: 1 M rays, 256^3 grid, maxsteps 256, outputper 16) is traced once and packed (srt_pack_rows_device); then the four
surfaces of the tests' case C5 (sphere 1.3 R_E, magnetic equator, latitude 20 degrees, L = 2) are located on the packed rows.
Timed with HIP events on the stream, one warm-up, then the median of `--repeats`: the count-only call (count pass + scan) and the
full call (count pass + scan + fill pass) with room for every event.  The call reads offsets[nrays] back once to size its
launches; that round trip is inside both figures.  A first measurement: it sets no bar.

    python tools/bench_crossings.py [--repeats 5] [--rays 1000000] [--grid 256] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch  # before the library, as in bench.py

    if not torch.cuda.is_available():
        raise SystemExit("bench_crossings.py needs an MI355X (no CPU fallback)")
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
    surf = [api.sphere(1.3 * wl.R_E), api.maglat(0.0), api.maglat(np.deg2rad(20.0)), api.lshell(2.0)]
    arr, ns = api.surface_array(surf)
    L = api.lib()
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream(dev)

    def timed(ev, meta, cap):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        api._check(L.srt_crossings_device(ns, arr, n, offsets.data_ptr(), packed.data_ptr(), ev.data_ptr() if cap else None,
                                          meta.data_ptr() if cap else None, C.c_int64(cap), count.data_ptr(), st.cuda_stream))
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1)

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
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
