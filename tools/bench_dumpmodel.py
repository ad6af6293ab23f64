#!/usr/bin/env python3
"""Time of a dump (Model.dump, the reference's dumpmodel on the device) and of its file: per case the HIP-event time of the dump's
launches (srt_last_kernel_ms), the wall clock of the whole call (allocation, launches, the copy to the host) and of
write_dump_file, each `--repeats` times after one warm-up.  The cases are the slices a user plots: a 512 x 1 x 512 meridian plane
of models 1 and 6, and a 64 x 1 x 64 one of model 7, whose every node is a field-line trace.  A first measurement; it sets no
bar.  Prints one JSON line.

    python tools/bench_dumpmodel.py [--repeats 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def time_case(api, model, n, bounds, repeats, path, mag=False):
    kernel, call, write = [], [], []
    for k in range(repeats + 1):  # pass 0 warms up
        t0 = time.perf_counter()
        f = model.dump(n[0], n[1], n[2], bounds, mag_coords=mag)
        t1 = time.perf_counter()
        api.write_dump_file(path, f, bounds)
        t2 = time.perf_counter()
        if k:
            kernel.append(model.last_kernel_ms())
            call.append((t1 - t0) * 1e3)
            write.append((t2 - t1) * 1e3)
    med = lambda v: round(float(np.median(v)), 3)  # noqa: E731
    return {"nodes": int(n[0] * n[1] * n[2]), "shape": list(n), "mag_coords": bool(mag), "kernel_ms": [round(v, 3) for v in kernel],
            "kernel_ms_median": med(kernel), "dump_call_ms_median": med(call), "file_write_ms_median": med(write),
            "end_to_end_ms_median": med(np.array(call) + np.array(write)), "file_bytes": os.path.getsize(path),
            "all_finite": bool(np.all(np.isfinite(f)))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch  # before the library, as in bench.py: torch brings up its own HIP runtime first

    if not torch.cuda.is_available():
        raise SystemExit("bench_dumpmodel.py needs an MI355X (no CPU fallback)")
    from stanford_raytracer_amd import api, workloads as wl

    api.init(0)
    R = wl.R_E
    plane = np.array([1.2, 6.0, 0.0, 0.0, -2.5, 2.5]) * R
    res = {"device": api.device_info()["name"], "repeats": a.repeats}
    with tempfile.TemporaryDirectory() as d:
        cfg, out = os.path.join(d, "newray.in"), os.path.join(d, "dump.txt")
        with open(cfg, "w") as f:
            f.write(wl.NEWRAY_PLASMAPAUSE)
        res["ngo_512x1x512"] = time_case(api, api.Model.ngo(cfg), (512, 1, 512), plane, a.repeats, out)
        m6 = api.Model.simple3d(4.0)
        res["simple3d_512x1x512"] = time_case(api, m6, (512, 1, 512), plane, a.repeats, out)
        res["simple3d_mag_512x1x512"] = time_case(api, m6, (512, 1, 512), plane, a.repeats, out, mag=True)
        W = wl.AT64THCH_100K
        m7 = api.Model.at64thch(W["gcpm_kp"], W["parmod"], yearday=W["yearday"], msec=W["msec"])
        res["at64thch_64x1x64"] = time_case(api, m7, (64, 1, 64), plane, min(a.repeats, 2), out)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
