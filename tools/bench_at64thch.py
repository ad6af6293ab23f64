#!/usr/bin/env python3
"""Kernel time of the modelnum-7 trace kernel (AT64ThCh: one field-line trace per evaluated point) on its workloads.py launch
set (config[1]'s 100 k rays, Kp 4), and of the Ngo kernel on the same rays with the same integrator settings in the same run.
HIP-event kernel time (srt_last_kernel_ms), `--launches` launches after a warm-up; inputs and outputs resident in HBM
(DeviceBatch, the entry point bench.py times).  Prints one JSON line.

A wave's attempt costs 43 density evaluations of 64 field-line traces each, in the order of a second, and a launch lasts as long
as its longest ray: --maxsteps cuts every ray off after that many rows (both models), so that a first figure per wave-step can
be had in seconds; the result line says which maxsteps it was taken with.

    python tools/bench_at64thch.py [--rays N] [--maxsteps M] [--launches 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def time_model(model, p, rays, launches):
    import torch
    from stanford_raytracer_amd.device_batch import DeviceBatch

    b = DeviceBatch(model, p, *rays, device=torch.device("cuda:0"))
    ms, steps = [], 0
    for k in range(launches + 1):  # launch 0 warms up
        o = b.launch()
        torch.cuda.synchronize()
        if k:
            ms.append(model.last_kernel_ms())
            steps = int(o["cnt"][1].item())
    stop = np.bincount(o["stop"].cpu().numpy(), minlength=10).tolist()
    med = float(np.median(ms))
    return {"kernel_ms": [round(v, 3) for v in ms], "kernel_ms_median": round(med, 3), "accepted_steps": steps,
            "steps_per_s": round(steps / (med * 1e-3), 1), "stop_histogram": stop}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=None)
    ap.add_argument("--maxsteps", type=int, default=None)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch  # before the library, as in bench.py: torch brings up its own HIP runtime first

    if not torch.cuda.is_available():
        raise SystemExit("bench_at64thch.py needs an MI355X (no CPU fallback)")
    torch.cuda.set_device(0)
    from stanford_raytracer_amd import api, workloads as wl

    api.init(0)
    W = wl.AT64THCH_100K
    rays = wl.at64thch_launch_set(a.rays)
    trace = dict(W["trace"])
    if a.maxsteps:
        trace["maxsteps"] = a.maxsteps
    res = {"workload": "at64thch_100k", "rays": int(len(rays[2])), "device": api.device_info()["name"], "trace": trace}
    p = api.make_params(minalt=wl.MINALT, **trace)
    m7 = api.Model.at64thch(W["gcpm_kp"], W["parmod"], yearday=W["yearday"], msec=W["msec"])
    with tempfile.TemporaryDirectory() as d:
        cfg = os.path.join(d, "newray.in")
        with open(cfg, "w") as f:
            f.write(wl.NEWRAY_PLASMAPAUSE)
        ngo = api.Model.ngo(cfg, W["yearday"], W["msec"])  # config[1]'s model on the same rays
    res["at64thch"] = time_model(m7, p, rays, a.launches)
    res["ngo_same_rays"] = time_model(ngo, p, rays, a.launches)
    res["at64thch_over_ngo_ms_per_step"] = round((res["at64thch"]["kernel_ms_median"] / res["at64thch"]["accepted_steps"]) /
                                                 (res["ngo_same_rays"]["kernel_ms_median"] / res["ngo_same_rays"]["accepted_steps"]), 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
