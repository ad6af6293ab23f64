#!/usr/bin/env python3
"""Kernel time of the trace kernel of modelnum 6 (simple3d), 5 (ngo3d) or 7 (at64thch) on its workloads.py launch set
(config[1]'s 100 k rays, Kp 4), and of the Ngo kernel on the same rays with the same integrator settings in the same run (the Ngo
kernel with its own FD step, the driver's delSP).  HIP-event kernel time (srt_last_kernel_ms), `--launches` launches after a
warm-up; inputs and outputs resident in HBM (DeviceBatch, the entry point bench.py times).  Prints one JSON line.

--maxsteps cuts every ray off after that many rows (both kernels); the result line says which maxsteps it was taken with.  It
is there for at64thch: a wave's attempt costs 43 density evaluations of 64 field-line traces each, in the order of a second,
and a launch lasts as long as its longest ray, so a first figure per wave-step can be had in seconds only that way.

    python tools/bench_model.py --model {simple3d,ngo3d,at64thch} [--rays N] [--maxsteps M] [--launches 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

# model -> (its workloads.py dict, constructor(api, W, card file), digits of the ratio to the Ngo kernel); the card file is
# the one the Ngo kernel of the comparison is created from
MODELS = {
    "simple3d": ("SIMPLE3D_100K", lambda api, W, cfg: api.Model.simple3d(W["kp"], yearday=W["yearday"], msec=W["msec"], fixed_mlt=W["fixed_mlt"]), 3),
    "ngo3d": ("NGO3D_100K", lambda api, W, cfg: api.Model.ngo3d(cfg, W["kp"], yearday=W["yearday"], msec=W["msec"], fixed_mlt=W["fixed_mlt"]), 3),
    "at64thch": ("AT64THCH_100K", lambda api, W, cfg: api.Model.at64thch(W["gcpm_kp"], W["parmod"], yearday=W["yearday"], msec=W["msec"]), 1),
}


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
    ap.add_argument("--model", required=True, choices=sorted(MODELS))
    ap.add_argument("--rays", type=int, default=None)
    ap.add_argument("--maxsteps", type=int, default=None)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch  # before the library, as in bench.py: torch brings up its own HIP runtime first

    if not torch.cuda.is_available():
        raise SystemExit("bench_model.py needs an MI355X (no CPU fallback)")
    torch.cuda.set_device(0)
    from stanford_raytracer_amd import api, workloads as wl

    api.init(0)
    name = a.model
    wname, make, digits = MODELS[name]
    W = getattr(wl, wname)
    rays = wl.model_launch_set(W, a.rays)
    trace = dict(W["trace"])
    if a.maxsteps:
        trace["maxsteps"] = a.maxsteps
    res = {"workload": wname.lower(), "rays": int(len(rays[2])), "device": api.device_info()["name"], "trace": trace}
    with tempfile.TemporaryDirectory() as d:
        cfg = os.path.join(d, "newray.in")
        with open(cfg, "w") as f:
            f.write(W.get("newray", wl.NEWRAY_PLASMAPAUSE))
        model = make(api, W, cfg)
        ngo = api.Model.ngo(cfg, W["yearday"], W["msec"])  # config[1]'s model on the same rays
    res[name] = time_model(model, api.make_params(minalt=wl.MINALT, **trace), rays, a.launches)
    res["ngo_same_rays"] = time_model(ngo, api.make_params(minalt=wl.MINALT, **dict(trace, del_=1e-4)), rays, a.launches)
    res[name + "_over_ngo_ms_per_step"] = round((res[name]["kernel_ms_median"] / res[name]["accepted_steps"]) /
                                                (res["ngo_same_rays"]["kernel_ms_median"] / res["ngo_same_rays"]["accepted_steps"]), digits)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
