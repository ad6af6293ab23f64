#!/usr/bin/env python3
"""Kernel time of the interp model's trace kernel in both device layouts -- the expanded coefficient table and the node table
(include/srt.h, SRT_INTERP_*) -- on the headline's launch set and grid (BASELINE config[2]: 1 M rays, 256^3 x 4 species,
RKF45, maxsteps 256, outputper 16, launch-cell ray order: bench.py's interp256) in the same run.  HIP-event kernel time
(srt_last_kernel_ms), a warm-up launch, then the median of `--launches` launches; inputs and outputs resident in HBM
(DeviceBatch, the entry point bench.py times).  Prints one JSON line that also holds each layout's creation time and
device_bytes, and whether the two layouts' row counts and stop codes are equal.

    python tools/bench_interp_layout.py [--rays N] [--grid N] [--maxsteps M] [--launches 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

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
    nrows, stop = o["nrows"].cpu().numpy().copy(), o["stop"].cpu().numpy().copy()
    med = float(np.median(ms))
    return {"kernel_ms": [round(v, 3) for v in ms], "kernel_ms_median": round(med, 3), "accepted_steps": steps,
            "steps_per_s": round(steps / (med * 1e-3), 1), "stop_histogram": np.bincount(stop, minlength=10).tolist()}, nrows, stop


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--maxsteps", type=int, default=256)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch  # before the library, as in bench.py: torch brings up its own HIP runtime first

    if not torch.cuda.is_available():
        raise SystemExit("bench_interp_layout.py needs an MI355X (no CPU fallback)")
    torch.cuda.set_device(0)
    from stanford_raytracer_amd import api, workloads as wl

    api.init(0)
    trace = dict(fixedstep=0, dt0=1e-3, dtmax=0.1, maxerr=5e-4, tmax=0.5, root=2, maxsteps=a.maxsteps, outputper=16, del_=1e-6,
                 ray_order=1)
    p = api.make_params(minalt=wl.MINALT, **trace)
    rays = wl.launch_set(a.rays, 3)
    F, bounds = wl.make_grid(a.grid, half_width=10.0 * wl.R_E)
    res = {"workload": "interp256" if (a.grid, a.rays, a.maxsteps) == (256, 1_000_000, 256) else "interp", "grid": a.grid,
           "rays": int(len(rays[2])), "device": api.device_info()["name"], "trace": trace}
    outs = {}
    for layout in ("expanded", "nodes"):
        t0 = time.time()
        model = api.Model.interp(F, bounds, wl.QS, wl.MS, layout=layout)
        create_s = time.time() - t0
        r, nrows, stop = time_model(model, p, rays, a.launches)
        r.update(create_s=round(create_s, 3), device_bytes=int(model.device_bytes))
        res[layout], outs[layout] = r, (nrows, stop)
        model.close()
    e, n = res["expanded"], res["nodes"]
    res["nodes_over_expanded_ms_per_step"] = round((n["kernel_ms_median"] / n["accepted_steps"]) / (e["kernel_ms_median"] / e["accepted_steps"]), 3)
    res["expanded_over_nodes_bytes"] = round(e["device_bytes"] / n["device_bytes"], 3)
    res["row_counts_equal"] = bool(np.array_equal(outs["expanded"][0], outs["nodes"][0]))
    res["stop_codes_equal"] = bool(np.array_equal(outs["expanded"][1], outs["nodes"][1]))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
