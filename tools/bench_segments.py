#!/usr/bin/env python3
"""What the trace in segments (include/srt.h) costs and what it buys.  One call; every figure is the median of `--repeats` runs
after one warm-up; per launch the HIP-event time (srt_last_kernel_ms), per run the wall clock.  First measurements: no bar.

(a) headline overhead: config[2]'s launch set (bench.py's interp256: 1 M rays, 256^3 grid, maxsteps 256, outputper 16 = 16
    slots) on device-resident buffers, unsegmented (srt_trace_batch_device) against srt_trace_segment_device with N = 16 (one
    segment: the pause test alone) and N = 4 (four segments: the state traffic and the compaction between them).
(b) long-ray throughput: config[1]'s Ngo rays at maxsteps 4096, outputper 1 through the executable, with its chunking of
    today (2 GiB of rows per launch = 3 276 rays) and with --segment_rows=64: accepted steps per second of wall clock and
    the peak resident host bytes of the process, both sides in this one run.

    python tools/bench_segments.py [--repeats 5] [--rays-a 1000000] [--rays-b 100000] [--skip a|b] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def med(v):
    return round(float(np.median(v)), 3)


def part_a(api, wl, torch, rays, grid, repeats):
    dev = torch.device("cuda:0")
    L = api.lib()
    F, bounds = wl.make_grid(grid, half_width=10.0 * wl.R_E)
    m = api.Model.interp(F, bounds, wl.QS, wl.MS)
    del F
    p = api.make_params(fixedstep=0, dt0=1e-3, dtmax=0.1, maxerr=5e-4, tmax=0.5, root=2, minalt=wl.MINALT, maxsteps=256,
                        outputper=16, del_=1e-6, ray_order=1)
    slots = L.srt_rows_per_ray(C.byref(p))
    pos, d, w = wl.launch_set(rays, 3)
    n = len(w)
    d_pos = torch.from_numpy(np.ascontiguousarray(pos.T)).to(dev)
    d_dir = torch.from_numpy(np.ascontiguousarray(d.T)).to(dev)
    d_w = torch.from_numpy(np.ascontiguousarray(w)).to(dev)
    rows = torch.zeros((n, slots, api.ROW), dtype=torch.float64, device=dev)
    nrows = torch.zeros(n, dtype=torch.int32, device=dev)
    stop = torch.zeros(n, dtype=torch.int32, device=dev)
    cnt = torch.zeros(4, dtype=torch.int64, device=dev)
    state = torch.zeros((n, api.STATE), dtype=torch.float64, device=dev)
    queue = torch.zeros(n, dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)

    def unsegmented():
        api._check(L.srt_trace_batch_device(m.h, C.byref(p), n, d_pos.data_ptr(), d_dir.data_ptr(), d_w.data_ptr(), rows.data_ptr(),
                                            nrows.data_ptr(), stop.data_ptr(), cnt.data_ptr(), None))
        torch.cuda.synchronize()
        return [m.last_kernel_ms()], int(cnt.cpu()[1])

    def segmented(N):
        ms, steps, nq = [], 0, n
        for s in range(api.trace_segment_count(p, N)):
            if nq == 0:
                break
            api._check(L.srt_trace_segment_device(m.h, C.byref(p), n, d_pos.data_ptr(), d_dir.data_ptr(), d_w.data_ptr(), N, s,
                                                  queue.data_ptr() if s else None, nq, state.data_ptr(), rows.data_ptr(),
                                                  nrows.data_ptr(), stop.data_ptr(), cnt.data_ptr(), None))
            api._check(L.srt_running_rays_device(n, stop.data_ptr(), queue.data_ptr(), count.data_ptr(), None))
            nq = int(count.cpu()[0])  # (synchronises: the host decides whether there is another segment)
            ms.append(m.last_kernel_ms())
            steps += int(cnt.cpu()[1])
        return ms, steps

    out = {"rays": n, "grid": grid, "maxsteps": 256, "outputper": 16, "slots": slots}
    for tag, fn in (("unsegmented", unsegmented), ("segment_rows_16", lambda: segmented(16)), ("segment_rows_4", lambda: segmented(4))):
        kernel, wall, launches, steps = [], [], None, None
        for k in range(repeats + 1):  # pass 0 warms up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ms, steps = fn()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if k:
                kernel.append(sum(ms))
                wall.append((t1 - t0) * 1e3)
                launches = [round(v, 3) for v in ms]
        out[tag] = {"kernel_ms_median": med(kernel), "wall_ms_median": med(wall), "kernel_ms": [round(v, 3) for v in kernel],
                    "launch_ms_last_run": launches, "accepted_steps": steps}
    base = out["unsegmented"]["kernel_ms_median"]
    for tag in ("segment_rows_16", "segment_rows_4"):
        out[tag]["kernel_vs_unsegmented"] = round(out[tag]["kernel_ms_median"] / base, 4)
        assert out[tag]["accepted_steps"] == out["unsegmented"]["accepted_steps"], "the segments' steps do not sum to the launch's"
    return out


def part_b(wl, rays, repeats, tmp):
    exe = os.path.join(ROOT, "stanford_raytracer_amd", "bin", "raytracer")
    cfg, rf = os.path.join(tmp, "newray.in"), os.path.join(tmp, "rays.txt")
    with open(cfg, "w") as f:
        f.write(wl.NEWRAY_PLASMAPAUSE)
    pos, d, w = wl.launch_set(rays, 2)
    wl.write_rays_file(rf, pos, d, w)
    base = [exe, "--outputper=1", "--dt0=0.001", "--dtmax=0.1", "--tmax=0.5", "--root=2", "--fixedstep=0", "--maxerr=5e-4",
            "--maxsteps=4096", "--minalt=%r" % wl.MINALT, "--inputraysfile=%s" % rf, "--modelnum=1", "--ngo_configfile=%s" % cfg,
            "--yearday=2010001", "--milliseconds_day=0", "--first_attempt_policy=0", "--timing=1"]
    out = {"rays": rays, "maxsteps": 4096, "outputper": 1}
    sizes = {}
    for tag, extra in (("chunked_2GiB", []), ("segment_rows_64", ["--segment_rows=64"])):
        wall, rss, steps, timing = [], [], None, None
        for k in range(repeats + 1):
            o = os.path.join(tmp, tag + ".ray")
            t0 = time.perf_counter()
            # (a child of its own per run: its peak resident set is read from wait4)
            pr = subprocess.Popen(base + ["--outputfile=%s" % o] + extra, stdout=subprocess.PIPE, text=True)
            text = pr.stdout.read()
            _, status, ru = os.wait4(pr.pid, 0)
            pr.returncode = os.waitstatus_to_exitcode(status)
            t1 = time.perf_counter()
            if pr.returncode != 0:
                raise SystemExit("%s: the executable ended with %d" % (tag, pr.returncode))
            steps = int(re.search(r"(\d+) accepted steps", text).group(1))
            timing = json.loads(re.search(r"timing: (\{.*\})", text).group(1))
            sizes[tag] = os.path.getsize(o)
            if k:
                wall.append(t1 - t0)
                rss.append(ru.ru_maxrss * 1024)
        out[tag] = {"wall_s_median": med(wall), "accepted_steps": steps, "steps_per_s": round(steps / float(np.median(wall)), 1),
                    "peak_host_bytes": int(max(rss)), "phases_last_run": timing, "ray_file_bytes": sizes[tag]}
    same = subprocess.run(["cmp", "-s", os.path.join(tmp, "chunked_2GiB.ray"), os.path.join(tmp, "segment_rows_64.ray")]).returncode == 0
    out["same_ray_file"] = bool(same)
    out["speedup_wall"] = round(out["chunked_2GiB"]["wall_s_median"] / out["segment_rows_64"]["wall_s_median"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rays-a", type=int, default=1_000_000)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--rays-b", type=int, default=100_000)
    ap.add_argument("--skip", default="", choices=["", "a", "b"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch  # before the library, as in bench.py

    if not torch.cuda.is_available():
        raise SystemExit("bench_segments.py needs an MI355X (no CPU fallback)")
    from stanford_raytracer_amd import api, workloads as wl

    api.init(0)
    res = {"device": api.device_info()["name"], "repeats": a.repeats}
    if a.skip != "a":
        res["a_headline_overhead"] = part_a(api, wl, torch, a.rays_a, a.grid, a.repeats)
    if a.skip != "b":
        with tempfile.TemporaryDirectory() as tmp:
            res["b_long_rays"] = part_b(wl, a.rays_b, a.repeats, tmp)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
