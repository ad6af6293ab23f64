"""What the bench tools of the packed-row post-processors share (bench_crossings.py, bench_approaches.py, bench_tubes.py,
bench_binning.py): the command line, config[2]'s launch set (bench.py's interp256: 1 M rays, 256^3 grid, maxsteps 256,
outputper 16) traced once and packed (srt_pack_rows_device), a HIP-event timer on the stream, the four surfaces of the tests'
case C5, and the one JSON line at the end."""
import argparse
import json
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--out", default=None)
    return ap


def traced_and_packed(a, tool):
    """-> the modules, the device and its stream, the model, and the packed rows of one trace of the launch set `a` asks for"""
    import torch  # before the library, as in bench.py

    if not torch.cuda.is_available():
        raise SystemExit("%s needs an MI355X (no CPU fallback)" % tool)
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
    return SimpleNamespace(torch=torch, api=api, parallel=parallel, wl=wl, dev=dev, st=torch.cuda.current_stream(dev), m=m, p=p,
                           batch=batch, packed=packed, offsets=offsets, trace_ms=m.last_kernel_ms(), n=len(w),
                           total=int(offsets[-1].item()), L=api.lib())


def timed(s, call):
    """HIP-event milliseconds around call() on the stream; call() answers the library's return code"""
    e0, e1 = s.torch.cuda.Event(enable_timing=True), s.torch.cuda.Event(enable_timing=True)
    e0.record(s.st)
    s.api._check(call())
    e1.record(s.st)
    e1.synchronize()
    return e0.elapsed_time(e1)


def c5_surfaces(s):
    """sphere 1.3 R_E, magnetic equator, latitude 20 degrees, L = 2"""
    import numpy as np

    return [s.api.sphere(1.3 * s.wl.R_E), s.api.maglat(0.0), s.api.maglat(np.deg2rad(20.0)), s.api.lshell(2.0)]


def emit(res, out):
    line = json.dumps(res)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")
