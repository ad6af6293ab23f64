"""The launches of tests/test_gpu_tail_stash.py, shared with tests/golden/make_tail_stash_golden.py (which records their digests
with the library of the commit BEFORE the tail stash: a ray's rows, row count, stop code and the launch's accepted steps and
attempts do not depend on how many waves a launch has or on the order in which they take the rays, so that library needs none
of the switches below).

600 rays of the seeded launch set on a 24^3 grid over +-5 R_E, maxsteps 64 (marks at 32, 48, 56, 60), outputper 4.  Under
SRT_MAX_BLOCKS=2 that is 4.7 rays per lane."""
import hashlib
import os

import numpy as np

NRAYS, SEED, GRID, HALF_WIDTH_RE = 600, 31, 24, 5.0
TRACE = dict(fixedstep=0, dt0=1e-3, dtmax=0.1, maxerr=5e-4, tmax=0.2, maxsteps=64, outputper=4, del_=1e-6)
MARKS = (32, 48, 56, 60)

# name -> (model, params on top of TRACE, environment on top of SRT_MAX_BLOCKS=2)
CASES = {
    "adaptive": ("interp4", {}, {}),
    "fixed": ("interp4", dict(fixedstep=1), {}),
    "morton": ("interp4", dict(ray_order=1), {}),
    "policy1": ("interp4", dict(first_attempt_policy=1), {}),
    "nspec1": ("interp1", {}, {}),
    "nodes": ("nodes4", {}, {}),
    "nodes_fixed": ("nodes4", dict(fixedstep=1), {}),
    "igrf": ("interp4_igrf", {}, {}),
    "threshold8": ("interp4", dict(refill_threshold=8), {}),
    "wavecap8": ("interp4", {}, {"SRT_WAVE_CAP": "8"}),
}
# same launches as "adaptive", hence its digests
SAME_AS_ADAPTIVE = {"off": {"SRT_TAIL_STASH": "0"}, "quota1": {"SRT_TAIL_STASH": "1"}}


def rays():
    from stanford_raytracer_amd import workloads as wl

    return wl.launch_set(NRAYS, SEED)


def make_model(kind):
    from stanford_raytracer_amd import api, workloads as wl

    F, b = wl.make_grid(GRID, half_width=HALF_WIDTH_RE * wl.R_E)
    if kind == "interp1":
        return api.Model.interp(F[..., :1], b, wl.QS[:1], wl.MS[:1])
    m = api.Model.interp(F, b, wl.QS, wl.MS, layout="nodes" if kind == "nodes4" else "expanded")
    if kind == "interp4_igrf":
        m.set_field(use_igrf=1)
    return m


class Env:
    """environment variables for the length of a `with` block (the library reads its switches at every launch)"""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def launch(model, params, pos, d, w, device="cuda:0"):
    """one unsegmented device launch -> rows, nrows, stop, counters (numpy)"""
    import torch

    from stanford_raytracer_amd.device_batch import DeviceBatch

    b = DeviceBatch(model, params, pos, d, w, device)
    o = b.launch()
    torch.cuda.synchronize()
    return tuple(o[k].cpu().numpy() for k in ("rows", "nrows", "stop", "cnt"))


def digests(rows, nrows, stop, cnt):
    h = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    return {"rows": h(rows.astype(np.float64)), "nrows": h(nrows.astype(np.int32)), "stop": h(stop.astype(np.int32)),
            "accepted": int(cnt[1]), "attempts": int(cnt[2])}
