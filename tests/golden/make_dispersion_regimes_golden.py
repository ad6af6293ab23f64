#!/usr/bin/env python3
"""tests/golden/dispersion_regimes_golden.npz: the REFERENCE's dispersion solver and handedness test across plasma regimes, on
the rows tests/dispersion_regimes.py builds (uniform-density modelnum-3 grids from 1e6 to 1e12 m^-3 and one with every density
zero; wave normals along, across, and within 1e-8 rad of B0; VLF to HF; on- and off-surface handedness tuples).

Needs oracle/_ref/ref_harness (python oracle/build_ref.py).  Rows on which the reference stops (cos^2 rounded above 1 -> NaN into
its SVD) are recorded as such (NaN outputs, `<key>_<family>_stopped`), never dropped: the run resumes behind each of them.

    python tests/golden/make_dispersion_regimes_golden.py
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dispersion_regimes as dr  # noqa: E402
from oracle import oracle, refharness  # noqa: E402
from stanford_raytracer_amd import workloads as wl  # noqa: E402

ZERO_RUN = dict(fixedstep=1, dt0=1e-3, dtmax=0.1, tmax=1.0, maxerr=5e-4, maxsteps=10, minalt=wl.MINALT, root=2)
ZERO_DEL = 1e-6


def disp_resuming(rows, model):
    """--mode=disp row by row past the reference's stops: (out[n, 10] with NaN rows where it stopped, stopped[n])."""
    n = len(rows)
    out, stopped, pos = np.full((n, 10), np.nan), np.zeros(n, dtype=bool), 0
    while pos < n:
        with tempfile.TemporaryDirectory() as td:
            fin, fout = os.path.join(td, "in.txt"), os.path.join(td, "out.bin")
            refharness._write_rows(fin, rows[pos:])
            cmd = [refharness.EXE, "--mode=disp", "--in=%s" % fin, "--out=%s" % fout] + refharness._model_flags(model)
            subprocess.run(cmd, check=False, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            got = np.fromfile(fout, dtype=np.float64)
        got = got[:10 * (got.size // 10)].reshape(-1, 10)
        out[pos:pos + len(got)] = got
        pos += len(got)
        if pos < n:            # the row after the last one written is the one it died on
            stopped[pos] = True
            pos += 1
    return out, stopped


def main():
    if not refharness.available():
        raise SystemExit("oracle/_ref/ref_harness missing: run python oracle/build_ref.py first")
    store = {"build_info": np.array(open(os.path.join(ROOT, "oracle", "_ref", "BUILD_INFO.txt")).read())}
    work = os.path.join(HERE, "_work")
    os.makedirs(work, exist_ok=True)
    for key in list(dr.GRIDS) + ["zero"]:
        F, b = dr.grid(key)
        gf = os.path.join(work, "uniform_%s.txt" % key)
        wl.write_grid_file(gf, F, b)
        mdl = {"kind": 3, "file": gf}
        om = oracle.Model.interp(F, b, wl.QS, wl.MS)
        if key == "zero":
            rows = dr.states("uniform", key, om, 65)
            store["zero_in"] = rows
            store["zero_disp"], st = disp_resuming(rows, mdl)
            assert not st.any()
            pos, d, w = wl.launch_set(8, 5)
            out, _ = refharness.run_rays(mdl, np.concatenate([pos, d, w[:, None]], axis=1), **dict(ZERO_RUN, **{"del": ZERO_DEL}))
            T = max(o["rows"].shape[0] for o in out)
            rr = np.zeros((8, T, 20))
            for i, o in enumerate(out):
                r = o["rows"]
                rr[i, :len(r)] = np.concatenate([r[:, :16], r[:, 24:28]], axis=1)
            store["zero_run_rows"] = rr
            store["zero_run_nrows"] = np.array([o["rows"].shape[0] for o in out], dtype=np.int32)
            store["zero_run_stop"] = np.array([o["stopcond"] for o in out], dtype=np.int32)
            dev = 0.0
            for i in range(8):
                t = rr[i, :store["zero_run_nrows"][i], 0:1]
                line = pos[i] + oracle.lib().so_speed_of_light() * t * d[i]
                dev = max(dev, float(np.max(np.linalg.norm(rr[i, :len(t), 1:4] - line, axis=1) / np.linalg.norm(line, axis=1))))
            store["zero_run_line_dev"] = np.array(dev)
            print("zero: reference's largest deviation from x0 + c t d = %.3g of |x|; rows %s stop %s" % (
                dev, store["zero_run_nrows"].tolist(), store["zero_run_stop"].tolist()))
            continue
        for fam in dr.FAMILIES:
            rows = dr.states(fam, key, om)
            out, st = disp_resuming(rows, mdl)
            store["%s_%s_in" % (key, fam)] = rows
            store["%s_%s_disp" % (key, fam)] = out
            store["%s_%s_stopped" % (key, fam)] = st
            # the comparable set is a property of the inputs: judged with the reference's own outputs where it survived and with
            # the tilted direction's where it did not
            judge = out.copy()
            if st.any() or fam == "aligned":
                tl, st2 = disp_resuming(dr.tilted(rows, om), mdl)
                assert not st2.any()
                judge[st] = tl[st]
                store["%s_%s_tilted" % (key, fam)] = tl
            m = dr.state_metrics(rows, judge, dr.field_at(om, rows[:, :3]))
            outside = 1.0 - m["comparable"].mean()
            print("%s %-11s stopped %3d  cos2>1 %3d  outside the comparable set %.3f  k1 propagates %.2f k2 %.2f" % (
                key, fam, st.sum(), (m["cos2"] > 1).sum(), outside, (judge[:, 6] > 0).mean(), (judge[:, 8] > 0).mean()))
            assert outside <= dr.OUTSIDE_CAP, (key, fam, outside)
    for fam in dr.RH_FAMILIES:
        t = dr.tuples(fam)
        store["rh_%s_in" % fam] = t
        store["rh_%s_out" % fam] = refharness.run_mode("rh", t)[:, 0].astype(np.uint8)
        low = (dr.rh_gap(t) < dr.GAP_MIN).mean()
        print("rh %-7s gap < 1e-6 on %.3f, right-handed on %.2f" % (fam, low, store["rh_%s_out" % fam].mean()))
        assert low <= dr.OUTSIDE_CAP
    path = os.path.join(HERE, "dispersion_regimes_golden.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1e3))
    for f in os.listdir(work):
        os.remove(os.path.join(work, f))
    os.rmdir(work)


if __name__ == "__main__":
    main()
