#!/usr/bin/env python3
"""Goldens of the reference's dumpmodel and of xform_double's SM <-> MAG rotations ->
tests/golden/dump_*.txt, tests/golden/dumpmodel_settings.json, tests/golden/dumpmodel_golden.npz.

Run where the reference's sources are (SRT_REFERENCE, as for oracle/build_ref.py) after build() has left the reference's
objects in oracle/_ref/obj.  The reference's own fortran/dumpmodel.f95 is compiled where it lies and linked against those
objects (xform_double, geopack, T04_s, GCPM and IRI included, as oracle/build_ref.py's build_driver links them); every product
goes to tests/golden/_work/, which is git-ignored.  Two departures, both forced by flang and neither changes arithmetic: the
GNU intrinsic iargc() (-cpp -Diargc=command_argument_count, as for the driver), and the GNU comma after the format of the
three final WRITE statements, which is streamed out by sed on the way into flang's stdin (the edited text is never written
to disk).  Model 6's adapter is the object with its three unset locals zeroed, made by make_simple3d_golden.build_harness.

What is committed is DATA: the text files the program wrote (a few KB each), the settings of each run, and in the .npz
  sens_<fixture>[nz, ny, nx]   the reference's own sensitivity per node: the largest relative change of any density when every
                               bound is scaled by 1 + 4.4e-16 and by 1 - 4.4e-16 (two further runs of the same program);
  xf_*                         sm_to_mag_d, mag_to_sm_d and the round trip at 206 points for each of six dates, from
                               xform_harness.f95 (ours, linked against the reference's xform_double objects).
Asserted here (conditions on the INPUTS: if one fails, move the bounds, do not loosen it): no node of the four SM fixtures moves
by more than 1e-12 relative, none of the MAG fixture by more than 1e-10; the round trip SM -> MAG -> SM returns every component
to 1e-14 |x| in the reference itself.
"""
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import make_simple3d_golden as s3d  # noqa: E402  (the zeroed model-6 adapter object: its helper, not a copy)
from oracle import build_ref  # noqa: E402
from stanford_raytracer_amd import api, workloads as wl  # noqa: E402

REF, OBJ, FC, OPT = build_ref.REF, build_ref.OBJ, build_ref.FC, build_ref.OPT
WORK = os.path.join(HERE, "_work")
R_E = wl.R_E
EPS = 4.4e-16
DATE = ["--yearday=2010001", "--milliseconds_day=0"]
# fixture -> (model flags without paths, nx ny nz, bounds in R_E).  Bounds away from the plasmapause knee (L = 5.55 in the card
# file, about 3.8 for Kp 4) and above 1000 km.
FIXTURES = {
    "dump_ngo_5x1x4": dict(modelnum=1, flags=["--use_igrf=0", "--use_tsyganenko=0"], n=(5, 1, 4),
                           bounds=(1.5, 4.5, 0.0, 0.0, -1.2, 1.2)),
    "dump_interp_4x3x2": dict(modelnum=3, flags=["--use_igrf=1", "--use_tsyganenko=0"], n=(4, 3, 2),
                              bounds=(1.3, 3.7, -1.1, 1.3, 0.4, 1.9)),
    "dump_scattered_3x3x1": dict(modelnum=4, flags=["--use_igrf=0", "--use_tsyganenko=0", "--scattered_interp_window_scale=1.5",
                                                    "--scattered_interp_order=2", "--scattered_interp_exact=0",
                                                    "--scattered_interp_local_window_scale=5.0"], n=(3, 3, 1),
                                 bounds=(1.4, 3.4, -1.5, 1.5, 0.7, 0.7)),
    "dump_simple3d_sm_6x1x5": dict(modelnum=6, flags=["--kp=4.0", "--use_igrf=0", "--use_tsyganenko=0", "--mag_coords=0"], n=(6, 1, 5),
                                   bounds=(1.6, 3.1, 0.0, 0.0, -0.9, 0.9)),
    "dump_simple3d_mag_6x1x5": dict(modelnum=6, flags=["--kp=4.0", "--use_igrf=0", "--use_tsyganenko=0", "--mag_coords=1"], n=(6, 1, 5),
                                    bounds=(1.6, 3.1, 0.0, 0.0, -0.9, 0.9)),
}
XF_DATES = [(2010001, 0), (2001093, 43200000), (2012060, 21600000), (2015200, 86399999), (1985123, 3600000), (2020300, 50000000)]

run = s3d.run


def build_programs():
    os.makedirs(WORK, exist_ok=True)
    s3d.build_harness(WORK)  # leaves simple3d_zeroed.o (and its .mod) in WORK
    zero_obj = os.path.join(WORK, "simple3d_zeroed.o")
    skip = {"ref_harness.o", "drv_raytracer_driver.o", "drv_simple_3d_model_adapter.o", "gb_gcpm_dens_model_buildgrid.o",
            "gb_gcpm_dens_model_buildgrid_random.o"}
    objs = sorted(os.path.join(OBJ, f) for f in os.listdir(OBJ) if f.endswith(".o") and f not in skip)
    text = run(["sed", "-E", r"s/^(  write\(outfile, '[^']*'\)),/\1/", os.path.join(REF, "fortran", "dumpmodel.f95")])
    dobj = os.path.join(WORK, "dumpmodel.o")
    run([FC, *OPT, "-cpp", "-Diargc=command_argument_count", "-x", "f95", "-ffree-form", "-c", "-", "-I", WORK, "-I", OBJ,
         "-module-dir", WORK, "-o", dobj], input=text)
    exe = os.path.join(WORK, "dumpmodel")
    run([FC, *OPT, "-o", exe, dobj, zero_obj, *objs])
    hobj = os.path.join(WORK, "xform_harness.o")
    run([FC, *OPT, "-c", os.path.join(HERE, "xform_harness.f95"), "-I", OBJ, "-module-dir", WORK, "-o", hobj])
    xexe = os.path.join(WORK, "xform_harness")
    xobjs = [os.path.join(OBJ, n + ".o") for n in ("types", "util")]
    xobjs += sorted(os.path.join(OBJ, f) for f in os.listdir(OBJ) if f.startswith("xd_") and f.endswith(".o"))
    run([FC, *OPT, "-o", xexe, hobj, *xobjs])
    return exe, xexe


def model_inputs():
    """The files the model flags name, written from the committed fixtures."""
    cfg = os.path.join(WORK, "newray_plasmapause.in")
    with open(cfg, "w") as f:
        f.write(wl.NEWRAY_PLASMAPAUSE)
    g = np.load(os.path.join(HERE, "grid16.npz"))
    grid = os.path.join(WORK, "grid16.txt")
    api.write_grid_file(grid, g["F"], g["bounds"], g["qs"], g["ms"])
    p = np.load(os.path.join(HERE, "points5500.npz"))
    pts = os.path.join(WORK, "points5500.txt")
    wl.write_points_file(pts, p["pts"], p["lnN"], p["bounds"], p["qs"], p["ms"])
    return {1: ["--ngo_configfile=" + cfg], 3: ["--interp_interpfile=" + grid], 4: ["--interp_interpfile=" + pts], 6: []}


def dump(exe, fx, paths, out, scale=1.0):
    b = [v * R_E * scale for v in fx["bounds"]]
    names = ("minx", "maxx", "miny", "maxy", "minz", "maxz")
    cmd = [exe, "--modelnum=%d" % fx["modelnum"], *DATE, *fx["flags"], *paths[fx["modelnum"]], "--filename=" + out,
           *["--%s=%.17e" % kv for kv in zip(names, b)], *["--n%s=%d" % kv for kv in zip("xyz", fx["n"])]]
    run(cmd, cwd=WORK)
    return b


def parse(path):
    v = np.array(open(path).read().split(), dtype=np.float64)
    nspec, nx, ny, nz = (int(t) for t in v[:4])
    return nspec, v[4:10], v[10:].reshape(nz, ny, nx, 4 * nspec + 3)


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference sources not found at %s" % REF)
    build_ref.build()
    exe, xexe = build_programs()
    paths = model_inputs()
    g, settings = {}, {}
    for name, fx in FIXTURES.items():
        out = os.path.join(HERE, name + ".txt")
        b = dump(exe, fx, paths, out)
        nspec, fb, f = parse(out)
        assert np.array_equal(fb, np.array(b)) and f.shape[:3] == fx["n"][::-1]
        Ns = f[..., nspec:2 * nspec]
        assert np.all(np.isfinite(f)) and np.all(Ns > 0), name
        sens = np.zeros(Ns.shape[:3])
        for s in (1.0 + EPS, 1.0 - EPS):
            tmp = os.path.join(WORK, name + "_shift.txt")
            dump(exe, fx, paths, tmp, s)
            Nss = parse(tmp)[2][..., nspec:2 * nspec]
            sens = np.maximum(sens, np.max(np.abs(Nss - Ns) / Ns, axis=-1))
        bar = 1e-10 if "--mag_coords=1" in fx["flags"] else 1e-12
        print("%s: %d nodes, nspec %d, sensitivity max %.2e (bar %.0e), %d bytes" % (name, sens.size, nspec, sens.max(), bar, os.path.getsize(out)))
        assert sens.max() <= bar, (name, sens.max())
        g["sens_" + name] = sens
        settings[name] = dict(modelnum=fx["modelnum"], yearday=2010001, milliseconds_day=0, flags=fx["flags"], n=list(fx["n"]),
                              bounds=b, file=name + ".txt")
    # ---- the rotations: 200 random points in 1 .. 10 R_E and the six axis points, at six dates
    rng = np.random.default_rng(20261)
    v = rng.normal(size=(200, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    x = np.concatenate([v * (R_E * rng.uniform(1.0, 10.0, (200, 1))), R_E * np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1.0]])])
    fin, fout = os.path.join(WORK, "xf_in.txt"), os.path.join(WORK, "xf_out.bin")
    with open(fin, "w") as f:
        for r in x:
            f.write(" ".join("%.17e" % t for t in r) + "\n")
    res = []
    for yd, ms in XF_DATES:
        run([xexe, "--yearday=%d" % yd, "--milliseconds_day=%d" % ms, "--in=" + fin, "--out=" + fout])
        o = np.fromfile(fout, dtype=np.float64).reshape(len(x), 9)
        rt = np.max(np.abs(o[:, 6:9] - x) / np.linalg.norm(x, axis=1, keepdims=True))
        print("xform %d %d: round trip max %.2e |x|" % (yd, ms, rt))
        assert rt <= 1e-14, rt
        res.append(o)
    res = np.array(res)
    g["xf_dates"], g["xf_x"] = np.array(XF_DATES, dtype=np.int64), x
    g["xf_sm_to_mag"], g["xf_mag_to_sm"], g["xf_round_trip"] = res[:, :, 0:3], res[:, :, 3:6], res[:, :, 6:9]
    with open(os.path.join(HERE, "dumpmodel_settings.json"), "w") as f:
        f.write("{\n" + ",\n".join(" %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in settings.items()) + "\n}\n")  # a line per fixture
    out = os.path.join(HERE, "dumpmodel_golden.npz")
    np.savez_compressed(out, **g)
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
