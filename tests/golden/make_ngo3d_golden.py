#!/usr/bin/env python3
"""Goldens of modelnum 5 (ngo_3d_dens_model_adapter.f95 + ngo_3d_dens_model.f95) from the real reference
-> tests/golden/ngo3d_golden.npz.

Run where the reference's sources are (SRT_REFERENCE, as for oracle/build_ref.py) after build() has left the reference's
objects in oracle/_ref/obj: the harness (ngo3d_harness.f95, ours) is linked against drv_ngo_3d_dens_model_adapter.o,
drv_ngo_3d_dens_model.o, drv_pp_profile_d.o and the raytracer module as they lie there.  Nothing is written into git but the
.npz: every product goes to a temporary directory.

No local of this adapter needed zeroing: the generator runs G0 twice and asserts identical bytes, and every density finite and
positive.  (If that ever fails, zero the local on the way into the compiler as make_simple3d_golden.py does.)

Contents (first_attempt_policy = 0, as for every golden of a flang build):
  G0   funcPlasmaParams at >= 2000 points over four settings (two Kp / date pairs, fixed_MLT 0 and 1, dipole / IGRF / T04_s,
       both workloads.py card files): Ns, B0, the density module's lk after the call, and the reference's own SENSITIVITY per
       point -- the largest relative change of any species when x is shifted by 1 .. 3 ulp.  The points: make_simple3d_golden's
       families, points within +-3 ddk of the local plasmapause at six MLT, and for the ducts file points either side of critl.
       The generator asserts: <= 0.1 % of the points above 1e-11, none above 1e-9, every density finite and positive.
  G2/3 dFdk, dFdw, dFdx, evalrhs and one rk4 / rk45 step at 24 states (x, k, w) per setting (a, b and e: the ducts file
       under the dipole field) on root 2 taken from the reference's own trajectories, each also at 256 few-ulp shifts of x and k (the reference's sensitivity of these layers).
  G4   raytracer_run on 64 rays of config[1]'s launch set, fixed-step and adaptive, each a second time with the launch
       point shifted by 1e-9 relative: the reference's own divergence.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import build_ref  # noqa: E402
from stanford_raytracer_amd import workloads as wl  # noqa: E402

REF, OBJ, FC, OPT = build_ref.REF, build_ref.OBJ, build_ref.FC, build_ref.OPT
R_E = wl.R_E
PARMOD = dict(Pdyn=3.0, Dst=-25.0, ByIMF=1.5, BzIMF=-4.0, W1=0.4, W2=0.5, W3=0.3, W4=0.3, W5=0.4, W6=0.6)
# (name, kp, yearday, msec, fixed_MLT, MLT, use_igrf, use_tsyganenko, card file: 0 = NEWRAY_PLASMAPAUSE, 1 = NEWRAY_DUCTS)
SETTINGS = [
    ("a", 4.0, 2010001, 0, 0, 0.0, 0, 0, 0),
    ("b", 4.0, 2010001, 0, 1, 2.0, 0, 0, 0),
    ("c", 2.0, 2012180, 43200000, 0, 0.0, 1, 0, 1),
    ("d", 2.0, 2012180, 43200000, 1, 14.5, 0, 1, 1),
]
# G2 / G3 also with the ducts file: under the dipole field, as a and b, so that those layers' bars measure the density model and
# not the single-precision field options (no G0 family of its own: c and d hold the ducts file's points)
SETTING_E = ("e", 2.0, 2012180, 43200000, 0, 0.0, 0, 0, 1)
NEWRAY = (wl.NEWRAY_PLASMAPAUSE, wl.NEWRAY_DUCTS)
# what the point families need of the card files: ddk, and the sinusoidal perturbation's l0(2), dd(2)
DDK = (0.07, 0.10)
L02, DD2 = -0.5, 0.4


def a8_of(mlt, kp):
    """bulge's plasmapause location (pp_profile_d.f95:52-131) -- only to place points; nothing is compared with it."""
    f = np.float32
    x = mlt - (47.0 / (kp + f(3.9)) + f(11.3))
    x = x + 24.0 if x < -12.0 else (x - 24.0 if x > 12.0 else x)
    absx = abs(x) * f(2.6179939e-1)
    s = np.sin(mlt * f(0.26179939) + f(1.5707963))
    return ((f(0.043) * s - f(0.4589)) * kp + (-(f(0.361) * s) + f(5.7464))) * (1.0 + np.exp(-(1.5 * absx * absx) + f(0.08) * absx - f(0.7)))


def run(cmd, **kw):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, **kw)
    if r.returncode != 0:
        sys.stderr.write("FAILED: %s\n%s\n" % (" ".join(cmd)[:400], r.stdout))
        raise SystemExit(1)
    return r.stdout


def link_objects():
    """The reference objects build() left behind that the harness needs (no driver, no other adapter)."""
    names = ["types", "constants", "util", "blas", "bmodel_dipole", "raytracer", "drv_pp_profile_d", "drv_ngo_3d_dens_model",
             "drv_ngo_3d_dens_model_adapter"]
    objs = [os.path.join(OBJ, n + ".o") for n in names]
    objs += sorted(os.path.join(OBJ, f) for f in os.listdir(OBJ) if f.startswith(("xd_", "tsy_", "la_")) and f.endswith(".o"))
    missing = [o for o in objs if not os.path.exists(o)]
    assert not missing, "run build() first: %s" % missing[:3]
    return objs


def build_harness(tmp):
    hobj = os.path.join(tmp, "ngo3d_harness.o")
    run([FC, *OPT, "-c", os.path.join(HERE, "ngo3d_harness.f95"), "-I", OBJ, "-module-dir", tmp, "-o", hobj])
    exe = os.path.join(tmp, "ngo3d_harness")
    run([FC, *OPT, "-o", exe, hobj, *link_objects()])
    for k, text in enumerate(NEWRAY):
        with open(os.path.join(tmp, "newray%d.in" % k), "w") as f:
            f.write(text)
    return exe


def flags(s, tmp):
    name, kp, yd, ms, fixed, mlt, igrf, tsy, card = s
    f = ["--ngo_configfile=" + os.path.join(tmp, "newray%d.in" % card),
         "--kp=%r" % kp, "--yearday=%d" % yd, "--milliseconds_day=%d" % ms, "--fixed_MLT=%d" % fixed, "--MLT=%r" % mlt,
         "--use_igrf=%d" % igrf, "--use_tsyganenko=%d" % tsy]
    if tsy:
        f += ["--tsyganenko_%s=%r" % kv for kv in PARMOD.items()]
    return f


def call(exe, tmp, mode, rows, extra, ncol=None):
    fin, fout = os.path.join(tmp, "in.txt"), os.path.join(tmp, "out.bin")
    with open(fin, "w") as f:
        for r in rows:
            f.write(" ".join("%.17e" % v for v in r) + "\n")
    run([exe, "--mode=" + mode, "--in=" + fin, "--out=" + fout, *extra])
    out = np.fromfile(fout, dtype=np.float64)
    return out.reshape(len(rows), ncol) if ncol else out


def ulp_shift(x, rng, count=4):
    """`count` copies of x with every coordinate moved by 1..3 ulp either way."""
    out = []
    for _ in range(count):
        k = rng.integers(1, 4, x.shape) * rng.choice([-1, 1], x.shape)
        out.append(x * (1.0 + k * 2.0 ** -52))
    return out


def sph(r, lat_deg, mlt):
    lat, phi = np.deg2rad(lat_deg), (mlt - 12.0) * 2.0 * np.pi / 24.0
    return [r * np.cos(lat) * np.cos(phi), r * np.cos(lat) * np.sin(phi), r * np.sin(lat)]


def g0_points(setting, rng):
    name, kp, fixed, fmlt, card = setting[0], setting[1], setting[4], setting[5], setting[8]
    pts = []
    # random: r in [1.02, 8.02] R_E, every direction
    n = 90
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    pts += list(v * (R_E * rng.uniform(1.02, 8.02, (n, 1))))
    centroid = 47.0 / (kp + 3.9) + 11.3
    # across the plasmapause at several MLT, on the equator and at +-30 degrees (r = L cos^2 lat)
    for mlt in (0.02, 3.5, 8.0, centroid, 21.0, 23.98):
        for L in np.linspace(2.0, 7.0, 11):
            for lat in (0.0, 30.0, -30.0):
                pts.append(sph(L * R_E * np.cos(np.deg2rad(lat)) ** 2, lat, mlt))
    # through the ionosphere merge, 200 .. 12 000 km, both hemispheres
    for mlt in (2.0, 13.0):
        for lat in (-60.0, -20.0, 0.0, 35.0, 70.0):
            for alt in np.geomspace(200e3, 12000e3, 9):
                pts.append(sph(R_E + alt, lat, mlt))
    # MLT near 0/24 (y just either side of 0 at x > 0), 3.5, 8 (the trough's branch) and the bulge centroid
    for r in (1.5 * R_E, 4.0 * R_E):
        for mlt in (1e-9, 24 - 1e-9, 3.5 - 1e-6, 3.5 + 1e-6, 8.0 - 1e-9, 8.0 + 1e-9, centroid - 1e-6, centroid + 1e-6, 12.0, 18.0, 6.0):
            for lat in (10.0, -25.0):
                pts.append(sph(r, lat, mlt))
    # within +-3 ddk of the local plasmapause lk = a8 - ddk (the knee's deltal = l - lk changes sign there) at six MLT
    ddk = DDK[card]
    for mlt in (0.5, 4.0, 9.0, centroid, 17.0, 22.5):
        lk = a8_of(fmlt if fixed else mlt, kp) - ddk
        for off in (-3.0, -1.5, -0.5, -1e-3, 1e-3, 0.5, 1.5, 3.0):
            for lat in (0.0, 25.0, -25.0):
                pts.append(sph((lk + off * ddk) * R_E * np.cos(np.deg2rad(lat)) ** 2, lat, mlt))
        if card == 1:  # either side of the sinusoidal perturbation's critl (ngo_3d_dens_model.f95: delk, critl)
            delk = -L02 - (lk + ddk) + DD2 / 2
            critl = (lk + ddk) + np.fmod(delk, DD2)
            for off in (-0.1, -0.01, -1e-4, 1e-4, 0.01, 0.1):
                for lat in (0.0, 20.0):
                    pts.append(sph((critl + off) * R_E * np.cos(np.deg2rad(lat)) ** 2, lat, mlt))
    return np.array(pts, dtype=np.float64)


def read_runs(buf, nrays):
    """--mode=run stream -> list of (stop, rows[T, 32])."""
    out, o = [], 0
    for _ in range(nrays):
        stop, T = int(buf[o + 1]), int(buf[o + 2])
        o += 3
        out.append((stop, buf[o:o + 32 * T].reshape(T, 32).copy()))
        o += 32 * T
    assert o == len(buf)
    return out


def pack_runs(runs, slots):
    n = len(runs)
    rows = np.full((n, slots, 7), np.nan)  # t, pos(3), vgrel(3): what the curve comparison reads
    nrows, stop = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for i, (s, r) in enumerate(runs):
        T = len(r)
        assert T <= slots
        nrows[i], stop[i] = T, s
        rows[i, :T, 0:4] = r[:, 0:4]
        rows[i, :T, 4:7] = r[:, 7:10]
    return rows, nrows, stop


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference sources not found at %s" % REF)
    build_ref.build()
    rng = np.random.default_rng(20260)
    g = {}
    with tempfile.TemporaryDirectory(prefix="ngo3dgold") as tmp:
        exe = build_harness(tmp)
        # ---- G0
        for s in SETTINGS:
            x = g0_points(s, rng)
            base = call(exe, tmp, "params", x, flags(s, tmp), 20)
            again = call(exe, tmp, "params", x, flags(s, tmp), 20)
            assert base.tobytes() == again.tobytes(), "setting %s: two runs differ -- an unset local?" % s[0]
            Ns, B0, lk = base[:, 4:8], base[:, 16:19], base[:, 19]
            assert np.all(np.isfinite(Ns)) and np.all(Ns > 0) and np.all(np.isfinite(lk)), s[0]
            sens = np.zeros(len(x))
            for xs in ulp_shift(x, rng):
                Nss = call(exe, tmp, "params", xs, flags(s, tmp), 20)[:, 4:8]
                sens = np.maximum(sens, np.max(np.abs(Nss - Ns) / Ns, axis=1))
            assert np.isclose(base[0, 0], -1.602e-19, rtol=1e-15) and np.isclose(base[0, 9], 1.6726e-27, rtol=1e-15)
            g["g0_x_" + s[0]], g["g0_Ns_" + s[0]], g["g0_B0_" + s[0]], g["g0_sens_" + s[0]] = x, Ns, B0, sens
            g["g0_lk_" + s[0]] = lk
            g["g0_setting_" + s[0]] = np.array(s[1:], dtype=np.float64)
            print("G0 %s: %d points, sens max %.2e, above 1e-11: %d, lk %.2f .. %.2f, beyond the plasmapause %d" % (
                s[0], len(x), sens.max(), int((sens > 1e-11).sum()), lk.min(), lk.max(),
                int((np.linalg.norm(x, axis=1) ** 3 / (R_E * (x[:, 0] ** 2 + x[:, 1] ** 2)) > lk).sum())))
        allsens = np.concatenate([g["g0_sens_" + s[0]] for s in SETTINGS])
        assert len(allsens) >= 2000
        assert np.mean(allsens > 1e-11) <= 1e-3 and allsens.max() <= 1e-9, (np.mean(allsens > 1e-11), allsens.max())
        g["parmod"] = np.array(list(PARMOD.values()))
        g["ddk"] = np.array(DDK)
        # ---- G4: 64 rays of config[1]'s launch set, settings a (free MLT) and b (fixed) half each
        P, D, W = wl.launch_set(100_000, 2)
        pick = np.arange(64) * 1562
        pos0, dir0, w0 = P[pick], D[pick], W[pick]
        g["run_pos0"], g["run_dir0"], g["run_w0"] = pos0, dir0, w0
        runkw = {"fixed": dict(fixedstep=1, dt0=1e-3, dtmax=0.1, tmax=10.0, maxerr=5e-4, maxsteps=16, minalt=wl.MINALT, del_=1e-6),
                 "adaptive": dict(fixedstep=0, dt0=1e-3, dtmax=0.05, tmax=0.6, maxerr=5e-4, maxsteps=24, minalt=wl.MINALT, del_=1e-6)}
        states = []
        for mode, kw in runkw.items():
            extra = ["--%s=%r" % (k.rstrip("_"), v) for k, v in kw.items()]
            g["run_%s_params" % mode] = np.array([kw[k] for k in ("fixedstep", "dt0", "dtmax", "tmax", "maxerr", "maxsteps", "minalt", "del_")], dtype=np.float64)
            for tag, p0 in (("", pos0), ("_shift", pos0 * (1.0 + 1e-9))):
                rows_all = []
                for half, s in ((slice(0, 32), SETTINGS[0]), (slice(32, 64), SETTINGS[1])):
                    inp = np.concatenate([p0[half], dir0[half], w0[half, None]], axis=1)
                    rows_all += read_runs(call(exe, tmp, "run", inp, flags(s, tmp) + extra), 32)
                rows, nrows, stop = pack_runs(rows_all, kw["maxsteps"])
                g["run_%s%s_rows" % (mode, tag)] = rows
                g["run_%s%s_nrows" % (mode, tag)], g["run_%s%s_stop" % (mode, tag)] = nrows, stop
                if mode == "fixed" and tag == "":
                    states = rows_all
            print("G4 %s: stop codes %s, rows %d..%d" % (mode, sorted(set(g["run_%s_stop" % mode].tolist())), g["run_%s_nrows" % mode].min(), g["run_%s_nrows" % mode].max()))
        # ---- G2/G3 at states of the reference's own fixed-step trajectories (k = n w / c, on root 2)
        C = float(np.sqrt(1.0 / 8.854187817e-12 / (np.pi * 4e-7)))
        fixed_extra = ["--%s=%r" % (k.rstrip("_"), v) for k, v in runkw["fixed"].items()]
        inp_all = np.concatenate([pos0, dir0, w0[:, None]], axis=1)
        for half, s in ((range(0, 32), SETTINGS[0]), (range(32, 64), SETTINGS[1]), (range(0, 32), SETTING_E)):
            if s[0] == "e":  # (the ducts file: trajectories of its own, kept only for their states)
                own = read_runs(call(exe, tmp, "run", inp_all[half.start:half.stop], flags(s, tmp) + fixed_extra), 32)
                states_of = dict(zip(half, own))
            else:
                states_of = {i: states[i] for i in half}
            st = []
            for i in half:
                _, r = states_of[i]
                for t in (0, min(len(r) - 1, 9)):
                    if len(r) > 1:
                        st.append(np.concatenate([r[t, 1:4], r[t, 10:13] * w0[i] / C, [w0[i]]]))
            st = np.array(st)[:24]
            dt = np.full((len(st), 1), 1e-3)  # the ladder's G3 step: dt0 of config[1] and of the other models' G3 goldens
            dl = np.full((len(st), 1), 1e-6)
            g["g23_state_" + s[0]] = st
            g["g0_setting_" + s[0]] = np.array(s[1:], dtype=np.float64)
            g["g2_" + s[0]] = call(exe, tmp, "grad", np.hstack([st, dl]), flags(s, tmp), 14)
            g["g3_" + s[0]] = call(exe, tmp, "step", np.hstack([st, dt, dl]), flags(s, tmp), 21)
            g["g3_dt"] = np.array(1e-3)
            # the reference's own sensitivity of these layers: the same calls at x shifted by a few ulp
            s2, s3 = np.zeros_like(g["g2_" + s[0]]), np.zeros_like(g["g3_" + s[0]])
            # (x and k together, 256 shifts: with the ducts file a state next to one of dens' kinks changes its answer by 1e-7 ..
            # 4e-7 under one shift in 8 .. 30, one state only when k moves, not x; eight shifts of x record such states as quiet)
            for xs in ulp_shift(st[:, 0:6], rng, 256):
                st2 = st.copy()
                st2[:, 0:6] = xs
                s2 = np.maximum(s2, np.abs(call(exe, tmp, "grad", np.hstack([st2, dl]), flags(s, tmp), 14) - g["g2_" + s[0]]))
                s3 = np.maximum(s3, np.abs(call(exe, tmp, "step", np.hstack([st2, dt, dl]), flags(s, tmp), 21) - g["g3_" + s[0]]))
            g["g2_sens_" + s[0]], g["g3_sens_" + s[0]] = s2, s3
    out = os.path.join(HERE, "ngo3d_golden.npz")
    np.savez_compressed(out, **g)
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))
    assert os.path.getsize(out) < os.path.getsize(os.path.join(HERE, "simple3d_golden.npz"))


if __name__ == "__main__":
    main()
