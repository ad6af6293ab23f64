#!/usr/bin/env python3
"""Goldens of modelnum 7 (AT64ThCh_adapter.f95) from the real reference -> tests/golden/at64thch_golden.npz.

Run where the reference's sources are (SRT_REFERENCE, as for oracle/build_ref.py) after build() has left the reference's
objects in oracle/_ref/obj.  Nothing is written into git but the .npz: every product goes to a temporary directory.

The adapter is streamed through sed into flang's stdin with exactly three edits; the edited text is never written to disk:
  * `external :: T04_s, IGRF_GSM` after :75, the line oracle/build_ref.py already uses;
  * `psi = 0.0` after :104: psi is a local that nothing sets and that the final T04_s call reads when use_tsyganenko = 1; the
    reference's own toolchain zeroes locals (-finit-local-zero, SURVEY A-1), flang does not;
  * `real(PARMOD)` for `PARMOD` at :204: the adapter hands a DOUBLE array to TRACE_08's REAL PARMOD(10) through an implicit
    interface, so the trace's T04_s reads the first 40 bytes of five doubles as ten floats.
The object that oracle/build_ref.py builds for the reference's driver (first edit only) is linked once as well, and this script
asserts that with Pdyn = 1.7 it does not return the edited build's densities (a crash counts): the reason for the third edit,
kept on record.

Our harness (at64thch_harness.f95) calls the module's funcPlasmaParams and, with correctly typed arguments, geopack's own
TRACE_08 for the foot, the ending and L.  A point at or below 400 km has no foot here (NaN): the model does not trace it, and
TRACE_08 started inside R0 interpolates towards XR, YR, ZR before it has set them (with -fno-automatic: the previous call's).

The trace is fp32, so a few-ulp shift of x in double never reaches it.  The reference's own SENSITIVITY of every output is
therefore taken over fp32-ulp shifts: each point is run again at x (1 - 6e-8), x (1 + 6e-8) and x (1 + 1.2e-7), and the largest
relative change of each density, the largest movement of the foot (R_E) and whether the ending changed are stored with it.
A point at or below 400 km has no trace; there the model is a closed form in double that falls by a factor e in a few km
(d ln N / d ln r is several thousand at 100 km), so an fp32-ulp shift measures that slope and nothing about rounding: its
density sensitivity is taken over shifts of +-2 and +3 ulp of double instead, as for the other closed-form models.
The trace enters the model through zbrat alone, and zbrat multiplies n_e; the ion densities are n_e times a closed-form
fraction.  The SENSITIVITY CONDITION is therefore on n_e, over all points of all families: at most 5 % above 1e-5, none above
1e-3.  (The O+ column is kept out of it for what it measures: n_O+ = n_e / (1 + R13), R13 = exp(z (H1 - H3) / (H1 H3)), and
d ln R13 / d ln r is 20 at 2 R_E and 160 at 400 km, so under the same shifts O+ moves by 1e-6 .. 2e-5 with no rounding in it; its
recorded sensitivity still sets its own bar in the tests.)  The generator also asserts at least 20 endings on the sphere and 20
on the outer boundary, every L <= 500, every density finite and positive.  When the condition fails the points are drawn
again with another seed (AT64_SEED).

Contents (first_attempt_policy = 0, as for every golden of a flang build):
  G0   funcPlasmaParams and TRACE_08 over four settings (a: kp 4, 2010-001, Pdyn 4; b: kp 2, 2012-180, Pdyn 1.7; c: a with
       use_igrf = 1; d: b with use_igrf = 1 and use_tsyganenko = 1) on five families of points: 400 random (r 1.08 .. 6 R_E,
       |lat| <= 55 deg), 40 at 100 .. 400 km (no trace) and 20 pairs +- 1 km about 400 km, 60 across the plasmapause L = 5.6 -
       0.46 kp +- 3 Lw at latitude 0 and 30 deg, and 60 high-latitude points at r = 5 .. 9 R_E whose lines leave through the
       outer boundary.  Settings a and b have all five; c and d, which differ from them only in the base field of |B(point)|
       and in B0, have the random and the high-latitude family.
  G2/3 dFdk, dFdw, dFdx, evalrhs and one rk4 / rk45 step at 24 states per setting a, b, d, with sensitivities over the same
       fp32-ulp shifts of x and of k.
  G4   raytracer_run on 16 rays in setting d, 4 fixed steps and 5 adaptive steps (6 attempts with the launch point's), each a
       second time with the launch point shifted by 1e-9 relative: the reference's own divergence.
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
ADAPTER = os.path.join(REF, "fortran", "AT64ThCh_adapter.f95")
EDITS = ["-e", r"75a\    external :: T04_s, IGRF_GSM", "-e", r"104a\    psi = 0.0", "-e", r"204s/IOPT,PARMOD,T04_s/IOPT,real(PARMOD),T04_s/"]
R_E = wl.R_E
DEL = 1e-4  # delSP, the driver's step for modelnum 7
LW = 0.14
PARMOD_A = dict(Pdyn=4.0, Dst=1.0, ByIMF=0.0, BzIMF=-5.0, W1=0.132, W2=0.303, W3=0.083, W4=0.070, W5=0.211, W6=0.308)
PARMOD_B = dict(Pdyn=1.7, Dst=-25.0, ByIMF=1.5, BzIMF=-4.0, W1=0.4, W2=0.5, W3=0.3, W4=0.3, W5=0.4, W6=0.6)
# (name, gcpm_kp, yearday, msec, use_igrf, use_tsyganenko, parmod, all five families of points)
SETTINGS = [
    ("a", 4, 2010001, 0, 0, 0, PARMOD_A, True),
    ("b", 2, 2012180, 43200000, 0, 0, PARMOD_B, True),
    ("c", 4, 2010001, 0, 1, 0, PARMOD_A, False),
    ("d", 2, 2012180, 43200000, 1, 1, PARMOD_B, False),
]
SHIFTS = (1.0 - 6e-8, 1.0 + 6e-8, 1.0 + 1.2e-7)
SHIFTS_DP = (1.0 - 2 * 2.0 ** -52, 1.0 + 2 * 2.0 ** -52, 1.0 + 3 * 2.0 ** -52)


def run(cmd, **kw):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, **kw)
    if r.returncode != 0:
        sys.stderr.write("FAILED: %s\n%s\n" % (" ".join(cmd)[:400], r.stdout))
        raise SystemExit(1)
    return r.stdout


def link_objects():
    """The reference objects build() left behind that the harness needs (no driver, no other adapter)."""
    names = ["types", "constants", "util", "blas", "bmodel_dipole", "raytracer"]
    objs = [os.path.join(OBJ, n + ".o") for n in names]
    objs += sorted(os.path.join(OBJ, f) for f in os.listdir(OBJ) if f.startswith(("xd_", "tsy_", "la_")) and f.endswith(".o"))
    missing = [o for o in objs if not os.path.exists(o)]
    assert not missing, "run build() first: %s" % missing[:3]
    return objs


def build_harness(tmp):
    edited = os.path.join(tmp, "at64thch_edited.o")
    text = run(["sed", *EDITS, ADAPTER])
    assert "external :: T04_s, IGRF_GSM" in text and "    psi = 0.0\n" in text and text.count("real(PARMOD),T04_s") == 1
    run([FC, *OPT, "-x", "f95", "-ffree-form", "-c", "-", "-I", OBJ, "-module-dir", tmp, "-o", edited], input=text)
    hobj = os.path.join(tmp, "at64thch_harness.o")
    run([FC, *OPT, "-c", os.path.join(HERE, "at64thch_harness.f95"), "-I", OBJ, "-module-dir", tmp, "-o", hobj])
    objs = link_objects()
    exe = os.path.join(tmp, "at64thch_harness")
    run([FC, *OPT, "-o", exe, hobj, edited, *objs])
    raw = os.path.join(OBJ, "drv_AT64ThCh_adapter.o")  # the driver's object: the external line only
    exe_raw = os.path.join(tmp, "at64thch_harness_unedited")
    run([FC, *OPT, "-o", exe_raw, hobj, raw, *objs])
    return exe, exe_raw


def flags(s):
    name, kp, yd, ms, igrf, tsy, parmod, _ = s
    f = ["--gcpm_kp=%d" % kp, "--yearday=%d" % yd, "--milliseconds_day=%d" % ms, "--use_igrf=%d" % igrf, "--use_tsyganenko=%d" % tsy]
    return f + ["--tsyganenko_%s=%r" % kv for kv in parmod.items()]


def call(exe, tmp, mode, rows, extra, ncol=None):
    fin, fout = os.path.join(tmp, "in.txt"), os.path.join(tmp, "out.bin")
    with open(fin, "w") as f:
        for r in rows:
            f.write(" ".join("%.17e" % v for v in r) + "\n")
    run([exe, "--mode=" + mode, "--in=" + fin, "--out=" + fout, *extra])
    out = np.fromfile(fout, dtype=np.float64)
    return out.reshape(len(rows), ncol) if ncol else out


def sph(r, lat_deg, lon_deg):
    lat, phi = np.deg2rad(lat_deg), np.deg2rad(lon_deg)
    return [r * np.cos(lat) * np.cos(phi), r * np.cos(lat) * np.sin(phi), r * np.sin(lat)]


def g0_points(setting, rng):
    """-> x[n, 3], family[n] (0 random, 1 below 400 km, 2 pairs about 400 km, 3 plasmapause, 4 open lines)"""
    kp, every = setting[1], setting[7]
    pts, fam = [], []
    for _ in range(400):
        pts.append(sph(R_E * rng.uniform(1.08, 6.0), rng.uniform(-55.0, 55.0), rng.uniform(0.0, 360.0)))
        fam.append(0)
    for _ in range(60):
        pts.append(sph(R_E * rng.uniform(5.0, 9.0), rng.uniform(65.0, 80.0) * rng.choice([-1.0, 1.0]), rng.uniform(0.0, 360.0)))
        fam.append(4)
    if not every:
        return np.array(pts, dtype=np.float64), np.array(fam, dtype=np.int8)
    for alt in np.linspace(100e3, 399e3, 40):  # (at 400 km itself a shift decides whether there is a trace)
        pts.append(sph(R_E + alt, rng.uniform(-70.0, 70.0), rng.uniform(0.0, 360.0)))
        fam.append(1)
    for _ in range(20):
        lat, lon = rng.uniform(-60.0, 60.0), rng.uniform(0.0, 360.0)
        for dz in (-1e3, 1e3):
            pts.append(sph(R_E + 400e3 + dz, lat, lon))
            fam.append(2)
    lpp = 5.6 - 0.46 * kp
    for lat in (0.0, 30.0):
        for L in np.linspace(lpp - 3 * LW, lpp + 3 * LW, 30):
            pts.append(sph(L * R_E * np.cos(np.deg2rad(lat)) ** 2, lat, rng.uniform(0.0, 360.0)))
            fam.append(3)
    return np.array(pts, dtype=np.float64), np.array(fam, dtype=np.int8)


def read_runs(buf, nrays, ncol):
    out, o = [], 0
    for _ in range(nrays):
        stop, T = int(buf[o + 1]), int(buf[o + 2])
        o += 3
        out.append((stop, buf[o:o + ncol * T].reshape(T, ncol).copy()))
        o += ncol * T
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


def g0(exe, tmp, rng, g):
    """G0 of every setting into g; False when the sensitivity condition fails."""
    for s in SETTINGS:
        t = s[0]
        x, fam = g0_points(s, rng)
        base = call(exe, tmp, "params", x, flags(s), 15)
        Ns, B0 = base[:, 3:6], base[:, 12:15]
        foot = call(exe, tmp, "trace", x, flags(s), 6)
        assert np.all(np.isfinite(Ns)) and np.all(Ns > 0), t
        assert np.all(foot[:, 5] <= 500), t
        untraced = np.linalg.norm(x, axis=1) - R_E <= 400e3
        sens, fsens, ksame = np.zeros((len(x), 3)), np.zeros(len(x)), np.ones(len(x), bool)
        for f, fdp in zip(SHIFTS, SHIFTS_DP):
            Nss = call(exe, tmp, "params", np.where(untraced[:, None], x * fdp, x * f), flags(s), 15)[:, 3:6]
            sens = np.maximum(sens, np.abs(Nss - Ns) / Ns)
            fs = call(exe, tmp, "trace", x * f, flags(s), 6)
            fsens = np.maximum(fsens, np.linalg.norm(fs[:, 0:3] - foot[:, 0:3], axis=1))
            ksame &= fs[:, 4] == foot[:, 4]
        assert np.isclose(base[0, 0], -1.602e-19, rtol=1e-15) and np.isclose(base[0, 7], 16.0 * 1.6726e-27, rtol=1e-15)
        foot[untraced], fsens[untraced] = np.nan, 0.0
        for k, v in (("x", x), ("fam", fam), ("Ns", Ns), ("B0", B0), ("sens", sens), ("foot", foot), ("foot_sens", fsens), ("kind_steady", ksame)):
            g["g0_%s_%s" % (k, t)] = v
        g["g0_setting_" + t] = np.array(s[1:6], dtype=np.float64)
        g["parmod_" + t] = np.array(list(s[6].values()))
        traced = fam != 1
        for k, name in enumerate(("n_e", "O+", "H+")):
            c = sens[traced, k]
            print("G0 %s %-3s: sensitivity median %.2e p90 %.2e max %.2e, above 1e-5: %d of %d" % (t, name, np.median(c), np.quantile(c, 0.9), sens[:, k].max(), int((sens[:, k] > 1e-5).sum()), len(x)))
        print("G0 %s: endings %s; L max %d; foot moves <= %.2e" % (t, np.bincount(foot[~untraced, 4].astype(int)).tolist(), int(foot[~untraced, 5].max()), fsens.max()))
    allsens = np.concatenate([g["g0_sens_" + s[0]] for s in SETTINGS])
    allkind = np.concatenate([g["g0_foot_" + s[0]][:, 4] for s in SETTINGS])
    ne = allsens[:, 0]
    print("all settings: %d points; n_e: %.2f %% above 1e-5, max %.2e; any species: %.2f %% above 1e-5, max %.2e"
          % (len(ne), 100 * np.mean(ne > 1e-5), ne.max(), 100 * np.mean(allsens.max(axis=1) > 1e-5), allsens.max()))
    assert (allkind == 0).sum() >= 20 and (allkind == 1).sum() >= 20
    return bool(np.mean(ne > 1e-5) <= 0.05 and ne.max() <= 1e-3)

NCOL_RUN = 28  # t pos(3) vprel(3) vgrel(3) n(3) B0(3) qs(3) ms(3) Ns(3) nus(3)


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference sources not found at %s" % REF)
    build_ref.build()
    g = {}
    with tempfile.TemporaryDirectory(prefix="at64gold") as tmp:
        exe, exe_raw = build_harness(tmp)
        # ---- G0
        seed = int(os.environ.get("AT64_SEED", "7064"))
        if not g0(exe, tmp, np.random.default_rng(seed), g):
            raise SystemExit("seed %d: the sensitivity condition does not hold; draw the points again (AT64_SEED)" % seed)
        g["seed"] = np.array(seed)
        # ---- the unedited adapter with Pdyn = 1.7 does not give these densities (a crash counts)
        sb = SETTINGS[1]
        probe = g["g0_x_b"][:4]
        fin, fout = os.path.join(tmp, "probe.txt"), os.path.join(tmp, "probe.bin")
        with open(fin, "w") as f:
            for r in probe:
                f.write(" ".join("%.17e" % v for v in r) + "\n")
        r = subprocess.run([exe_raw, "--mode=params", "--in=" + fin, "--out=" + fout, *flags(sb)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        same = False
        if r.returncode == 0 and os.path.exists(fout):
            raw = np.fromfile(fout, dtype=np.float64)
            same = raw.size == 60 and np.array_equal(raw.reshape(4, 15)[:, 3:6], g["g0_Ns_b"][:4])
        assert not same, "the unedited adapter was expected to differ from the edited build at Pdyn = 1.7"
        print("unedited adapter at Pdyn = 1.7: exit code %d, densities %s" % (r.returncode, "differ" if r.returncode == 0 else "none"))
        # ---- G4: 16 rays of config[1]'s launch set in setting d (IGRF base field, T04_s in B0)
        P, D, W = wl.launch_set(100_000, 2)
        pick = np.arange(16) * 6247
        pos0, dir0, w0 = P[pick], D[pick], W[pick]
        g["run_pos0"], g["run_dir0"], g["run_w0"] = pos0, dir0, w0
        runkw = {"fixed": dict(fixedstep=1, dt0=1e-3, dtmax=0.1, tmax=10.0, maxerr=5e-4, maxsteps=5, minalt=wl.MINALT, del_=DEL),
                 "adaptive": dict(fixedstep=0, dt0=1e-3, dtmax=0.05, tmax=0.6, maxerr=5e-4, maxsteps=6, minalt=wl.MINALT, del_=DEL)}
        states = {}
        for mode, kw in runkw.items():
            extra = ["--%s=%r" % (k.rstrip("_"), v) for k, v in kw.items()]
            g["run_%s_params" % mode] = np.array([kw[k] for k in ("fixedstep", "dt0", "dtmax", "tmax", "maxerr", "maxsteps", "minalt", "del_")], dtype=np.float64)
            for tag, p0 in (("", pos0), ("_shift", pos0 * (1.0 + 1e-9))):
                inp = np.concatenate([p0, dir0, w0[:, None]], axis=1)
                rows_all = read_runs(call(exe, tmp, "run", inp, flags(SETTINGS[3]) + extra), len(inp), NCOL_RUN)
                rows, nrows, stop = pack_runs(rows_all, kw["maxsteps"])
                g["run_%s%s_rows" % (mode, tag)] = rows
                g["run_%s%s_nrows" % (mode, tag)], g["run_%s%s_stop" % (mode, tag)] = nrows, stop
                if mode == "fixed" and tag == "":
                    states = rows_all
            print("G4 %s: stop codes %s, rows %d..%d" % (mode, sorted(set(g["run_%s_stop" % mode].tolist())), g["run_%s_nrows" % mode].min(), g["run_%s_nrows" % mode].max()))
        # ---- G2/G3 at 24 states per setting a, b, d: the rays' launch states and their last fixed-step rows (k = n w / c, root 2)
        C = float(np.sqrt(1.0 / 8.854187817e-12 / (np.pi * 4e-7)))
        st = []
        for i in range(16):
            _, r = states[i]
            for t_ in (0, len(r) - 1):
                st.append(np.concatenate([r[t_, 1:4], r[t_, 10:13] * w0[i] / C, [w0[i]]]))
        st = np.array(st)[:24]
        g["g23_state"] = st
        g["g3_dt"] = np.array(1e-3)
        dt, dl = np.full((len(st), 1), 1e-3), np.full((len(st), 1), DEL)
        for s in (SETTINGS[0], SETTINGS[1], SETTINGS[3]):
            t = s[0]
            g["g2_" + t] = call(exe, tmp, "grad", np.hstack([st, dl]), flags(s), 14)
            g["g3_" + t] = call(exe, tmp, "step", np.hstack([st, dt, dl]), flags(s), 21)
            s2, s3 = np.zeros_like(g["g2_" + t]), np.zeros_like(g["g3_" + t])
            for cols in (slice(0, 3), slice(3, 6)):  # x, then k
                for f in SHIFTS:
                    st2 = st.copy()
                    st2[:, cols] *= f
                    s2 = np.maximum(s2, np.abs(call(exe, tmp, "grad", np.hstack([st2, dl]), flags(s), 14) - g["g2_" + t]))
                    s3 = np.maximum(s3, np.abs(call(exe, tmp, "step", np.hstack([st2, dt, dl]), flags(s), 21) - g["g3_" + t]))
            g["g2_sens_" + t], g["g3_sens_" + t] = s2, s3
            print("G2/G3 %s: %d states" % (t, len(st)))
    out = os.path.join(HERE, "at64thch_golden.npz")
    np.savez_compressed(out, **g)
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))
    assert os.path.getsize(out) < os.path.getsize(os.path.join(HERE, "simple3d_golden.npz"))


if __name__ == "__main__":
    main()
