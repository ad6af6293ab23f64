"""GPU (-m gpu): `raytracer --approach_in=<.ray> --approach_observers=<file> --approach_out=<file>` -- the tool mode on a .ray file
the executable itself wrote equals api.approaches on api.read_ray_file of that file, and api.write_approaches_file writes the same
bytes; a file without events gives an empty output and exit code 0; a missing flag is refused by name with exit code 2, a bad
observers file by name with exit code 1."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from stanford_raytracer_amd import workloads as wl

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "stanford_raytracer_amd", "bin", "raytracer")


def rounded(a):
    """what es24.15e3 keeps of a double"""
    return np.array([float("%.15e" % v) for v in np.ravel(a)]).reshape(np.shape(a))


@pytest.fixture(scope="module")
def rayfile(tmp_path_factory):
    """16 Appendix-B rays through the Ngo model, adaptive, every 4th row kept, written by the executable."""
    d = tmp_path_factory.mktemp("cliap")
    cfg, rf, out = d / "newray.in", d / "rays.txt", d / "out.ray"
    cfg.write_text(wl.NEWRAY_PLASMAPAUSE)
    pos, dr, w = wl.appendix_b_rays()
    wl.write_rays_file(str(rf), pos, dr, w)
    cmd = [EXE, "--modelnum=1", "--ngo_configfile=%s" % cfg, "--yearday=2010001", "--milliseconds_day=0", "--outputper=4",
           "--dt0=0.001", "--dtmax=0.1", "--tmax=1.0", "--root=2", "--fixedstep=0", "--maxerr=5e-4", "--maxsteps=400",
           "--minalt=%r" % wl.MINALT, "--inputraysfile=%s" % rf, "--outputfile=%s" % out]
    subprocess.run(cmd, check=True, timeout=120)
    return d, str(out)


def parse_events(path):
    meta, dist, rows = [], [], []
    for ln in open(path).read().split("\n")[:-1]:
        assert len(ln) == 40 + 21 * 24
        meta.append([int(ln[10 * k:10 * k + 10]) for k in range(4)])
        dist.append(float(ln[40:64]))
        rows.append([float(ln[64 + 24 * k:88 + 24 * k]) for k in range(20)])
    return np.array(meta, dtype=np.int64).reshape(-1, 4), np.array(dist), np.array(rows).reshape(-1, 20)


def observers_of(f):
    """beside the middle of two intervals of every ray of the file: 30 km off along z, radius 100 km"""
    offsets = np.concatenate([[0], np.cumsum(f["kept"])]).astype(np.int64)
    obs = []
    for r in range(len(f["kept"])):
        for i in sorted({int(f["kept"][r]) // 3, (2 * int(f["kept"][r])) // 3} - {int(f["kept"][r]) - 1}):
            a, b = f["rows"][offsets[r] + i], f["rows"][offsets[r] + i + 1]
            obs.append(np.concatenate([0.5 * (a[1:4] + b[1:4]) + [0.0, 0.0, 30e3], [100e3]]))
    return offsets, np.array(obs)


def test_tool_mode_equals_the_api_on_the_same_file(rayfile):
    from stanford_raytracer_amd import api

    d, ray = rayfile
    of, out = d / "observers.txt", d / "events.txt"
    api.init(0)
    f = api.read_ray_file(ray)
    offsets, obs = observers_of(f)
    # list-directed: commas or blanks, a Fortran exponent, an empty line
    lines = [" ".join(repr(float(v)) for v in o) for o in obs]
    lines[0] = ", ".join(repr(float(v)) for v in obs[0])
    lines[1] = " ".join(("%.17e" % v).replace("e", "d") for v in obs[1])
    of.write_text("\n".join(lines[:3]) + "\n\n" + "\n".join(lines[3:]) + "\n")
    r = subprocess.run([EXE, "--approach_in=%s" % ray, "--approach_observers=%s" % of, "--approach_out=%s" % out],
                       stdout=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and "%d observers" % len(obs) in r.stdout
    ev, meta, dist = api.approaches(obs, offsets, f["rows"])
    gm, gd, ge = parse_events(str(out))
    assert len(meta) == len(gm) >= len(f["kept"]) and "%d approaches" % len(meta) in r.stdout
    assert len(set(meta[:, 0].tolist())) == len(f["kept"]) and len(set(meta[:, 1].tolist())) > len(f["kept"]) and np.all(dist > 0.0)
    assert np.array_equal(gm[:, 0], f["raynum"][meta[:, 0]]) and np.array_equal(gm[:, 1], meta[:, 1] + 1)
    assert np.array_equal(gm[:, 2], meta[:, 2] + 1) and not gm[:, 3].any()
    assert np.array_equal(ge, rounded(ev)) and np.array_equal(gd, rounded(dist))  # as es24.15e3 keeps them
    # the same through the writer of the API
    out2 = d / "events_api.txt"
    api.write_approaches_file(str(out2), f["raynum"][meta[:, 0]], meta, dist, ev)
    assert open(out2, "rb").read() == open(out, "rb").read()


def test_a_file_without_events_gives_an_empty_output(rayfile):
    d, ray = rayfile
    of, out = d / "far.txt", d / "none.txt"
    of.write_text("1e12 0 0 1.0\n")
    r = subprocess.run([EXE, "--approach_in=%s" % ray, "--approach_observers=%s" % of, "--approach_out=%s" % out],
                       stdout=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and " 0 approaches" in r.stdout
    assert os.path.exists(out) and os.path.getsize(out) == 0


def test_missing_flags_and_bad_files_are_refused_by_name(rayfile):
    d, ray = rayfile
    of = d / "one.txt"
    of.write_text("7e6 0 0 1e5\n")
    flags = {"approach_in": ray, "approach_observers": str(of), "approach_out": str(d / "x.txt")}
    for missing in flags:
        cmd = [EXE] + ["--%s=%s" % (k, v) for k, v in flags.items() if k != missing]
        r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True, timeout=120)
        assert r.returncode == 2 and "--%s=" % missing in r.stderr, (missing, r.stderr)

    def run(observers_text=None, **over):
        f = dict(flags, **over)
        if observers_text is not None:
            bad = d / "bad.txt"
            bad.write_text(observers_text)
            f["approach_observers"] = str(bad)
        return subprocess.run([EXE] + ["--%s=%s" % kv for kv in f.items()], stderr=subprocess.PIPE, text=True, timeout=120)

    r = run(approach_observers=str(d / "absent.txt"))
    assert r.returncode == 1 and "approach_observers" in r.stderr and "absent.txt" in r.stderr
    r = run("7e6 0 0 1e5\nhere 0 0 1e5\n")
    assert r.returncode == 1 and "bad.txt, line 2" in r.stderr
    r = run("7e6 0 0\n")
    assert r.returncode == 1 and "bad.txt, line 1" in r.stderr
    r = run("7e6 0 0 1e5 3\n")
    assert r.returncode == 1 and "bad.txt, line 1" in r.stderr
    r = run("\n\n")
    assert r.returncode == 1 and "holds 0 observers" in r.stderr
    r = run("7e6 0 0 1e5\n" * 65537)
    assert r.returncode == 1 and "holds 65537 observers" in r.stderr
    r = run("7e6 0 0 1e5\n7e6 0 0 0\n")
    assert r.returncode == 1 and "observer 1: radius 0 is not finite and > 0" in r.stderr
    r = run("7e6 0 0 1e5\n7e6 nan 0 1\n")
    assert r.returncode == 1 and "observer 1: coordinate x[1] is not finite" in r.stderr
    r = run(approach_in=str(d / "absent.ray"))
    assert r.returncode == 1 and "approach_in" in r.stderr and "absent.ray" in r.stderr
