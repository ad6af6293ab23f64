"""GPU (-m gpu): `raytracer --crossings_in=<.ray> --crossings_surfaces=<file> --crossings_out=<file>` -- the tool mode on a .ray
file the executable itself wrote equals api.crossings on api.read_ray_file of that file; a file without events gives an empty
output and exit code 0; a missing flag is refused by name with exit code 2, a bad surfaces file by name."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from stanford_raytracer_amd import workloads as wl

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "stanford_raytracer_amd", "bin", "raytracer")
R_E = 6371.2e3


def rounded(a):
    """what es24.15e3 keeps of a double"""
    return np.array([float("%.15e" % v) for v in np.ravel(a)]).reshape(np.shape(a))


@pytest.fixture(scope="module")
def rayfile(tmp_path_factory):
    """16 Appendix-B rays through the Ngo model, adaptive, every 4th row kept, written by the executable."""
    d = tmp_path_factory.mktemp("clicx")
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
    meta, rows = [], []
    for ln in open(path).read().split("\n")[:-1]:
        assert len(ln) == 40 + 20 * 24
        meta.append([int(ln[10 * k:10 * k + 10]) for k in range(4)])
        rows.append([float(ln[40 + 24 * k:64 + 24 * k]) for k in range(20)])
    return np.array(meta, dtype=np.int64).reshape(-1, 4), np.array(rows).reshape(-1, 20)


def test_tool_mode_equals_the_api_on_the_same_file(rayfile):
    from stanford_raytracer_amd import api

    d, ray = rayfile
    sf, out = d / "surfaces.txt", d / "events.txt"
    # list-directed: commas or blanks, a Fortran exponent, a real kind (floored), trailing values absent
    sf.write_text("0 %r\n2.0, 0.0\n\n2.7 0.349065850398866d0\n1 2.0 0 0\n3 0.0 0.0 1.0 1.0e5\n" % (1.3 * R_E))
    r = subprocess.run([EXE, "--crossings_in=%s" % ray, "--crossings_surfaces=%s" % sf, "--crossings_out=%s" % out],
                       stdout=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and "5 surfaces" in r.stdout
    api.init(0)
    f = api.read_ray_file(ray)
    offsets = np.concatenate([[0], np.cumsum(f["kept"])]).astype(np.int64)
    surf = [api.sphere(1.3 * R_E), api.maglat(0.0), api.maglat(0.349065850398866), api.lshell(2.0), api.plane((0, 0, 1), 1.0e5)]
    ev, meta = api.crossings(offsets, f["rows"], surf)
    gm, ge = parse_events(str(out))
    assert len(meta) == len(gm) > 20 and len(set(meta[:, 1].tolist())) == 5
    assert np.array_equal(gm[:, 0], f["raynum"][meta[:, 0]]) and np.array_equal(gm[:, 1], meta[:, 1] + 1)
    assert np.array_equal(gm[:, 2], meta[:, 2] + 1) and np.array_equal(gm[:, 3], meta[:, 3])
    assert np.array_equal(ge, rounded(ev))  # as es24.15e3 keeps it
    # the same through the writer of the API
    out2 = d / "events_api.txt"
    api.write_crossings_file(str(out2), f["raynum"][meta[:, 0]], meta, ev)
    assert open(out2, "rb").read() == open(out, "rb").read()


def test_a_file_without_events_gives_an_empty_output(rayfile):
    d, ray = rayfile
    sf, out = d / "far.txt", d / "none.txt"
    sf.write_text("0 1e12\n")
    r = subprocess.run([EXE, "--crossings_in=%s" % ray, "--crossings_surfaces=%s" % sf, "--crossings_out=%s" % out],
                       stdout=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and " 0 crossings" in r.stdout
    assert os.path.exists(out) and os.path.getsize(out) == 0


def test_missing_flags_and_bad_files_are_refused_by_name(rayfile):
    d, ray = rayfile
    sf = d / "one.txt"
    sf.write_text("0 7e6\n")
    flags = {"crossings_in": ray, "crossings_surfaces": str(sf), "crossings_out": str(d / "x.txt")}
    for missing in flags:
        cmd = [EXE] + ["--%s=%s" % (k, v) for k, v in flags.items() if k != missing]
        r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True, timeout=120)
        assert r.returncode == 2 and "--%s=" % missing in r.stderr, (missing, r.stderr)

    def run(surfaces_text=None, **over):
        f = dict(flags, **over)
        if surfaces_text is not None:
            bad = d / "bad.txt"
            bad.write_text(surfaces_text)
            f["crossings_surfaces"] = str(bad)
        return subprocess.run([EXE] + ["--%s=%s" % kv for kv in f.items()], stderr=subprocess.PIPE, text=True, timeout=120)

    r = run(crossings_surfaces=str(d / "absent.txt"))
    assert r.returncode == 1 and "crossings_surfaces" in r.stderr and "absent.txt" in r.stderr
    r = run("0 7e6\nsphere 7e6\n")
    assert r.returncode == 1 and "bad.txt, line 2" in r.stderr
    r = run("3 1 0 0 5 6\n")
    assert r.returncode == 1 and "bad.txt, line 1" in r.stderr
    r = run("\n\n")
    assert r.returncode == 1 and "holds 0 surfaces" in r.stderr
    r = run("0 7e6\n" * 17)
    assert r.returncode == 1 and "holds 17 surfaces" in r.stderr
    r = run("0 7e6\n5 1.0\n")
    assert r.returncode == 1 and "surface 1: unknown kind 5" in r.stderr
    r = run("2 1.6\n")
    assert r.returncode == 1 and "not below pi/2" in r.stderr
    r = run(crossings_in=str(d / "absent.ray"))
    assert r.returncode == 1 and "crossings_in" in r.stderr and "absent.ray" in r.stderr
