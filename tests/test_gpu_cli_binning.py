"""GPU (-m gpu): `raytracer --bin_in=<.ray> --bin_axes=<file> --bin_out=<file> [--bin_nsub=..] [--bin_quantum=..]` -- the tool mode
on a .ray file the executable itself wrote equals api.bin_rays on api.read_ray_file of that file, and api.write_bin_file writes
the same bytes; named and numeric kinds, commas and d exponents are accepted; a missing flag, a malformed axes file, --bin_nsub=0
and an absent .ray file are refused by name with exit code 2."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from stanford_raytracer_amd import workloads as wl

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "stanford_raytracer_amd", "bin", "raytracer")
R_E = 6371.2e3


@pytest.fixture(scope="module")
def rayfile(tmp_path_factory):
    """16 Appendix-B rays through the Ngo model, adaptive, every 4th row kept, written by the executable."""
    d = tmp_path_factory.mktemp("clibn")
    cfg, rf, out = d / "newray.in", d / "rays.txt", d / "out.ray"
    cfg.write_text(wl.NEWRAY_PLASMAPAUSE)
    pos, dr, w = wl.appendix_b_rays()
    wl.write_rays_file(str(rf), pos, dr, w)
    cmd = [EXE, "--modelnum=1", "--ngo_configfile=%s" % cfg, "--yearday=2010001", "--milliseconds_day=0", "--outputper=4",
           "--dt0=0.001", "--dtmax=0.1", "--tmax=1.0", "--root=2", "--fixedstep=0", "--maxerr=5e-4", "--maxsteps=400",
           "--minalt=%r" % wl.MINALT, "--inputraysfile=%s" % rf, "--outputfile=%s" % out]
    subprocess.run(cmd, check=True, timeout=120)
    return d, str(out)


def test_tool_mode_equals_the_api_on_the_same_file(rayfile):
    from stanford_raytracer_amd import api

    d, ray = rayfile
    af, out = d / "axes.txt", d / "map.txt"
    le = np.array([1.0, 1.5, 2.0, 2.5, 3.0, 4.0, 6.0])
    se = np.array([-0.9, -0.5, -0.25, 0.0, 0.25, 0.5, 0.9])
    # a named kind and a numeric one (a real, floored), commas, a Fortran exponent, an empty line
    af.write_text("L 6 " + " ".join("%r" % float(v) for v in le) + "\n\n6.0, 6, -0.9d0, -0.5, -2.5d-1, 0.0, 0.25, 0.5, 0.9\n")
    r = subprocess.run([EXE, "--bin_in=%s" % ray, "--bin_axes=%s" % af, "--bin_out=%s" % out, "--bin_nsub=4", "--bin_quantum=1d-9"],
                       stdout=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and "36 cells" in r.stdout
    api.init(0)
    f = api.read_ray_file(ray)
    offsets = np.concatenate([[0], np.cumsum(f["kept"])]).astype(np.int64)
    axes = [api.axis("L", le), api.axis("sinlat", se)]
    m = api.bin_rays(offsets, f["rows"], axes, nsub=4, quantum=1e-9)
    assert " %d intervals used, %d skipped, %d samples deposited, %d outside" % tuple(m["counters"]) in r.stdout
    assert m["counters"][0] > 100 and np.count_nonzero(m["hits"]) > 8
    back = api.read_bin_file(str(out))
    assert back["nsub"] == 4 and back["quantum"] == 1e-9 and [k for k, _ in back["axes"]] == [5, 6]
    assert np.array_equal(back["axes"][0][1], le) and np.array_equal(back["axes"][1][1], se)
    assert np.array_equal(back["hits"], m["hits"])
    assert np.array_equal(back["sum"], np.array([float("%.15e" % v) for v in m["sum"].ravel()]).reshape(m["sum"].shape))  # as es24.15e3 keeps it
    # the same through the writer of the API
    out2 = d / "map_api.txt"
    api.write_bin_file(str(out2), axes, m["ticks"], m["hits"], nsub=4, quantum=1e-9)
    assert open(out2, "rb").read() == open(out, "rb").read()
    # the defaults: nsub 8, quantum 2^-30 s
    r = subprocess.run([EXE, "--bin_in=%s" % ray, "--bin_axes=%s" % af, "--bin_out=%s" % out], stdout=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0
    m8 = api.bin_rays(offsets, f["rows"], axes)
    api.write_bin_file(str(out2), axes, m8["ticks"], m8["hits"])
    assert open(out2, "rb").read() == open(out, "rb").read()


def test_missing_flags_and_bad_files_are_refused_by_name_with_exit_code_2(rayfile):
    d, ray = rayfile
    af = d / "one.txt"
    af.write_text("r 2 0 1e7 1e8\n")
    flags = {"bin_in": ray, "bin_axes": str(af), "bin_out": str(d / "x.txt")}
    for missing in flags:
        cmd = [EXE] + ["--%s=%s" % (k, v) for k, v in flags.items() if k != missing]
        r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True, timeout=120)
        assert r.returncode == 2 and "--%s=" % missing in r.stderr, (missing, r.stderr)

    def run(axes_text=None, **over):
        f = dict(flags, **over)
        if axes_text is not None:
            bad = d / "bad.txt"
            bad.write_text(axes_text)
            f["bin_axes"] = str(bad)
        return subprocess.run([EXE] + ["--%s=%s" % kv for kv in f.items()], stderr=subprocess.PIPE, text=True, timeout=120)

    for text, line, why in (("r 2 0 1e7 1e8\nlat 2 0 1 2\n", 2, "the kind is neither"), ("r 2 0 1e7\n", 1, "n + 1 edges"),
                            ("r 2 0 1e7 1e8 1e9\n", 1, "n + 1 edges"), ("r 2 0 1e7 x\n", 1, "not a number"), ("r\n", 1, "n is not"),
                            ("r 1.5 0 1 2\n", 1, "n is not"), ("r 0 1\n", 1, "n is not"), ("x 1 0 1\ny 1 0 1\nz 1 0 1\nr 1 0 1\n", 4, "a fourth axis")):
        r = run(text)
        assert r.returncode == 2 and "bad.txt, line %d" % line in r.stderr and why in r.stderr, (text, r.stderr)
    r = run("\n\n")
    assert r.returncode == 2 and "holds no axis" in r.stderr
    r = run(bin_axes=str(d / "absent.txt"))
    assert r.returncode == 2 and "bin_axes" in r.stderr and "absent.txt" in r.stderr
    for text, why in (("r 2 0 2e7 1e7\n", "edges do not increase at edge 2"), ("9 1 0 1\n", "axis 0: unknown kind 9"),
                      ("sinlat 1 0 1.5\n", "outside [-1, 1]"), ("mlt 1 0 25\n", "outside [0, 24]")):
        r = run(text)
        assert r.returncode == 2 and why in r.stderr, (text, r.stderr)
    r = run(bin_nsub="0")
    assert r.returncode == 2 and "nsub = 0" in r.stderr
    r = run(bin_nsub="65")
    assert r.returncode == 2 and "nsub = 65" in r.stderr
    r = run(bin_quantum="0")
    assert r.returncode == 2 and "quantum" in r.stderr
    r = run(bin_in=str(d / "absent.ray"))
    assert r.returncode == 2 and "bin_in" in r.stderr and "absent.ray" in r.stderr
    assert not os.path.exists(d / "x.txt")  # nothing was written by any refused call
