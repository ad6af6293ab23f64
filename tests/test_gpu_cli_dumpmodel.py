"""GPU (-m gpu): `raytracer --dumpmodel=1` -- the reference's dumpmodel flags, the file it writes against Model.dump of the same
settings and against the golden's header bytes, --mag_coords for the models that read it and for one that does not, and the
refusals."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN_DIR, ROOT

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "stanford_raytracer_amd", "bin", "raytracer")
NAMES = ("minx", "maxx", "miny", "maxy", "minz", "maxz")


def settings(name):
    return json.load(open(os.path.join(GOLDEN_DIR, "dumpmodel_settings.json")))[name]


def printed(a):
    """what es24.15e3 keeps of a double"""
    return np.array([float("%.15e" % v) for v in np.ravel(a)]).reshape(np.shape(a))


def run_cli(st, out, extra=(), n=None, drop=()):
    n = n or ["--nx=%d" % st["n"][0], "--ny=%d" % st["n"][1], "--nz=%d" % st["n"][2]]
    cmd = [EXE, "--dumpmodel=1", "--filename=%s" % out, "--modelnum=%d" % st["modelnum"], "--yearday=%d" % st["yearday"],
           "--milliseconds_day=%d" % st["milliseconds_day"], *n, *["--%s=%.17e" % kv for kv in zip(NAMES, st["bounds"])],
           *[f for f in st["flags"] if not f.startswith("--mag_coords")], *extra]
    cmd = [c for c in cmd if not c.startswith(tuple(drop))] if drop else cmd
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)


def head(path):
    with open(path, "rb") as f:
        return f.readline() + f.readline()


def test_cli_dump_of_model_1_equals_the_library(tmp_path, cfgfiles):
    from stanford_raytracer_amd import api

    api.init(0)
    st = settings("dump_ngo_5x1x4")
    out = str(tmp_path / "ngo.txt")
    # counts are read as reals and floored: 5.0 and 4.9 are 5 and 4
    r = run_cli(st, out, ["--ngo_configfile=" + cfgfiles["ngo"]], n=["--nx=5.0", "--ny=1", "--nz=4.9"])
    assert r.returncode == 0, r.stderr
    d = api.read_dump_file(out)
    f = api.Model.ngo(cfgfiles["ngo"], st["yearday"], st["milliseconds_day"]).dump(5, 1, 4, st["bounds"])
    assert d["f"].shape == (4, 1, 5, 19) and np.array_equal(d["f"], printed(f))
    assert head(out) == head(os.path.join(GOLDEN_DIR, st["file"]))
    # the flag is not read for this model: the SM dump, and a notice
    out2 = str(tmp_path / "ngo_mag.txt")
    r = run_cli(st, out2, ["--ngo_configfile=" + cfgfiles["ngo"], "--mag_coords=1"])
    assert r.returncode == 0 and "--mag_coords" in r.stderr and "ignored" in r.stderr
    assert open(out2, "rb").read() == open(out, "rb").read()


def test_cli_dump_of_model_6_sm_and_mag(tmp_path):
    from stanford_raytracer_amd import api

    api.init(0)
    st = settings("dump_simple3d_sm_6x1x5")
    m = api.Model.simple3d(4.0, st["yearday"], st["milliseconds_day"])
    files = {}
    for tag, extra, mag in (("absent", [], False), ("sm", ["--mag_coords=0"], False), ("mag", ["--mag_coords=1"], True)):
        out = str(tmp_path / (tag + ".txt"))
        r = run_cli(st, out, extra)
        assert r.returncode == 0 and "ignored" not in r.stderr, r.stderr
        d = api.read_dump_file(out)
        assert np.array_equal(d["f"], printed(m.dump(*st["n"], st["bounds"], mag_coords=mag)))
        assert head(out) == head(os.path.join(GOLDEN_DIR, st["file"]))
        files[tag] = open(out, "rb").read()
    assert files["absent"] == files["sm"] != files["mag"]  # an absent --mag_coords is 0


def test_cli_refusals(tmp_path, cfgfiles):
    st = settings("dump_ngo_5x1x4")
    out = str(tmp_path / "x.txt")
    r = run_cli(st, out, ["--ngo_configfile=" + cfgfiles["ngo"]], drop=("--filename",))
    assert r.returncode == 2 and "--filename" in r.stderr
    r = run_cli(st, out, ["--ngo_configfile=" + cfgfiles["ngo"]], n=["--nx=0", "--ny=1", "--nz=4"])
    assert r.returncode == 2 and "--nx" in r.stderr
    st5 = dict(st, modelnum=5)
    r = run_cli(st5, out, ["--ngo_configfile=" + cfgfiles["ngo"], "--kp=4"])
    assert r.returncode == 2 and "1, 3, 4 and 6" in r.stderr  # today's refusal, in this mode as in every other
    assert not os.path.exists(out)
