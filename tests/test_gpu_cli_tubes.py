"""GPU (-m gpu): `raytracer --tube_in=<.ray> --tube_neighbours=<file> --tube_out=<file>` -- the tool mode on a .ray file the
executable itself wrote equals api.tubes on api.read_ray_file of that file, as es24.15e3 keeps it, and api.write_tubes_file writes
the same bytes; a missing flag, an absent or malformed file, a ray number the .ray file does not hold and a centre listed twice are
refused by name with exit code 2."""
import os
import subprocess

import numpy as np
import pytest

import tubes_cases as tc
from conftest import ROOT
from stanford_raytracer_amd import workloads as wl

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "stanford_raytracer_amd", "bin", "raytracer")


@pytest.fixture(scope="module")
def rayfile(tmp_path_factory):
    """The 16 Appendix-B rays and their companions (api.tube_fan, 50 km) through the Ngo model, adaptive (every ray has its own
    time stamps), every 4th row kept, written by the executable."""
    from stanford_raytracer_amd import api

    d = tmp_path_factory.mktemp("clitb")
    cfg, rf, out = d / "newray.in", d / "rays.txt", d / "out.ray"
    cfg.write_text(wl.NEWRAY_PLASMAPAUSE)
    pos, dr, w, nb = api.tube_fan(*wl.appendix_b_rays(), delta_pos=50e3)
    wl.write_rays_file(str(rf), pos, dr, w)
    cmd = [EXE, "--modelnum=1", "--ngo_configfile=%s" % cfg, "--yearday=2010001", "--milliseconds_day=0", "--outputper=4",
           "--dt0=0.001", "--dtmax=0.1", "--tmax=1.0", "--root=2", "--fixedstep=0", "--maxerr=5e-4", "--maxsteps=400",
           "--minalt=%r" % wl.MINALT, "--inputraysfile=%s" % rf, "--outputfile=%s" % out]
    subprocess.run(cmd, check=True, timeout=120)
    return d, str(out), nb


def test_tool_mode_equals_the_api_on_the_same_file(rayfile):
    from stanford_raytracer_amd import api

    d, ray, nb = rayfile
    nf, out = d / "nb.txt", d / "tubes.txt"
    api.init(0)
    f = api.read_ray_file(ray)
    assert len(f["kept"]) == len(nb)
    offsets = np.concatenate([[0], np.cumsum(f["kept"])]).astype(np.int64)
    num = f["raynum"]
    # list-directed: commas or blanks, an empty line
    lines = ["%d %d %d" % (num[a], num[nb[a, 0]], num[nb[a, 1]]) for a in range(len(nb)) if nb[a, 0] >= 0]
    lines[0] = lines[0].replace(" ", ", ")
    nf.write_text("\n".join(lines[:3]) + "\n\n" + "\n".join(lines[3:]) + "\n")
    r = subprocess.run([EXE, "--tube_in=%s" % ray, "--tube_neighbours=%s" % nf, "--tube_out=%s" % out], stdout=subprocess.PIPE,
                       text=True, timeout=120)
    assert r.returncode == 0 and "%d tubes" % len(lines) in r.stdout, r.stdout
    section, flag = api.tubes(offsets, f["rows"], nb)
    got = tc.parse_tubes_file(str(out))
    want = [(int(num[a]), j - int(offsets[a]) + 1, int(flag[j]), [f["rows"][j, 0]] + section[j].tolist())
            for a in range(len(nb)) for j in range(int(offsets[a]), int(offsets[a + 1])) if flag[j] != 1]
    assert len(got) == len(want) == int(np.sum(f["kept"][0::3])) and "%d sections" % len(want) in r.stdout
    nok = sum(1 for g in got if g[2] == 0)
    assert nok > len(got) // 2 and "(%d ok)" % nok in r.stdout  # (the rest: the rows of a centre that outlives a neighbour)
    for g, w in zip(got, want):
        assert g[:3] == w[:3]
        assert all((np.isnan(a) and np.isnan(b)) or a == tc.es24(b) for a, b in zip(g[3], w[3])), (g, w)
    # the same through the writer of the API
    out2 = d / "tubes_api.txt"
    api.write_tubes_file(str(out2), num, offsets, f["rows"], section, flag)
    assert open(out2, "rb").read() == open(out, "rb").read()


def test_missing_flags_and_bad_files_are_refused_by_name(rayfile):
    from stanford_raytracer_amd import api

    d, ray, _ = rayfile
    num = api.read_ray_file(ray)["raynum"]
    a, b, c, e = (int(v) for v in num[:4])
    nf = d / "one.txt"
    nf.write_text("%d %d %d\n" % (a, b, c))
    flags = {"tube_in": ray, "tube_neighbours": str(nf), "tube_out": str(d / "x.txt")}
    for missing in flags:
        cmd = [EXE] + ["--%s=%s" % (k, v) for k, v in flags.items() if k != missing]
        r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True, timeout=120)
        assert r.returncode == 2 and "--%s=" % missing in r.stderr, (missing, r.stderr)

    def run(text=None, **over):
        f = dict(flags, **over)
        if text is not None:
            bad = d / "bad.txt"
            bad.write_text(text)
            f["tube_neighbours"] = str(bad)
        return subprocess.run([EXE] + ["--%s=%s" % kv for kv in f.items()], stderr=subprocess.PIPE, text=True, timeout=120)

    r = run(tube_neighbours=str(d / "absent.txt"))
    assert r.returncode == 2 and "tube_neighbours" in r.stderr and "absent.txt" in r.stderr
    r = run(tube_in=str(d / "absent.ray"))
    assert r.returncode == 2 and "tube_in" in r.stderr and "absent.ray" in r.stderr
    r = run("%d %d %d\nhere %d %d\n" % (a, b, c, b, c))
    assert r.returncode == 2 and "bad.txt, line 2" in r.stderr
    r = run("%d %d\n" % (a, b))
    assert r.returncode == 2 and "bad.txt, line 1" in r.stderr
    r = run("%d %d %d %d\n" % (a, b, c, e))
    assert r.returncode == 2 and "bad.txt, line 1" in r.stderr
    r = run("%d %d %d\n" % (a, b, int(num.max()) + 5))
    assert r.returncode == 2 and "holds no ray number %d" % (int(num.max()) + 5) in r.stderr, r.stderr
    r = run("%d %d 2.5\n" % (a, b))
    assert r.returncode == 2 and "holds no ray number 2.5" in r.stderr
    r = run("%d %d %d\n%d %d %d\n" % (a, b, c, a, c, e))
    assert r.returncode == 2 and "tube 2: centre %d is listed twice" % a in r.stderr
    r = run("%d %d %d\n" % (a, b, b))
    assert r.returncode == 2 and "three different rays" in r.stderr
