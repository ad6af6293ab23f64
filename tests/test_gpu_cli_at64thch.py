"""GPU (-m gpu): `raytracer --modelnum=7` -- the driver's own flags for AT64ThCh_adapter (raytracer_driver.f95:1024-1136): the
.ray records of a three-species model against the library's rows, and the refusal by name of a missing --gcpm_kp, of a missing
T04_s parameter (needed even with --use_tsyganenko=0: the model's field-line trace runs through T04_s) and of a --gcpm_kp that
is not an integer."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from stanford_raytracer_amd import workloads as wl

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "stanford_raytracer_amd", "bin", "raytracer")
PARMOD = dict(Pdyn=1.7, Dst=-25.0, ByIMF=1.5, BzIMF=-4.0, W1=0.4, W2=0.5, W3=0.3, W4=0.3, W5=0.4, W6=0.6)
MODEL = ["--modelnum=7", "--gcpm_kp=2", "--yearday=2012180", "--milliseconds_day=43200000", "--use_tsyganenko=0", "--use_igrf=0"] + \
        ["--tsyganenko_%s=%r" % kv for kv in PARMOD.items()]
RUN = ["--outputper=1", "--dt0=0.001", "--dtmax=0.05", "--tmax=0.3", "--root=2", "--fixedstep=1", "--maxerr=5e-4", "--maxsteps=4",
       "--minalt=%r" % wl.MINALT, "--first_attempt_policy=0"]


def rounded(a):
    """what es24.15e3 keeps of a double"""
    return np.array([float("%.15e" % v) for v in np.ravel(a)]).reshape(np.shape(a))


def parse_ray_file_3(path):
    """A .ray file of a three-species model (raytracer_driver.f95:1197-1217): records of 32 columns = raynum, stopcond, t, pos3,
    vprel3, vgrel3, n3, B03, w, nspec, qs3, ms3, Ns3, nus3."""
    rows = []
    for line in open(path):
        assert len(line.rstrip("\n")) == 10 + 10 + 17 * 24 + 10 + 12 * 24
        head = [int(line[0:10]), int(line[10:20])]
        vals = [float(line[20 + 24 * i:44 + 24 * i]) for i in range(17)]
        nspec = int(line[428:438])
        tail = [float(line[438 + 24 * i:462 + 24 * i]) for i in range(12)]
        rows.append(head + vals + [nspec] + tail)
    return np.array(rows)


def test_cli_ray_file_equals_the_api_rows(tmp_path):
    from stanford_raytracer_amd import api
    api.init(0)
    pos, d, w = wl.launch_set(4, 5)
    rf, out = tmp_path / "rays.txt", tmp_path / "out.ray"
    wl.write_rays_file(str(rf), pos, d, w)
    subprocess.run([EXE] + RUN + ["--inputraysfile=%s" % rf, "--outputfile=%s" % out] + MODEL, check=True, timeout=120)
    rec = parse_ray_file_3(str(out))
    assert rec.shape[1] == 32
    m = api.Model.at64thch(2, list(PARMOD.values()), yearday=2012180, msec=43200000)
    p = api.make_params(dt0=1e-3, dtmax=0.05, tmax=0.3, maxerr=5e-4, maxsteps=4, minalt=wl.MINALT, fixedstep=1, outputper=1,
                        del_=1e-4, first_attempt_policy=0)    # del = delSP, the driver's step for this model (:1189-1194)
    p2, d2, w2 = api.read_rays_file(str(rf))
    rows, nrows, stop, _ = m.trace(p2, d2, w2, params=p)
    qs, ms = m.species()
    k = 0
    for r in range(len(w)):
        kept = nrows[r]
        mine = rec[k:k + kept]
        k += kept
        assert np.all(mine[:, 0] == r + 1) and np.all(mine[:, 1] == stop[r])
        assert np.array_equal(mine[:, 2:18], rounded(rows[r, :kept, 0:16]))      # t pos vprel vgrel n B0
        assert np.array_equal(mine[:, 26:29], rounded(rows[r, :kept, 16:19]))    # Ns
        assert np.all(mine[:, 19] == 3) and np.array_equal(mine[0, 20:23], rounded(qs[:3])) and np.array_equal(mine[0, 23:26], rounded(ms[:3]))
    assert k == len(rec) and k > len(w)


def test_cli_refuses_missing_and_non_integer_flags_by_name(tmp_path):
    rf = tmp_path / "rays.txt"
    pos, d, w = wl.launch_set(2, 5)
    wl.write_rays_file(str(rf), pos, d, w)
    cmd = [EXE] + RUN + ["--inputraysfile=%s" % rf, "--outputfile=%s" % (tmp_path / "o.ray")]
    r = subprocess.run(cmd + [f for f in MODEL if not f.startswith("--gcpm_kp")], stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 2 and "--gcpm_kp" in r.stderr
    r = subprocess.run(cmd + [f for f in MODEL if not f.startswith("--tsyganenko_Pdyn")], stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 2 and "--tsyganenko_Pdyn" in r.stderr
    r = subprocess.run(cmd + [f.replace("--gcpm_kp=2", "--gcpm_kp=4.5") for f in MODEL], stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 2 and "--gcpm_kp" in r.stderr and "integer" in r.stderr
    # the refusal of what is not on the accelerated path keeps its exit code and names the models that are
    for num in ("5", "2"):
        r = subprocess.run(cmd + ["--modelnum=" + num, "--yearday=2010001", "--milliseconds_day=0"], stderr=subprocess.PIPE, text=True, timeout=120)
        assert r.returncode == 2 and "1, 3, 4 and 6" in r.stderr and "7" in r.stderr
