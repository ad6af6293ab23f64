"""GPU (-m gpu): `raytracer --modelnum=6` -- the driver's own flags for simple_3d_model_adapter (raytracer_driver.f95:893-992),
the refusal of a missing required flag by name, and the grid builder with the model-6 handle as its source."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, parse_ray_file
from stanford_raytracer_amd import workloads as wl

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "stanford_raytracer_amd", "bin", "raytracer")
MODEL = ["--modelnum=6", "--kp=4.0", "--yearday=2010001", "--milliseconds_day=0", "--use_tsyganenko=0", "--use_igrf=0",
         "--fixed_MLT=1", "--MLT=2.0", "--ngo_configfile=ignored.in"]


def rounded(a):
    """what es24.15e3 keeps of a double"""
    return np.array([float("%.15e" % v) for v in np.ravel(a)]).reshape(np.shape(a))


def test_cli_ray_file_equals_the_api_rows(tmp_path):
    from stanford_raytracer_amd import api
    api.init(0)
    pos, d, w = wl.launch_set(24, 5)
    rf, out = tmp_path / "rays.txt", tmp_path / "out.ray"
    wl.write_rays_file(str(rf), pos, d, w)
    cmd = [EXE, "--outputper=4", "--dt0=0.001", "--dtmax=0.05", "--tmax=0.3", "--root=2", "--fixedstep=0", "--maxerr=5e-4",
           "--maxsteps=40", "--minalt=%r" % wl.MINALT, "--first_attempt_policy=0", "--inputraysfile=%s" % rf,
           "--outputfile=%s" % out] + MODEL
    subprocess.run(cmd, check=True, timeout=120)
    rec = parse_ray_file(str(out))
    m = api.Model.simple3d(4.0, yearday=2010001, msec=0, fixed_mlt=2.0)
    p = api.make_params(dt0=1e-3, dtmax=0.05, tmax=0.3, maxerr=5e-4, maxsteps=40, minalt=wl.MINALT, fixedstep=0, outputper=4,
                        del_=1e-6, first_attempt_policy=0)    # del = delDP, the driver's step for this model (:1188)
    # the rays as the CLI read them from the text file
    p2, d2, w2 = api.read_rays_file(str(rf))
    rows, nrows, stop, _ = m.trace(p2, d2, w2, params=p)
    qs, ms = m.species()
    k = 0
    for r in range(len(w)):
        kept = (nrows[r] - 1) // 4 + 1
        mine = rec[k:k + kept]
        k += kept
        assert np.all(mine[:, 0] == r + 1) and np.all(mine[:, 1] == stop[r])
        assert np.array_equal(mine[:, 2:18], rounded(rows[r, :kept, 0:16]))      # t pos vprel vgrel n B0
        assert np.array_equal(mine[:, 28:32], rounded(rows[r, :kept, 16:20]))    # Ns
        assert np.all(mine[:, 19] == 4) and np.array_equal(mine[0, 20:24], rounded(qs)) and np.array_equal(mine[0, 24:28], rounded(ms))
    assert k == len(rec) and k > len(w)


def test_cli_refuses_a_missing_kp_by_name(tmp_path):
    rf = tmp_path / "rays.txt"
    pos, d, w = wl.launch_set(2, 5)
    wl.write_rays_file(str(rf), pos, d, w)
    cmd = [EXE, "--outputper=1", "--dt0=0.001", "--dtmax=0.05", "--tmax=0.1", "--root=2", "--fixedstep=0", "--maxerr=5e-4",
           "--maxsteps=10", "--minalt=%r" % wl.MINALT, "--inputraysfile=%s" % rf, "--outputfile=%s" % (tmp_path / "o.ray")]
    r = subprocess.run(cmd + [f for f in MODEL if not f.startswith("--kp")], stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 2 and "--kp" in r.stderr
    r = subprocess.run(cmd + [f for f in MODEL if not f.startswith("--MLT")], stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 2 and "--MLT" in r.stderr
    r = subprocess.run(cmd + ["--modelnum=5", "--yearday=2010001", "--milliseconds_day=0"], stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 2 and "1, 3, 4 and 6" in r.stderr


def test_cli_buildgrid_with_model_6_writes_a_readable_grid(tmp_path):
    from stanford_raytracer_amd import api
    api.init(0)
    gf = tmp_path / "grid6.txt"
    b = np.array([1.3, 4.5, -2.0, 2.5, -1.5, 1.8]) * wl.R_E
    names = ["minx", "maxx", "miny", "maxy", "minz", "maxz"]
    cmd = [EXE, "--buildgrid=1", "--filename=%s" % gf, "--nx=6", "--ny=5", "--nz=4", "--compder=0"] + \
          ["--%s=%r" % (n, float(v)) for n, v in zip(names, b)] + MODEL
    subprocess.run(cmd, check=True, timeout=120)
    t = api.Model.interp_file(str(gf))
    assert t.kind == 3 and t.nspec == 4
    src = api.Model.simple3d(4.0, yearday=2010001, msec=0, fixed_mlt=2.0)
    F, _ = src.build_grid(6, 5, 4, b)
    node = np.array([[b[0], b[2], b[4]], [b[1], b[3], b[5]]])
    got = np.log(t.plasma_params(node)[:, 4:8])
    assert np.abs(got[0] - F[0, 0, 0]).max() <= 1e-12 * np.abs(F).max() and np.abs(got[1] - F[-1, -1, -1]).max() <= 1e-12 * np.abs(F).max()
