"""GPU (-m gpu): bin/raytracer --interp_layout=expanded|nodes|auto on the inputs of tests/test_gpu_cli.py's adaptive modelnum-3
run (the 16^3 grid, the 16 Appendix-B rays).  The node table's .ray file against the expanded layout's: record count and stop
codes equal, positions within SURVEY A-9's curve tolerance (1e-3, the floor of the adaptive trajectory rung and the bar
tests/test_gpu_cli.py holds its records to); whether the two files are byte-identical is printed.

The files are expected to be byte-identical (printed, not asserted): an adaptive run splits its step sequence on the first
last-bit difference, so equal record counts need the two layouts' trace kernels to be bit-equal, which they are
(HISTORY section 22: before the node-table lookups ended in a memory clobber, 488 records against 506)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, parse_ray_file, vrel
from stanford_raytracer_amd import workloads as wl

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "stanford_raytracer_amd", "bin", "raytracer")


@pytest.fixture(scope="module")
def inputs(tmp_path_factory, grid16):
    d = tmp_path_factory.mktemp("cli_layout")
    F, b, qs, ms = grid16
    gf, rf = str(d / "grid16.txt"), str(d / "rays.txt")
    wl.write_grid_file(gf, F, b, qs, ms)
    p0, d0, w0 = wl.appendix_b_rays()
    wl.write_rays_file(rf, p0, d0, w0)
    return d, gf, rf


def command(gf, rf, out, *extra):
    return [EXE, "--outputper=16", "--tmax=0.2", "--fixedstep=0", "--modelnum=3", "--first_attempt_policy=0",
            "--interp_interpfile=%s" % gf, "--dt0=0.001", "--dtmax=0.1", "--root=2", "--maxerr=5e-4", "--maxsteps=2000",
            "--minalt=%r" % wl.MINALT, "--inputraysfile=%s" % rf, "--outputfile=%s" % out, "--yearday=2010001",
            "--milliseconds_day=0", "--use_tsyganenko=0", "--use_igrf=0"] + list(extra)


def test_the_layout_flag(inputs):
    d, gf, rf = inputs
    files = {}
    for name, flag in (("default", []), ("expanded", ["--interp_layout=expanded"]), ("nodes", ["--interp_layout=nodes"]),
                       ("auto", ["--interp_layout=auto"])):
        files[name] = str(d / (name + ".ray"))
        subprocess.run(command(gf, rf, files[name], *flag), check=True)
    raw = {k: open(v, "rb").read() for k, v in files.items()}
    assert raw["default"] == raw["expanded"] == raw["auto"] and len(raw["default"]) > 0  # (16^3: auto = expanded)
    print("FIGURE CLI .ray files of the two layouts byte-identical: %s" % (raw["nodes"] == raw["expanded"]))
    a, e = parse_ray_file(files["nodes"]), parse_ray_file(files["expanded"])
    assert a.shape == e.shape and np.array_equal(a[:, 0:2], e[:, 0:2])  # record count; ray numbers and stop codes
    assert np.array_equal(a[:, 18:28], e[:, 18:28])                    # w, nspec, qs, ms
    assert vrel(a[:, 3:6], e[:, 3:6]).max() <= 1e-3 and np.allclose(a[:, 2], e[:, 2], rtol=1e-3, atol=0)
    assert np.max(np.abs(a[:, 28:32] - e[:, 28:32]) / e[:, 28:32]) <= 1e-2  # Ns along the paths


def test_an_unknown_layout_is_refused_with_the_flags_name(inputs):
    d, gf, rf = inputs
    out = str(d / "bogus.ray")
    r = subprocess.run(command(gf, rf, out, "--interp_layout=bogus"), capture_output=True, text=True)
    assert r.returncode != 0 and "--interp_layout=bogus" in r.stderr
