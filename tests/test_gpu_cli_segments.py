"""GPU (-m gpu): the executable's --segment_rows.  The adaptive 16-ray model-3 run of tests/test_gpu_cli.py, traced in segments
of 4 kept rows, writes the bytes it writes without the flag -- also across two shards and with a chunk size given."""
import os
import subprocess

import pytest

from conftest import ROOT
from stanford_raytracer_amd import workloads as wl

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "stanford_raytracer_amd", "bin")


@pytest.fixture(scope="module")
def run16(tmp_path_factory, grid16):
    """the command line of test_cli_adaptive_model3_matches_the_reference_drivers_file, less its output file, and its bytes"""
    tmp = tmp_path_factory.mktemp("cliseg")
    F, b, qs, ms = grid16
    gf, rf = tmp / "grid16.txt", tmp / "rays.txt"
    wl.write_grid_file(str(gf), F, b, qs, ms)
    p0, d0, w0 = wl.appendix_b_rays()
    wl.write_rays_file(str(rf), p0, d0, w0)
    cmd = [os.path.join(BIN, "raytracer"), "--outputper=16", "--tmax=0.2", "--fixedstep=0", "--modelnum=3",
           "--first_attempt_policy=0", "--interp_interpfile=%s" % gf, "--dt0=0.001", "--dtmax=0.1", "--root=2", "--maxerr=5e-4",
           "--maxsteps=2000", "--minalt=%r" % wl.MINALT, "--inputraysfile=%s" % rf, "--yearday=2010001",
           "--milliseconds_day=0", "--use_tsyganenko=0", "--use_igrf=0"]
    out = tmp / "plain.ray"
    subprocess.run(cmd + ["--outputfile=%s" % out], check=True)
    plain = out.read_bytes()
    assert plain.count(b"\n") > 16  # more than the launch rows: the rays kept rows behind several segment boundaries
    return tmp, cmd, plain


@pytest.mark.parametrize("extra", [[], ["--devices=0,0"], ["--chunk_rays=64"]], ids=["one", "devices", "chunk"])
def test_segment_rows_writes_the_same_bytes(run16, extra, request):
    tmp, cmd, plain = run16
    out = tmp / ("seg_%s.ray" % request.node.callspec.id)
    r = subprocess.run(cmd + ["--outputfile=%s" % out, "--segment_rows=4"] + extra, check=True, capture_output=True, text=True)
    assert out.read_bytes() == plain
    assert not list(tmp.glob(out.name + ".part*"))
    # the step count the executable reports is the sum over the segments
    base = subprocess.run(cmd + ["--outputfile=%s" % (tmp / "again.ray")], check=True, capture_output=True, text=True)
    assert [ln for ln in r.stdout.splitlines() if "accepted steps" in ln] == [ln for ln in base.stdout.splitlines() if "accepted steps" in ln]


def test_segment_rows_zero_is_the_unsegmented_path(run16):
    tmp, cmd, plain = run16
    out = tmp / "zero.ray"
    subprocess.run(cmd + ["--outputfile=%s" % out, "--segment_rows=0"], check=True)
    assert out.read_bytes() == plain


def test_damping_with_segments_is_refused_by_name(run16):
    tmp, cmd, _ = run16
    r = subprocess.run(cmd + ["--outputfile=%s" % (tmp / "d.ray"), "--segment_rows=4", "--damping_out=%s" % (tmp / "d.txt")],
                       capture_output=True, text=True)
    assert r.returncode == 2 and "--damping_out together with --segment_rows" in r.stderr
    assert not (tmp / "d.txt").exists()
