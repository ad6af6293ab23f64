"""modelnum 6 on the CPU: stanford_raytracer_amd/csrc/srt_simple3d.hpp -- the very header the device compiles -- built for
the host with g++ (tests/native/simple3d_host.cpp) and held against goldens captured from the reference's own
simple_3d_model_adapter (tests/golden/simple3d_golden.npz, make_simple3d_golden.py).

Bar, per point and with no point skipped: max(1e-11, 10 x the reference's recorded sensitivity) relative.  1e-11 is the
project's G0 bar; the second term is DESIGN section 4's sensitivity rule (a point where the reference itself moves by more under
a few-ulp shift of x -- a flipped decision of one of the model's halving searches -- cannot be held tighter than that)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN_DIR, ROOT
from model_ladder import check_g0_density

SETTINGS = "abcd"


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN_DIR, "simple3d_golden.npz"))


@pytest.fixture(scope="module")
def hostlib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("s3d") / "libs3dh.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                           os.path.join(ROOT, "tests", "native", "simple3d_host.cpp")])
    L = C.CDLL(so)
    L.s3dh_density.argtypes = [C.c_double, C.c_int, C.c_int, C.c_double, C.c_long, C.c_void_p, C.c_void_p]
    L.s3dh_mlt_terms.argtypes = [C.c_double, C.c_double, C.c_double, C.c_void_p]
    return L


def host_density(L, setting, x):
    kp, yearday, _, fixed, mlt = setting[:5]
    x = np.ascontiguousarray(x, dtype=np.float64)
    Ns = np.zeros((len(x), 4))
    L.s3dh_density(kp, int(yearday), int(fixed), mlt, len(x), x.ctypes.data, Ns.ctypes.data)
    return Ns


def test_the_committed_golden_meets_the_generators_input_conditions(gold):
    sens = np.concatenate([gold["g0_sens_" + t] for t in SETTINGS])
    Ns = np.concatenate([gold["g0_Ns_" + t] for t in SETTINGS])
    assert len(sens) >= 2000
    assert np.all(np.isfinite(Ns)) and np.all(Ns > 0)
    assert np.mean(sens > 1e-11) <= 1e-3
    assert sens.max() <= 1e-6
    # at least two (Kp, date) settings, fixed_MLT both ways, IGRF and T04_s for one setting each
    st = np.array([gold["g0_setting_" + t] for t in SETTINGS])
    assert len({(a, b) for a, b in st[:, 0:2]}) >= 2 and set(st[:, 3]) == {0.0, 1.0}
    assert st[:, 5].sum() >= 1 and st[:, 6].sum() >= 1
    # the points reach into every transition: 200 km .. 12 000 km, both hemispheres, across L = 2 .. 7, MLT either side of 0/24
    x = gold["g0_x_a"]
    r = np.linalg.norm(x, axis=1)
    mlt = np.mod(24.0 * np.arctan2(x[:, 1], x[:, 0]) / (2 * np.pi) + 12.0, 24.0)
    assert r.min() <= 6371.2e3 + 201e3 and r.max() >= 7.0 * 6371.2e3
    assert (x[:, 2] > 0).sum() > 100 and (x[:, 2] < 0).sum() > 100
    assert (mlt < 1e-6).any() and (mlt > 24 - 1e-6).any()


@pytest.mark.parametrize("tag", list(SETTINGS))
def test_host_build_of_the_device_header_against_the_reference(gold, hostlib, tag):
    x = gold["g0_x_" + tag]
    got = host_density(hostlib, gold["g0_setting_" + tag], x)
    check_g0_density(got, gold, tag, floor=1e-11, per_species=False, report=lambda err: print(
        "setting %s: %d points, max error %.3g, bit-equal %.1f %%" % (tag, len(x), err.max(), 100 * np.mean(err == 0))))


def test_mlt_only_terms_are_in_their_physical_range(hostlib):
    """What the header evaluates once per point from MLT, Kp and the date alone (bulge, the geosynchronous trough density,
    the annual term of ne_ps, check_crossing): the plasmapause lies within bulge's own bounds for Kp 0 .. 8 -- (b1 Kp + b2) between 5.3854 - 8 x 0.5019 = 1.37 and
    6.1074, times 1 .. 1 + exp(-0.7 + 0.08^2 / 6) = 1.497 -- at every MLT; the crossing is
    a8 plus the halving search's steps (0.5, -0.25, 0.125, -0.0625, 0.03125, each taken any number of times), a multiple
    of 1/32, and lies outside the Earth."""
    for kp in (0.0, 2.5, 4.0, 8.0):
        for mlt in np.linspace(0.0, 24.0, 49):
            out = np.zeros(5)
            hostlib.s3dh_mlt_terms(mlt, kp, 1.0, out.ctypes.data)
            a8, a9, geosync, season, zl = out
            assert np.all(np.isfinite(out)), (kp, mlt)
            assert 1.37 < a8 < 9.15 and a9 > 1.0 and geosync > 0 and abs(season) < 0.3, (kp, mlt, out)
            k32 = (zl - a8) * 32.0
            assert abs(k32 - round(k32)) < 1e-9 and zl > 1.0, (kp, mlt, out)


def test_failed_knee_search_becomes_a_nan_density(hostlib):
    """Where the reference stops the process ("Failed to find knee in check_crossing") the density is NaN: a non-finite Kp
    never lets the halving search change direction."""
    x = np.array([[2.0 * 6371.2e3, 0.0, 0.0]])
    got = host_density(hostlib, (float("nan"), 2010001, 0, 0, 0.0), x)
    assert np.all(np.isnan(got))
