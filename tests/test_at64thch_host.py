"""modelnum 7 on the CPU: the field-line tracer (stanford_raytracer_amd/csrc/srt_fieldline.hpp) and the AT64ThCh model around it
(srt_at64thch.hpp) -- the very source the device compiles -- built for the host (tests/native/at64thch_host.cpp) and held against
goldens captured from the reference's own AT64ThCh_adapter and geopack's TRACE_08 (tests/golden/at64thch_golden.npz,
make_at64thch_golden.py).

Bars, per point and with no point skipped:
  foot      at every golden point the model traces (above 400 km; below, TRACE_08 reads its previous point before setting it):
            max(2e-6 R_E, 10 x the reference's own foot movement under its fp32-ulp shifts).  The floor is 10 fp32 ulps at the
            foot's radius: r = 1.063, ulp 1.2e-7, and a coordinate of the foot is the last point of an fp32 integration.
  ending    equal wherever the recorded sensitivity of n_e (the density the trace enters) is below 1e-5.
  density   per species max(1e-6, 10 x that species' sensitivity).  The floor: n_e goes with sqrt(zbrat), zbrat is the fp32 quotient of two fp32 square
            roots -- three half-ulp roundings, 3 x 6e-8 / 2 = 9e-8 in n_e -- times 10.
"""
import os

import numpy as np
import pytest

from at64thch_checks import Host, build_host_library, check_foot
from conftest import GOLDEN_DIR
from model_ladder import check_g0_density
from stanford_raytracer_amd import workloads as wl

SETTINGS = "abcd"


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN_DIR, "at64thch_golden.npz"))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return build_host_library(tmp_path_factory.mktemp("at64thch"))


@pytest.fixture(scope="module")
def hosts(gold, lib):
    return {t: Host(lib, gold["g0_setting_" + t], gold["parmod_" + t]) for t in SETTINGS}


def test_the_committed_golden_meets_the_generators_conditions(gold):
    sens = np.concatenate([gold["g0_sens_" + t] for t in SETTINGS])
    Ns = np.concatenate([gold["g0_Ns_" + t] for t in SETTINGS])
    foot = np.concatenate([gold["g0_foot_" + t] for t in SETTINGS])
    foot = foot[np.isfinite(foot[:, 0])]
    assert np.all(np.isfinite(Ns)) and np.all(Ns > 0)
    # the sensitivity condition, on n_e (through which alone the trace enters the model) over every point of every family
    assert sens.shape == (2120, 3) and np.mean(sens[:, 0] > 1e-5) <= 0.05 and sens[:, 0].max() <= 1e-3
    assert (foot[:, 4] == 0).sum() >= 20 and (foot[:, 4] == 1).sum() >= 20 and np.all(foot[:, 5] <= 500)
    for t in "ab":
        fam, x = gold["g0_fam_" + t], gold["g0_x_" + t]
        assert [(fam == k).sum() for k in range(5)] == [400, 40, 40, 60, 60]
        alt = np.linalg.norm(x, axis=1) - wl.R_E
        assert np.all(alt[fam == 1] <= 400e3) and (alt[fam == 2] > 400e3).sum() == 20 and (alt[fam == 2] < 400e3).sum() == 20
    st = np.array([gold["g0_setting_" + t] for t in SETTINGS])
    assert len({(a, b) for a, b in st[:, 0:2]}) >= 2 and st[:, 3].sum() >= 2 and st[:, 4].sum() >= 1
    assert gold["parmod_a"][0] == 4.0 and gold["parmod_b"][0] == 1.7


@pytest.mark.parametrize("tag", list(SETTINGS))
def test_foot_against_the_references_trace_08(gold, hosts, tag):
    check_foot(hosts[tag].foot(gold["g0_x_" + tag]), gold, tag)


@pytest.mark.parametrize("tag", list(SETTINGS))
def test_densities_against_the_reference(gold, hosts, tag):
    check_g0_density(hosts[tag].density(gold["g0_x_" + tag]), gold, tag, floor=1e-6, per_species=True)


def test_at_or_below_400_km_the_density_is_the_closed_form_with_ratio_one(gold, hosts):
    x, fam = gold["g0_x_a"], gold["g0_fam_a"]
    alt = np.linalg.norm(x, axis=1) - wl.R_E
    low = x[alt <= 400e3]
    assert len(low) >= 60
    got, want = hosts["a"].density(low), hosts["a"].closed_form(low, 1.0)
    assert np.array_equal(got, want)
    # and just above, the ratio is not one: the trace runs
    up = x[(fam == 2) & (alt > 400e3)]
    assert np.all(hosts["a"].density(up) != hosts["a"].closed_form(up, 1.0))


def test_a_line_of_more_than_500_points_and_a_nan_start_give_nan_and_terminate(hosts):
    h = hosts["b"]
    x = np.array([[4.0 * wl.R_E, 0.0, 0.5 * wl.R_E]])
    ok = h.foot(x)
    assert ok[0, 4] == 0 and 10 < ok[0, 5] <= 500
    # the same line with a step limit of 0.004 R_E needs more than 500 points: no foot
    far = h.foot(x, dsmax=0.004)
    assert far[0, 4] == 3 and far[0, 5] == 501 and np.all(np.isnan(far[0, 0:4]))
    # with room for them it ends on the sphere, where the coarse trace ended
    fine = h.foot(x, dsmax=0.004, lmax=4000)
    assert fine[0, 4] == 0 and 500 < fine[0, 5] <= 4000 and np.linalg.norm(fine[0, 0:3] - ok[0, 0:3]) < 1e-3
    nan = h.foot(np.array([[np.nan, 0.0, 2.0 * wl.R_E]]))
    assert nan[0, 4] == 3 and np.all(np.isnan(nan[0, 0:4]))
    assert np.all(np.isnan(h.density(np.array([[np.nan, 0.0, 2.0 * wl.R_E]]))))


def test_geopacks_tilt_angle_is_not_the_adapters_alias(hosts):
    """RECALC_08's PSI for 2010-001 00:00 UT is the dipole tilt, about -0.45 rad in northern winter at midnight UT; the word the
    other adapters hand to T04_s (ST0, about 0.17) is something else."""
    psi = hosts["a"].L.at64h_psi(hosts["a"].h)
    mu = -np.arctan2(np.sin(np.deg2rad(23.44)) * 1.0, 1.0)  # the Sun's declination alone: -23 deg at the solstice
    assert -0.62 < psi < -0.25 and abs(psi - 0.17) > 0.3 and abs(psi - mu) < 0.25
