"""modelnum 7 (AT64ThCh_adapter.f95; srt_at64thch.hpp around the field-line tracer srt_fieldline.hpp) on the device against
goldens from the real reference (tests/golden/at64thch_golden.npz, make_at64thch_golden.py): srt_field_line_foot against
geopack's own TRACE_08 and the parity ladder G0 .. G4, at the bars of tests/test_at64thch_host.py (foot, densities) and of the
ladder (G1 .. G4), each with DESIGN section 4's sensitivity clause: a sample is held no tighter than 10 x what the reference
itself does under an fp32-ulp shift of x (and of k for G2 / G3), because a few-ulp shift in double never reaches the fp32 trace.
Plus what is particular to this model: the device against the host build of the same source, lane independence of the
wave-uniform trace, partial waves, the refusal of a handle without a coefficient table, the grid builder."""
import os

import numpy as np
import pytest

import model_ladder as ladder
from at64thch_checks import Host, build_host_library, check_foot, foot_bar
from conftest import GOLDEN_DIR, vrel
from stanford_raytracer_amd import workloads as wl

pytestmark = pytest.mark.gpu
SETTINGS = "abcd"
DEL = 1e-4  # delSP, the driver's step for modelnum 7 (raytracer_driver.f95:1189-1194)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN_DIR, "at64thch_golden.npz"))


def make_model(gold, tag):
    from stanford_raytracer_amd import api
    api.init(0)
    kp, yearday, msec, igrf, tsy = gold["g0_setting_" + tag]
    m = api.Model.at64thch(int(kp), gold["parmod_" + tag], yearday=int(yearday), msec=int(msec))
    if igrf or tsy:
        m.set_field(use_igrf=int(igrf), use_tsyganenko=int(tsy))
    return m


@pytest.fixture(scope="module")
def models(gold):
    return {t: make_model(gold, t) for t in SETTINGS}


@pytest.fixture(scope="module")
def g0(gold, models):
    """the device's plasma_params and feet at every golden point, once for all tests"""
    return {t: (models[t].plasma_params(gold["g0_x_" + t]), models[t].field_line_foot(gold["g0_x_" + t])) for t in SETTINGS}


def test_model_kind_is_7_with_three_species(models):
    from stanford_raytracer_amd import api
    assert models["a"].kind == 7 and api.lib().srt_model_kind(models["b"].h) == 7 and models["a"].nspec == 3
    qs, ms = models["a"].species()
    assert np.array_equal(qs, 1.602e-19 * np.array([-1.0, 1.0, 1.0, 0.0]))
    assert np.array_equal(ms, [9.10938188e-31, 16.0 * 1.6726e-27, 1.6726e-27, 0.0])
    with pytest.raises(ValueError):
        api.Model.at64thch(4.5, np.zeros(10))


@pytest.mark.parametrize("tag", list(SETTINGS))
def test_field_line_foot_against_the_references_trace_08(gold, g0, tag):
    check_foot(g0[tag][1], gold, tag)


@pytest.mark.parametrize("tag", list(SETTINGS))
def test_g0_plasma_params(gold, g0, tag):
    g = g0[tag][0]
    ladder.check_g0_density(g[:, 4:7], gold, tag, floor=1e-6, per_species=True)
    eB = vrel(g[:, 16:19], gold["g0_B0_" + tag])
    print("G0 %s: B0 error max %.3g" % (tag, eB.max()))
    assert np.all(g[:, 7] == 0) and np.all(g[:, 12:16] == 0) and np.all(g[:, 3] == 0)
    assert eB.max() <= 2e-7


@pytest.mark.parametrize("tag", ["b", "d"])
def test_device_against_the_host_build_of_the_same_source(gold, g0, tag, tmp_path_factory):
    """The same headers compiled for the host: the device's T04_s takes its elementary functions from srt_fastmath.hpp, the
    host's from libm, so a T04_s component may differ in its last fp32 bit and a trace may then take another step sequence:
    the bars are those against the reference (the reference's own sensitivity), and most points are bit-equal."""
    L = build_host_library(tmp_path_factory.mktemp("at64thch_dev"))
    h = Host(L, gold["g0_setting_" + tag], gold["parmod_" + tag])
    x = gold["g0_x_" + tag]
    hf, hn = h.foot(x), h.density(x)
    df, dn = g0[tag][1], g0[tag][0][:, 4:7]
    traced = np.linalg.norm(x, axis=1) - wl.R_E > 400e3   # (the points the model traces, as in the tests against the reference)
    move = np.linalg.norm(df[:, 0:3] - hf[:, 0:3], axis=1)
    err = np.abs(dn - hn) / hn
    print("device vs host %s: feet bit-equal %.1f %%, max distance %.3g; densities bit-equal %.1f %%, max %.3g"
          % (tag, 100 * np.mean(move == 0), move.max(), 100 * np.mean(err == 0), err.max()))
    assert np.all(move[traced] <= foot_bar(gold, tag)[traced])
    quiet = gold["g0_sens_" + tag][:, 0] < 1e-5
    assert np.array_equal(df[quiet, 4], hf[quiet, 4])
    assert np.all(err <= np.maximum(1e-6, 10.0 * gold["g0_sens_" + tag]))
    assert np.mean(move[traced] == 0) >= 0.5


def test_g1_dispersion_from_own_plasma_params(gold, models):
    from dispersion_checks import check_dispersion_against_own_params
    check_dispersion_against_own_params(models["a"], gold["g23_state"])


@pytest.mark.parametrize("tag", ["a", "b", "d"])
def test_g2_gradients_and_right_hand_side(gold, models, tag):
    ladder.check_g2(models[tag], gold["g23_state"], gold["g2_" + tag], gold["g2_sens_" + tag], DEL, tag)


@pytest.mark.parametrize("tag", ["a", "b", "d"])
def test_g3_single_steps(gold, models, tag):
    ladder.check_g3(models[tag], gold["g23_state"], gold["g3_" + tag], gold["g3_sens_" + tag], gold["g3_dt"], DEL, tag)


def golden_launches(models):
    """The 16 golden rays, in setting d: one launch."""
    return [(models["d"], slice(None))]


def test_g4_fixed_step_trajectories(gold, models):
    ladder.check_g4_fixed(ladder.trace_golden_rays(gold, golden_launches(models), "fixed"), gold, min_steady=14)


def test_g4_adaptive_trajectories(gold, models):
    # 15 curves: the sixteenth ray stops at its launch point, on both
    ladder.check_g4_adaptive(ladder.trace_golden_rays(gold, golden_launches(models), "adaptive"), gold, min_curves=15, yard_curves=15,
                             same_t=ladder.same_t_all_rows)


def test_a_lanes_bits_do_not_depend_on_the_other_lanes(gold, models):
    """The trace loop runs until every lane of the wave has ended and the IGRF synthesis reads its terms across the wave: a
    point's densities and foot must be the same bits alone and among 63 others whose lines have very different lengths
    (5 .. 300 points, open lines) or no trace at all (two lanes below 400 km)."""
    x, fam, foot = gold["g0_x_a"], gold["g0_fam_a"], gold["g0_foot_a"]
    L = np.nan_to_num(foot[:, 5])
    order = np.argsort(L[fam == 0])
    rnd = np.nonzero(fam == 0)[0][order]
    pick = np.concatenate([rnd[:10], rnd[-10:], rnd[100:124], np.nonzero(fam == 4)[0][:18], np.nonzero(fam == 1)[0][:2]])
    assert len(pick) == 64 and L[pick].max() >= 10 * L[pick][L[pick] > 0].min() and (L[pick] == 0).sum() == 2
    batch = x[pick][np.random.default_rng(3).permutation(64)]
    m = models["a"]
    whole, feet = m.plasma_params(batch), m.field_line_foot(batch)
    assert np.array_equal(whole, m.plasma_params(batch[::-1])[::-1]) and np.array_equal(feet, m.field_line_foot(batch[::-1])[::-1])
    for i in range(64):
        assert np.array_equal(m.plasma_params(batch[i:i + 1])[0], whole[i]), i
        assert np.array_equal(m.field_line_foot(batch[i:i + 1])[0], feet[i]), i


@pytest.mark.parametrize("n", [1, 63, 65])
def test_partial_waves(gold, models, g0, n):
    x = gold["g0_x_b"][:n]
    assert np.array_equal(models["b"].plasma_params(x), g0["b"][0][:n])
    assert np.array_equal(models["b"].field_line_foot(x), g0["b"][1][:n])


def test_foot_needs_a_coefficient_table_and_parmod(cfgfiles, gold):
    from stanford_raytracer_amd import api
    api.init(0)
    ngo = api.Model.ngo(cfgfiles["ngo"])
    x = gold["g0_x_a"][:3]
    with pytest.raises(Exception, match="coefficient table"):
        ngo.field_line_foot(x)
    ngo.set_field(use_igrf=1)
    with pytest.raises(Exception, match="T04_s parameters"):
        ngo.field_line_foot(x)
    # with both it is the trace of the model-7 handle of the same date and parmod
    ngo.set_field(use_igrf=1, parmod=gold["parmod_a"])
    m7 = api.Model.at64thch(4, gold["parmod_a"], yearday=2010001, msec=0)
    assert np.array_equal(ngo.field_line_foot(x), m7.field_line_foot(x))


def test_grid_built_from_the_handle(models):
    ladder.check_grid_from_handle(models["a"], 4, 4, 3, ladder.BOUNDS, compder=False, nspec=3, then_trace=False)
