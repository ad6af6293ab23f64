"""modelnum 6 (simple_3d_model_adapter.f95, srt_simple3d.hpp) on the device against goldens from the real reference
(tests/golden/simple3d_golden.npz, make_simple3d_golden.py): the parity ladder G0 .. G4 at the ladder's existing bars, each
with DESIGN section 4's sensitivity clause (a sample is held no tighter than 10 x what the reference itself does under a few-ulp
shift of x), plus what is particular to this model: a launch on the z axis, the builders, the exactness of the hoisting."""
import os

import numpy as np
import pytest

import model_ladder as ladder
from conftest import GOLDEN_DIR, vrel
from stanford_raytracer_amd import workloads as wl

pytestmark = pytest.mark.gpu
SETTINGS = "abcd"
DEL = 1e-6  # delDP of the driver's modelnum 6 (raytracer_driver.f95:1188)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN_DIR, "simple3d_golden.npz"))


def make_model(gold, tag):
    from stanford_raytracer_amd import api
    api.init(0)
    kp, yearday, msec, fixed, mlt, igrf, tsy = gold["g0_setting_" + tag]
    m = api.Model.simple3d(kp, yearday=int(yearday), msec=int(msec), fixed_mlt=(mlt if fixed else None))
    if igrf or tsy:
        m.set_field(use_igrf=int(igrf), use_tsyganenko=int(tsy), parmod=gold["parmod"] if tsy else None)
    return m


@pytest.fixture(scope="module")
def models(gold):
    return {t: make_model(gold, t) for t in SETTINGS}


def test_model_kind_is_6(models):
    from stanford_raytracer_amd import api
    assert models["a"].kind == 6 and api.lib().srt_model_kind(models["b"].h) == 6 and models["a"].nspec == 4
    qs, ms = models["a"].species()
    assert np.array_equal(qs, 1.602e-19 * np.array([-1.0, 1.0, 1.0, 1.0]))
    assert np.array_equal(ms, [9.10938188e-31, 1.6726e-27, 4.0 * 1.6726e-27, 16.0 * 1.6726e-27])


@pytest.mark.parametrize("tag", list(SETTINGS))
def test_g0_plasma_params(gold, models, tag):
    x, wantB = gold["g0_x_" + tag], gold["g0_B0_" + tag]
    g = models[tag].plasma_params(x)
    eB = vrel(g[:, 16:19], wantB)
    ladder.check_g0_density(g[:, 4:8], gold, tag, floor=1e-11, per_species=False, report=lambda err: print(
        "G0 %s: %d points, density error max %.3g (bit-equal %.1f %%), B0 error max %.3g" % (tag, len(x), err.max(), 100 * np.mean(err == 0), eB.max())))
    assert np.all(np.isfinite(g[:, 4:8])) and np.all(g[:, 12:16] == 0)
    assert eB.max() <= 2e-7


@pytest.mark.parametrize("tag", ["a", "b"])
def test_g1_dispersion_from_own_plasma_params(gold, models, tag):
    from dispersion_checks import check_dispersion_against_own_params
    check_dispersion_against_own_params(models[tag], gold["g23_state_" + tag])


@pytest.mark.parametrize("tag", ["a", "b"])
def test_g2_gradients_and_right_hand_side(gold, models, tag):
    ladder.check_g2(models[tag], gold["g23_state_" + tag], gold["g2_" + tag], gold["g2_sens_" + tag], DEL, tag)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_g3_single_steps(gold, models, tag):
    ladder.check_g3(models[tag], gold["g23_state_" + tag], gold["g3_" + tag], gold["g3_sens_" + tag], gold["g3_dt"], DEL, tag)


def golden_launches(models):
    """The 64 golden rays: the first 32 in setting a (free MLT), the others in setting b (fixed MLT)."""
    return [(models["a"], slice(0, 32)), (models["b"], slice(32, 64))]


def test_g4_fixed_step_trajectories(gold, models):
    ladder.check_g4_fixed(ladder.trace_golden_rays(gold, golden_launches(models), "fixed"), gold, min_steady=56)


def test_g4_adaptive_trajectories(gold, models):
    ladder.check_g4_adaptive(ladder.trace_golden_rays(gold, golden_launches(models), "adaptive"), gold, min_curves=48, same_t=ladder.same_t_first_rows)


def test_a_ray_on_the_z_axis_stops_and_leaves_its_neighbours_alone(gold, models):
    """On the z axis cos(latitude) is 6e-17 and L is 1e33 or infinite: the ray must end with a stop code of its own, and the
    other 63 lanes of its wave must produce the rows they produce without it."""
    assert ladder.z_axis_ray(gold, models["a"]) != 0


NX, NY, NZ = 6, 5, 4


@pytest.mark.parametrize("compder", [0, 1])
def test_grid_built_from_the_handle(models, compder):
    ladder.check_grid_from_handle(models["a"], NX, NY, NZ, ladder.BOUNDS, compder=bool(compder), nspec=4, then_trace=True)


def test_sample_builder_accepts_the_handle(models):
    ladder.check_sample_builder(models["a"])


def test_hoisting_is_exact(gold, models):
    """Points that share an MLT share everything the header evaluates once per point; a point's bits depend neither on its
    lane nor on what the other lanes of the wave evaluate: alone or in a batch of 64 mixed points, the same result."""
    rng = np.random.default_rng(8)
    mlt = 9.3
    phi = (mlt - 12.0) * 2.0 * np.pi / 24.0
    r = wl.R_E * rng.uniform(1.05, 7.0, 16)
    lat = np.deg2rad(rng.uniform(-70, 70, 16))
    same = np.stack([r * np.cos(lat) * np.cos(phi), r * np.cos(lat) * np.sin(phi), r * np.sin(lat)], axis=1)
    mixed = gold["g0_x_a"][:48]
    batch = np.concatenate([same, mixed])
    batch = batch[rng.permutation(len(batch))]
    for tag in ("a", "b"):
        whole = models[tag].plasma_params(batch)
        for i in range(0, 64, 5):
            alone = models[tag].plasma_params(batch[i:i + 1])
            assert np.array_equal(alone[0], whole[i]), (tag, i)
    # fixed MLT: the same points, rotated about the z axis, have the same densities as at the fixed meridian
    rot = same.copy()
    rot[:, 0], rot[:, 1] = -same[:, 1], same[:, 0]
    fa, fb = models["b"].plasma_params(same)[:, 4:8], models["b"].plasma_params(rot)[:, 4:8]
    assert np.abs(fa - fb).max() <= 1e-12 * fa.max() and np.all(fa > 0)
