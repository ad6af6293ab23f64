"""modelnum 5 (ngo_3d_dens_model_adapter.f95, srt_ngo3d.hpp) on the device against goldens from the real reference
(tests/golden/ngo3d_golden.npz, make_ngo3d_golden.py): the parity ladder G0 .. G4 at the bars tests/test_gpu_simple3d.py holds
modelnum 6 to, each with DESIGN section 4's sensitivity clause, plus what is particular to this model: a cross-check against
modelnum 1 that needs no golden, lane independence, a launch on the z axis, the tail modes, the builders."""
import os

import numpy as np
import pytest

import model_ladder as ladder
from conftest import GOLDEN_DIR, vrel
from stanford_raytracer_amd import workloads as wl

pytestmark = pytest.mark.gpu
SETTINGS = "abcd"
G23 = "abe"  # dipole field: a, b the plasmapause file (free / fixed MLT), e the ducts file
DEL = 1e-6  # delDP of the driver's modelnum 5 (raytracer_driver.f95:772-891)
NEWRAY = (wl.NEWRAY_PLASMAPAUSE, wl.NEWRAY_DUCTS)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN_DIR, "ngo3d_golden.npz"))


@pytest.fixture(scope="module")
def cards(tmp_path_factory):
    d = tmp_path_factory.mktemp("ngo3d")
    out = []
    for k, text in enumerate(NEWRAY):
        out.append(str(d / ("newray%d.in" % k)))
        with open(out[-1], "w") as f:
            f.write(text)
    return out


def make_model(gold, cards, tag):
    from stanford_raytracer_amd import api
    api.init(0)
    kp, yearday, msec, fixed, mlt, igrf, tsy, card = gold["g0_setting_" + tag]
    m = api.Model.ngo3d(cards[int(card)], kp, yearday=int(yearday), msec=int(msec), fixed_mlt=(mlt if fixed else None))
    if igrf or tsy:
        m.set_field(use_igrf=int(igrf), use_tsyganenko=int(tsy), parmod=gold["parmod"] if tsy else None)
    return m


@pytest.fixture(scope="module")
def models(gold, cards):
    return {t: make_model(gold, cards, t) for t in SETTINGS + "e"}


def test_model_kind_is_5(models):
    from stanford_raytracer_amd import api
    assert models["a"].kind == 5 and api.lib().srt_model_kind(models["c"].h) == 5 and models["a"].nspec == 4
    assert api.lib().srt_model_nspec(models["d"].h) == 4
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


@pytest.mark.parametrize("tag", list(G23))
def test_g1_dispersion_from_own_plasma_params(gold, models, tag):
    from dispersion_checks import check_dispersion_against_own_params
    check_dispersion_against_own_params(models[tag], gold["g23_state_" + tag])


@pytest.mark.parametrize("tag", list(G23))
def test_g2_gradients_and_right_hand_side(gold, models, tag):
    ladder.check_g2(models[tag], gold["g23_state_" + tag], gold["g2_" + tag], gold["g2_sens_" + tag], DEL, tag)


@pytest.mark.parametrize("tag", list(G23))
def test_g3_single_steps(gold, models, tag):
    """One rk4 / rk45 step at the ladder's bars (position: median 1e-8, max 1e-7; k: median 1e-7, max 1e-2), each sample held no
    tighter than 10 x the reference's own movement of that sample under 256 few-ulp shifts of x and k.  (k as well as x: with
    the ducts file the reference's 5th-order position at one state of e has two answers 1.017e-7 apart, and only a few-ulp shift
    of k, one in eight, moves it from one to the other; the device gives the other one.)"""
    ladder.check_g3(models[tag], gold["g23_state_" + tag], gold["g3_" + tag], gold["g3_sens_" + tag], gold["g3_dt"], DEL, tag)


def golden_launches(models):
    """The 64 golden rays: the first 32 in setting a (free MLT), the others in setting b (fixed MLT)."""
    return [(models["a"], slice(0, 32)), (models["b"], slice(32, 64))]


def test_g4_fixed_step_trajectories(gold, models):
    ladder.check_g4_fixed(ladder.trace_golden_rays(gold, golden_launches(models), "fixed"), gold, min_steady=56)


def test_g4_adaptive_trajectories(gold, models):
    ladder.check_g4_adaptive(ladder.trace_golden_rays(gold, golden_launches(models), "adaptive"), gold, min_curves=48, same_t=ladder.same_t_first_rows)


def a8_of(mlt, kp):
    """bulge's a8 (pp_profile_d.f95:52-131) in numpy, with the Fortran's default-real literals as float32"""
    f = np.float32
    x = mlt - (47.0 / (kp + np.float64(f(3.9))) + np.float64(f(11.3)))
    x = x + 24.0 if x < -12.0 else (x - 24.0 if x > 12.0 else x)
    absx = abs(x) * np.float64(f(2.6179939e-1))
    s = np.sin(mlt * np.float64(f(0.26179939)) + np.float64(f(1.5707963)))
    b1 = np.float64(f(0.043)) * s - np.float64(f(0.4589))
    b2 = -(np.float64(f(0.361)) * s) + np.float64(f(5.7464))
    return (b1 * kp + b2) * (1.0 + np.exp(-(1.5 * absx * absx) + np.float64(f(0.08)) * absx - np.float64(f(0.7))))


@pytest.mark.parametrize("kp,mlt", [(4.0, 2.0), (2.0, 14.5), (6.5, 19.0)])
def test_fixed_mlt_equals_model_1_with_the_plasmapause_rewritten(cards, tmp_path, kp, mlt):
    """No golden needed: with fixed_MLT = 1 every point has the plasmapause a8(MLT, Kp) - ddk, and modelnum 1 created from the
    same card file with that number in its lk field is the same model -- provided both lk, the file's 5.55 and the rewritten
    one, lie above dsrrng = 2, so that readinput's normalisation at L = 2 sees no knee in either.  Bar 1e-10 relative:
    |d ln N / d lk| <= sqrt(160) / ddk = 181 (argl is capped at 80), so a few-ulp difference between numpy's a8 and the device's
    (<= 1e-14) moves a density by <= 2e-12."""
    from stanford_raytracer_amd import api
    api.init(0)
    ddk = 0.07
    lk = float(a8_of(mlt, kp)) - ddk
    assert lk > 2.0
    assert NEWRAY[0].count("\n5.55 3.0 0.07 ") == 1
    card1 = str(tmp_path / "newray_lk.in")
    with open(card1, "w") as f:
        f.write(NEWRAY[0].replace("\n5.55 3.0 0.07 ", "\n%.17g 3.0 0.07 " % lk))
    m5 = api.Model.ngo3d(cards[0], kp, fixed_mlt=mlt)
    m1 = api.Model.ngo(card1)
    rng = np.random.default_rng(55)
    v = rng.normal(size=(500, 3))
    x = v / np.linalg.norm(v, axis=1, keepdims=True) * (wl.R_E * rng.uniform(1.1, 7.0, (500, 1)))
    a, b = m5.plasma_params(x)[:, 4:8], m1.plasma_params(x)[:, 4:8]
    L = np.linalg.norm(x, axis=1) ** 3 / (wl.R_E * (x[:, 0] ** 2 + x[:, 1] ** 2))
    err = np.abs(a - b) / b
    print("Kp %g MLT %g: lk %.6f, %d of 500 points beyond it, max difference %.3g, bit-equal %.1f %%"
          % (kp, mlt, lk, (L > lk).sum(), err.max(), 100 * np.mean(err == 0)))
    assert (L > lk).sum() >= 50 and (L < lk).sum() >= 50
    assert np.all(b > 0) and err.max() <= 1e-10
    # and it is not modelnum 1 of the unchanged file
    c = api.Model.ngo(cards[0]).plasma_params(x)[:, 4:8]
    assert np.max(np.abs(a - c) / c) > 1e-3


def test_a_points_bits_depend_neither_on_its_lane_nor_on_its_neighbours(gold, models):
    """alone or inside a batch of 64 mixed points: the same bits (one compiled body for every path, both MLT modes)"""
    rng = np.random.default_rng(8)
    batch = np.concatenate([gold["g0_x_c"][-40:], gold["g0_x_a"][:24]])
    batch = batch[rng.permutation(len(batch))]
    for tag in ("a", "b", "c"):
        whole = models[tag].plasma_params(batch)
        for i in range(0, 64, 5):
            alone = models[tag].plasma_params(batch[i:i + 1])
            assert np.array_equal(alone[0], whole[i]), (tag, i)
    # fixed MLT: points rotated about the z axis have the densities they have at the first meridian
    same = gold["g0_x_a"][:32]
    rot = same.copy()
    rot[:, 0], rot[:, 1] = -same[:, 1], same[:, 0]
    fa, fb = models["b"].plasma_params(same)[:, 4:8], models["b"].plasma_params(rot)[:, 4:8]
    # (x^2 + y^2 may round differently with the roles swapped under contraction: 1 ulp of l, times |d ln N / d l| <= 181, l < 7)
    assert np.all(np.abs(fa - fb) <= 1e-12 * fa) and np.all(fa > 0)


def test_a_ray_on_the_z_axis_stops_and_leaves_its_neighbours_alone(gold, models):
    """On the z axis rho = 0: L is infinite and the longitude atan2(0, 0).  The ray must end with a stop code of its own, and the
    other 63 lanes of its wave must produce the rows they produce without it."""
    assert 0 <= ladder.z_axis_ray(gold, models["a"]) <= 9


@pytest.mark.parametrize("tag", ["a", "c"])
def test_tail_modes_give_the_bits_of_a_full_wave(gold, models, tag):
    """The 64 golden rays in one wave (every lane evaluates its own stencil) and each ray alone (1 needy lane: its stencil is
    spread over four lanes, the offset points of its right-hand sides over eight): rows, row counts and stop codes bit for bit."""
    p, _ = ladder.run_params(gold, "adaptive")
    pos0, d, w = gold["run_pos0"], gold["run_dir0"], gold["run_w0"]
    rows, nrows, stop, _ = models[tag].trace(pos0, d, w, params=p)
    assert nrows.max() > 8
    for i in range(len(w)):
        r1, n1, s1, _ = models[tag].trace(pos0[i:i + 1], d[i:i + 1], w[i:i + 1], params=p)
        assert n1[0] == nrows[i] and s1[0] == stop[i], (i, n1[0], nrows[i], s1[0], stop[i])
        assert np.array_equal(r1[0, :n1[0]], rows[i, :n1[0]], equal_nan=True), i


NX, NY, NZ = 6, 5, 4


@pytest.mark.parametrize("compder", [0, 1])
def test_grid_built_from_the_handle(models, compder):
    ladder.check_grid_from_handle(models["a"], NX, NY, NZ, ladder.BOUNDS, compder=bool(compder), nspec=4, then_trace=True)


def test_sample_builder_accepts_the_handle(models):
    ladder.check_sample_builder(models["a"])
