"""modelnum 5 (ngo_3d_dens_model_adapter.f95, srt_ngo3d.hpp) on the device against goldens from the real reference
(tests/golden/ngo3d_golden.npz, make_ngo3d_golden.py): the parity ladder G0 .. G4 at the bars tests/test_gpu_simple3d.py holds
modelnum 6 to, each with DESIGN section 4's sensitivity clause, plus what is particular to this model: a cross-check against
modelnum 1 that needs no golden, lane independence, a launch on the z axis, the tail modes, the builders."""
import os

import numpy as np
import pytest

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
    x, want, wantB, sens = (gold["g0_%s_%s" % (k, tag)] for k in ("x", "Ns", "B0", "sens"))
    g = models[tag].plasma_params(x)
    err = np.max(np.abs(g[:, 4:8] - want) / want, axis=1)
    bar = np.maximum(1e-11, 10.0 * sens)
    eB = vrel(g[:, 16:19], wantB)
    print("G0 %s: %d points, density error max %.3g (bit-equal %.1f %%), B0 error max %.3g" % (tag, len(x), err.max(), 100 * np.mean(err == 0), eB.max()))
    assert np.all(np.isfinite(g[:, 4:8])) and np.all(g[:, 12:16] == 0)
    assert np.all(err <= bar), "%d points over their bar, worst ratio %.3g" % ((err > bar).sum(), np.max(err / bar))
    assert eB.max() <= 2e-7


def held(err, sens, bar):
    """err / its bar, per sample: the ladder's bar, or 10 x the reference's own recorded sensitivity of that sample where that is
    more (DESIGN section 4's sensitivity clause).  <= 1 means held."""
    return err / np.maximum(bar, 10.0 * sens)


def sens_rel(s, ref):
    """recorded absolute sensitivity of a vector -> relative to the vector"""
    return np.linalg.norm(s, axis=-1) / np.maximum(np.linalg.norm(ref, axis=-1), 1e-300)


@pytest.mark.parametrize("tag", list(G23))
def test_g1_dispersion_from_own_plasma_params(gold, models, tag):
    from dispersion_checks import check_dispersion_against_own_params
    check_dispersion_against_own_params(models[tag], gold["g23_state_" + tag])


@pytest.mark.parametrize("tag", list(G23))
def test_g2_gradients_and_right_hand_side(gold, models, tag):
    st, ref, sn = gold["g23_state_" + tag], gold["g2_" + tag], gold["g2_sens_" + tag]
    g = models[tag].gradients(st[:, 0:3], st[:, 3:6], st[:, 6], DEL)
    ek, sk = vrel(g[:, 0:3], ref[:, 0:3]), sens_rel(sn[:, 0:3], ref[:, 0:3])
    ew, sw = np.abs(g[:, 3] - ref[:, 3]) / np.abs(ref[:, 3]), sn[:, 3] / np.abs(ref[:, 3])
    ex, sx = vrel(g[:, 4:7], ref[:, 4:7]), sens_rel(sn[:, 4:7], ref[:, 4:7])
    ev, sv = vrel(g[:, 7:10], ref[:, 7:10]), sens_rel(sn[:, 7:10], ref[:, 7:10])
    ed, sd = vrel(g[:, 10:13], ref[:, 10:13]), sens_rel(sn[:, 10:13], ref[:, 10:13])
    print("G2 %s: dFdk %.3g dFdw %.3g dFdx %.3g (reference's own %.3g) dx/dt %.3g dk/dt median %.3g max %.3g (own %.3g)"
          % (tag, ek.max(), ew.max(), ex.max(), sx.max(), ev.max(), np.median(ed), ed.max(), sd.max()))
    assert held(ek, sk, 1e-7).max() <= 1
    assert held(ew, sw, 1e-6).max() <= 1
    assert held(ex, sx, 1e-7).max() <= 1
    assert held(ev, sv, 1e-6).max() <= 1
    assert np.median(held(ed, sd, 1e-6)) <= 1 and held(ed, sd, 2e-5).max() <= 1


@pytest.mark.parametrize("tag", list(G23))
def test_g3_single_steps(gold, models, tag):
    """One rk4 / rk45 step at the ladder's bars (position: median 1e-8, max 1e-7; k: median 1e-7, max 1e-2), each sample held no
    tighter than 10 x the reference's own movement of that sample under 256 few-ulp shifts of x and k.  (k as well as x: with
    the ducts file the reference's 5th-order position at one state of e has two answers 1.017e-7 apart, and only a few-ulp shift
    of k, one in eight, moves it from one to the other; the device gives the other one.)"""
    st, ref, sn = gold["g23_state_" + tag], gold["g3_" + tag], gold["g3_sens_" + tag]
    g = models[tag].rk_step(st, np.full(len(st), float(gold["g3_dt"])), DEL)
    for o in (0, 7, 14):
        ex, sx = vrel(g[:, o:o + 3], ref[:, o:o + 3]), sens_rel(sn[:, o:o + 3], ref[:, o:o + 3])
        ek, sk = vrel(g[:, o + 3:o + 6], ref[:, o + 3:o + 6]), sens_rel(sn[:, o + 3:o + 6], ref[:, o + 3:o + 6])
        print("G3 %s out %d: position median %.3g max %.3g (own %.3g), k median %.3g max %.3g (own %.3g)"
              % (tag, o // 7, np.median(ex), ex.max(), sx.max(), np.median(ek), ek.max(), sk.max()))
        assert np.median(held(ex, sx, 1e-8)) <= 1 and held(ex, sx, 1e-7).max() <= 1, (np.sort(held(ex, sx, 1e-7))[-3:], np.median(held(ex, sx, 1e-8)))
        assert np.median(held(ek, sk, 1e-7)) <= 1 and held(ek, sk, 1e-2).max() <= 1
        assert np.array_equal(g[:, o + 6], st[:, 6])  # omega is carried unchanged


def run_params(gold, mode):
    from stanford_raytracer_amd import api
    fixedstep, dt0, dtmax, tmax, maxerr, maxsteps, minalt, del_ = gold["run_%s_params" % mode]
    return api.make_params(dt0=dt0, dtmax=dtmax, tmax=tmax, maxerr=maxerr, maxsteps=int(maxsteps), minalt=minalt,
                           fixedstep=int(fixedstep), del_=del_, outputper=1), float(tmax)


def trace_golden_rays(gold, models, mode, pos0=None):
    """The 64 golden rays: the first 32 in setting a (free MLT), the others in setting b (fixed MLT)."""
    p, _ = run_params(gold, mode)
    pos0 = gold["run_pos0"] if pos0 is None else pos0
    d, w = gold["run_dir0"], gold["run_w0"]
    out = [models[t].trace(pos0[h], d[h], w[h], params=p)[:3] for t, h in (("a", slice(0, 32)), ("b", slice(32, 64)))]
    return tuple(np.concatenate([o[k] for o in out]) for k in range(3))


def widen(rows7):
    """golden rows (t, pos, vgrel) -> the library's 20-column layout (only those columns filled)"""
    r = np.full(rows7.shape[:2] + (20,), np.nan)
    r[:, :, 0:4] = rows7[:, :, 0:4]
    r[:, :, 7:10] = rows7[:, :, 4:7]
    return r


def test_g4_fixed_step_trajectories(gold, models):
    rows, nrows, stop = trace_golden_rays(gold, models, "fixed")
    ref, rn, rs = gold["run_fixed_rows"], gold["run_fixed_nrows"], gold["run_fixed_stop"]
    sh, shn, shs = gold["run_fixed_shift_rows"], gold["run_fixed_shift_nrows"], gold["run_fixed_shift_stop"]
    steady = (rn == shn) & (rs == shs)      # rays whose fate the reference itself keeps under its 1e-9 shift
    assert steady.sum() >= 56
    assert np.array_equal(nrows[steady], rn[steady]) and np.array_equal(stop[steady], rs[steady])
    worst = 0.0
    for i in np.nonzero(steady & (rn > 1))[0]:
        T = rn[i]
        assert np.array_equal(rows[i, 0, 1:4], ref[i, 0, 1:4])
        e = vrel(rows[i, :T, 1:4], ref[i, :T, 1:4]).max()
        own = vrel(sh[i, :T, 1:4], ref[i, :T, 1:4]).max()
        bar = 10.0 * max(own, 1e-8)             # floor: the G3 median bar
        worst = max(worst, e / bar)
        assert e <= bar, (i, e, own)
        assert np.allclose(rows[i, :T, 0], ref[i, :T, 0], rtol=1e-14, atol=0)
    print("G4 fixed: worst error / bar = %.3g" % worst)


def test_g4_adaptive_trajectories(gold, models):
    from test_gpu_trajectory_stats import compare
    _, tmax = run_params(gold, "adaptive")
    mine_run = trace_golden_rays(gold, models, "adaptive")
    ref = (widen(gold["run_adaptive_rows"]), gold["run_adaptive_nrows"], gold["run_adaptive_stop"])
    sh = (widen(gold["run_adaptive_shift_rows"]), gold["run_adaptive_shift_nrows"], gold["run_adaptive_shift_stop"])
    cap = ref[0].shape[1]
    mine = compare((mine_run[0][:, :cap], mine_run[1], mine_run[2]), ref, tmax)
    yard = compare(sh, ref, tmax)
    msg = "\nGPU vs reference: %s\nreference vs reference (launch shifted 1e-9): %s\ncurve ratio: median %.2f p90 %.2f" % (
        mine, yard, mine["curve_median"] / yard["curve_median"], mine["curve_p90"] / yard["curve_p90"])
    print(msg)
    n = len(ref[1])
    assert mine["n_curves"] >= 48
    both = (mine_run[1] > 1) & (ref[1] > 1)
    assert np.array_equal(mine_run[0][both, 0, 1:4], ref[0][both, 0, 1:4])
    # curves: no further from the reference than 2 x the reference is from itself (floors: the survey ladder's, as for the
    # other models' adaptive trajectories)
    assert mine["curve_median"] <= 2 * max(yard["curve_median"], 7e-8), msg
    assert mine["curve_p90"] <= 2 * max(yard["curve_p90"], 4e-5), msg
    # decisions: stop codes and row counts
    assert mine["stop_agree"] >= yard["stop_agree"] - 1.5 / n, msg
    assert mine["same_t"] >= yard["same_t"] - 2.5 / n, msg
    assert mine["rows_rel"] <= max(2 * yard["rows_rel"], 0.02), msg


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
    p, _ = run_params(gold, "adaptive")
    pos0, d, w = gold["run_pos0"].copy(), gold["run_dir0"], gold["run_w0"]
    base = models["a"].trace(pos0, d, w, params=p)
    k = 5
    pos0[k] = [0.0, 0.0, 2.0 * wl.R_E]
    rows, nrows, stop, _ = models["a"].trace(pos0, d, w, params=p)
    assert 0 <= stop[k] <= 9 and 1 <= nrows[k] <= int(gold["run_adaptive_params"][5])
    others = np.arange(len(w)) != k
    assert np.array_equal(nrows[others], base[1][others]) and np.array_equal(stop[others], base[2][others])
    assert np.array_equal(np.nan_to_num(rows[others]), np.nan_to_num(base[0][others]))
    # the density there is what the layered entry point gives for the same point: finite or not, never a fault
    g = models["a"].plasma_params(pos0[k:k + 1])
    assert g.shape == (1, 19)


@pytest.mark.parametrize("tag", ["a", "c"])
def test_tail_modes_give_the_bits_of_a_full_wave(gold, models, tag):
    """The 64 golden rays in one wave (every lane evaluates its own stencil) and each ray alone (1 needy lane: its stencil is
    spread over four lanes, the offset points of its right-hand sides over eight): rows, row counts and stop codes bit for bit."""
    p, _ = run_params(gold, "adaptive")
    pos0, d, w = gold["run_pos0"], gold["run_dir0"], gold["run_w0"]
    rows, nrows, stop, _ = models[tag].trace(pos0, d, w, params=p)
    assert nrows.max() > 8
    for i in range(len(w)):
        r1, n1, s1, _ = models[tag].trace(pos0[i:i + 1], d[i:i + 1], w[i:i + 1], params=p)
        assert n1[0] == nrows[i] and s1[0] == stop[i], (i, n1[0], nrows[i], s1[0], stop[i])
        assert np.array_equal(r1[0, :n1[0]], rows[i, :n1[0]], equal_nan=True), i


NX, NY, NZ = 6, 5, 4
BOUNDS = np.array([1.3, 4.5, -2.0, 2.5, -1.5, 1.8]) * wl.R_E


@pytest.mark.parametrize("compder", [0, 1])
def test_grid_built_from_the_handle(models, compder):
    g = models["a"]
    F, D = g.build_grid(NX, NY, NZ, BOUNDS, compder=bool(compder))
    x = np.arange(NX) * ((BOUNDS[1] - BOUNDS[0]) / (NX - 1.0)) + BOUNDS[0]
    y = np.arange(NY) * ((BOUNDS[3] - BOUNDS[2]) / (NY - 1.0)) + BOUNDS[2]
    z = np.arange(NZ) * ((BOUNDS[5] - BOUNDS[4]) / (NZ - 1.0)) + BOUNDS[4]
    Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
    P = np.stack([X, Y, Z], axis=-1)
    mine = np.log(g.plasma_params(P.reshape(-1, 3))[:, 4:8]).reshape(F.shape)
    assert np.all(np.isfinite(F))
    assert np.abs(F - mine).max() <= 2e-14        # device log vs host log of the same densities
    assert (D is None) == (not compder)
    if compder:
        assert len(D) == 7 and all(np.all(np.isfinite(b)) for b in D)
    # the model-3 handle made from it traces
    t = g.to_interp(NX, NY, NZ, BOUNDS, compder=bool(compder))
    assert t.kind == 3
    pos, d, w = wl.launch_set(64, 11)
    rows, nrows, stop, steps = t.trace(pos * 0.5, d, w, fixedstep=1, dt0=1e-3, dtmax=0.1, tmax=0.01, maxerr=5e-4, maxsteps=8, del_=1e-6)
    assert steps > 0 and set(np.unique(stop).tolist()) <= {0, 1, 2, 3, 5, 6, 9}
    at_nodes = t.plasma_params(P.reshape(-1, 3))[:, 4:8]
    assert np.abs(np.log(at_nodes) - F.reshape(-1, 4)).max() <= 1e-12 * np.abs(F).max()


def test_sample_builder_accepts_the_handle(models):
    rec, counts = models["a"].build_samples(BOUNDS, n_initial_uniform=200, seed=3)
    assert rec.shape == (200, 7) and counts[2] == 200
    want = np.log(models["a"].plasma_params(rec[:, 0:3])[:, 4:8])
    assert np.abs(rec[:, 3:7] - want).max() <= 2e-14
