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
    from test_at64thch_host import check_foot
    check_foot(g0[tag][1], gold, tag)


@pytest.mark.parametrize("tag", list(SETTINGS))
def test_g0_plasma_params(gold, g0, tag):
    from test_at64thch_host import check_density
    g = g0[tag][0]
    check_density(g[:, 4:7], gold, tag)
    eB = vrel(g[:, 16:19], gold["g0_B0_" + tag])
    print("G0 %s: B0 error max %.3g" % (tag, eB.max()))
    assert np.all(g[:, 7] == 0) and np.all(g[:, 12:16] == 0) and np.all(g[:, 3] == 0)
    assert eB.max() <= 2e-7


@pytest.mark.parametrize("tag", ["b", "d"])
def test_device_against_the_host_build_of_the_same_source(gold, g0, tag, tmp_path_factory):
    """The same headers compiled for the host: the device's T04_s takes its elementary functions from srt_fastmath.hpp, the
    host's from libm, so a T04_s component may differ in its last fp32 bit and a trace may then take another step sequence:
    the bars are those against the reference (the reference's own sensitivity), and most points are bit-equal."""
    import test_at64thch_host as th
    L = th.build_host_library(tmp_path_factory.mktemp("at64thch_dev"))
    h = th.Host(L, gold["g0_setting_" + tag], gold["parmod_" + tag])
    x = gold["g0_x_" + tag]
    hf, hn = h.foot(x), h.density(x)
    df, dn = g0[tag][1], g0[tag][0][:, 4:7]
    traced = np.linalg.norm(x, axis=1) - wl.R_E > 400e3   # (the points the model traces, as in the tests against the reference)
    move = np.linalg.norm(df[:, 0:3] - hf[:, 0:3], axis=1)
    err = np.abs(dn - hn) / hn
    print("device vs host %s: feet bit-equal %.1f %%, max distance %.3g; densities bit-equal %.1f %%, max %.3g"
          % (tag, 100 * np.mean(move == 0), move.max(), 100 * np.mean(err == 0), err.max()))
    assert np.all(move[traced] <= th.foot_bar(gold, tag)[traced])
    quiet = gold["g0_sens_" + tag][:, 0] < 1e-5
    assert np.array_equal(df[quiet, 4], hf[quiet, 4])
    assert np.all(err <= np.maximum(1e-6, 10.0 * gold["g0_sens_" + tag]))
    assert np.mean(move[traced] == 0) >= 0.5


def held(err, sens, bar):
    """err / its bar, per sample: the ladder's bar, or 10 x the reference's own recorded sensitivity of that sample where that is
    more (DESIGN section 4's sensitivity clause).  <= 1 means held."""
    return err / np.maximum(bar, 10.0 * sens)


def sens_rel(s, ref):
    """recorded absolute sensitivity of a vector -> relative to the vector"""
    return np.linalg.norm(s, axis=-1) / np.maximum(np.linalg.norm(ref, axis=-1), 1e-300)


def test_g1_dispersion_from_own_plasma_params(gold, models):
    from dispersion_checks import check_dispersion_against_own_params
    check_dispersion_against_own_params(models["a"], gold["g23_state"])


@pytest.mark.parametrize("tag", ["a", "b", "d"])
def test_g2_gradients_and_right_hand_side(gold, models, tag):
    st, ref, sn = gold["g23_state"], gold["g2_" + tag], gold["g2_sens_" + tag]
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


@pytest.mark.parametrize("tag", ["a", "b", "d"])
def test_g3_single_steps(gold, models, tag):
    st, ref, sn = gold["g23_state"], gold["g3_" + tag], gold["g3_sens_" + tag]
    g = models[tag].rk_step(st, np.full(len(st), float(gold["g3_dt"])), DEL)
    for o in (0, 7, 14):
        ex, sx = vrel(g[:, o:o + 3], ref[:, o:o + 3]), sens_rel(sn[:, o:o + 3], ref[:, o:o + 3])
        ek, sk = vrel(g[:, o + 3:o + 6], ref[:, o + 3:o + 6]), sens_rel(sn[:, o + 3:o + 6], ref[:, o + 3:o + 6])
        print("G3 %s out %d: position median %.3g max %.3g (own %.3g), k median %.3g max %.3g (own %.3g)"
              % (tag, o // 7, np.median(ex), ex.max(), sx.max(), np.median(ek), ek.max(), sk.max()))
        assert np.median(held(ex, sx, 1e-8)) <= 1 and held(ex, sx, 1e-7).max() <= 1
        assert np.median(held(ek, sk, 1e-7)) <= 1 and held(ek, sk, 1e-2).max() <= 1
        assert np.array_equal(g[:, o + 6], st[:, 6])  # omega is carried unchanged


def run_params(gold, mode):
    from stanford_raytracer_amd import api
    fixedstep, dt0, dtmax, tmax, maxerr, maxsteps, minalt, del_ = gold["run_%s_params" % mode]
    return api.make_params(dt0=dt0, dtmax=dtmax, tmax=tmax, maxerr=maxerr, maxsteps=int(maxsteps), minalt=minalt,
                           fixedstep=int(fixedstep), del_=del_, outputper=1), float(tmax)


def trace_golden_rays(gold, models, mode):
    """The 16 golden rays, in setting d: one launch."""
    p, _ = run_params(gold, mode)
    pos0, d, w = gold["run_pos0"], gold["run_dir0"], gold["run_w0"]
    return models["d"].trace(pos0, d, w, params=p)[:3]


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
    assert steady.sum() >= 14
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
    assert mine["n_curves"] >= 15 == yard["n_curves"]  # (the sixteenth ray stops at its launch point, on both)
    both = (mine_run[1] > 1) & (ref[1] > 1)
    assert np.array_equal(mine_run[0][both, 0, 1:4], ref[0][both, 0, 1:4])
    # curves: no further from the reference than 2 x the reference is from itself (floors: the survey ladder's, as for the
    # other models' adaptive trajectories)
    assert mine["curve_median"] <= 2 * max(yard["curve_median"], 7e-8), msg
    assert mine["curve_p90"] <= 2 * max(yard["curve_p90"], 4e-5), msg
    # decisions: stop codes and row counts
    assert mine["stop_agree"] >= yard["stop_agree"] - 1.5 / n, msg
    assert mine["rows_rel"] <= max(2 * yard["rows_rel"], 0.02), msg
    # the time stamps of all kept rows
    def same_t(run):
        full = (run[1] == ref[1]) & (ref[1] > 1)
        return np.mean([np.array_equal(run[0][i, :ref[1][i], 0], ref[0][i, :ref[1][i], 0]) for i in np.nonzero(full)[0]])
    assert same_t(mine_run) >= same_t(sh) - 2.5 / n, msg


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
    NX, NY, NZ = 4, 4, 3
    B = np.array([1.3, 4.5, -2.0, 2.5, -1.5, 1.8]) * wl.R_E
    g = models["a"]
    F, D = g.build_grid(NX, NY, NZ, B, compder=False)
    assert F.shape == (NZ, NY, NX, 3) and D is None
    x = np.arange(NX) * ((B[1] - B[0]) / (NX - 1.0)) + B[0]
    y = np.arange(NY) * ((B[3] - B[2]) / (NY - 1.0)) + B[2]
    z = np.arange(NZ) * ((B[5] - B[4]) / (NZ - 1.0)) + B[4]
    Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
    P = np.stack([X, Y, Z], axis=-1)
    mine = np.log(g.plasma_params(P.reshape(-1, 3))[:, 4:7]).reshape(F.shape)
    assert np.all(np.isfinite(F))
    assert np.abs(F - mine).max() <= 2e-14        # device log vs host log of the same densities
