"""Real GCPM-derived inputs (tests/golden/gcpm_golden.npz, made by tests/golden/make_gcpm_golden.py with the reference's
OWN producers gcpm_dens_model_buildgrid / gcpm_dens_model_buildgrid_random) through the whole ladder G0..G4.

What this data has that workloads.analytic_lnN does not (all of it met by BASELINE configs 3-5's "precomputed GCPM grid" /
"random GCPM samples" in the field):
  * the surface of the Earth inside the table: GCPM returns its floor below it (the adapter maps exact zeros to 1e-12 cm^-3 =
    ln(1e-6 m^-3) = -13.8: no log(0), no NaN node ever reaches a file) and IRI's F2 peak right above it -- a jump of 41 in ln N
    between x-neighbours of the 36^3 grid, which the tricubic turns into overshoots of tens of e-folds inside those cells;
  * the plasmapause step and a day/night asymmetry;
  * samples INSIDE the Earth in the scattered set: the reference's setup skips their nearest-sample search
    (scattered_interp_dens_model_adapter.f95:171), so their stored spacing stays at the placeholder 1.0 (m) -- a quirk no
    analytic fixture reached; the builder's structured shells (400 samples at R_E, 2 500 below R_E + 2 000 km) on top of the
    adaptive refinement, hence a search radius (1.5 x the largest nearest-sample distance of the sparse outer region) that
    holds thousands of ionospheric samples.

CPU tests: the oracle against the reference's outputs.  GPU tests (-m gpu): the HIP path against the same outputs, at the
bars of the analytic fixtures (tests/test_gpu_parity.py, tests/test_gpu_trace.py) unless a comment says otherwise.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR, vrel
from stanford_raytracer_amd import workloads as wl

gpu = pytest.mark.gpu


def rel(a, b):
    return np.abs(a - b) / np.maximum(np.abs(b), 1e-300)


def close(a, b, rtol):
    a, b = np.asarray(a), np.asarray(b)
    both_nan = np.isnan(a) & np.isnan(b)
    return np.all(both_nan | (np.abs(a - b) <= rtol * np.abs(b)) | (a == b))


@pytest.fixture(scope="module")
def gc():
    return np.load(os.path.join(GOLDEN_DIR, "gcpm_golden.npz"))


@pytest.fixture(scope="module")
def gcpm_pointsfile(gc, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("gcpm") / "gcpm_points.txt")
    wl.write_points_file(path, gc["pts"], gc["lnN"], gc["pts_bounds"], gc["qs"], gc["ms"])
    return path


def date(gc):
    return dict(yearday=int(gc["yearday"]), msec=int(gc["msec"]))


@pytest.fixture(scope="module")
def oracle_interp(gc):
    from oracle import oracle

    return oracle.Model.interp(gc["grid_F"], gc["grid_bounds"], gc["qs"], gc["ms"], **date(gc))


def oracle_scattered_like_reference(gc, path, true_root=False):
    """The oracle's model-4 state as the reference holds it: every sample's true nearest-sample distance (bit 31 of perm_seed),
    then the ONE sample at the root of the reference's kd-tree back to 0 (its kdtree_nearest starts from the root) unless
    `true_root` (what the HIP path stores).  A root inside the Earth keeps the placeholder either way."""
    from oracle import oracle

    m = oracle.Model.scattered_file(path, perm_seed=2 | 0x80000000, **date(gc))
    rp = gc["ref_root_point"]
    if not true_root and float(rp @ rp) >= wl.R_E ** 2:
        m.set_spacing(rp, 0.0)
    return m


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_what_the_reference_producers_write(gc):
    """No non-finite node or sample; the floor inside the Earth; the steps the fixture is here for."""
    F, lnN, pts = gc["grid_F"], gc["lnN"], gc["pts"]
    assert np.all(np.isfinite(F)) and np.all(np.isfinite(lnN))
    n = F.shape[0]
    b = gc["grid_bounds"]
    ax = np.arange(n) * ((b[1] - b[0]) / (n - 1.0)) + b[0]
    Z, Y, X = np.meshgrid(ax, ax, ax, indexing="ij")
    inside = np.sqrt(X * X + Y * Y + Z * Z) < 0.98 * wl.R_E
    assert inside.sum() > 100
    assert np.allclose(F[inside], np.log(1e-12 * 1e6))                    # gcpm_dens_model_adapter.f95:175-186, :193
    assert np.abs(np.diff(F[..., 0], axis=2)).max() > 30                  # the surface of the Earth between two nodes
    r = np.linalg.norm(pts, axis=1)
    assert (r < wl.R_E - 1.0).sum() > 100                                 # samples inside the Earth
    assert (np.abs(r - wl.R_E) < 1.0).sum() == 400                        # --n_zero_altitude
    assert len(pts) <= 20000 and F.shape[0] <= 48


def test_oracle_interp_on_the_gcpm_grid_is_the_reference(gc, oracle_interp):
    m = oracle_interp
    x, ref = gc["g0_interp_x"], gc["g0_interp_out"]
    mine = np.array([np.concatenate(m.plasma_params(p)) for p in x])
    assert close(mine, ref, 1e-13)
    rows, ref = gc["g1_interp_in"], gc["g1_interp_out"]
    assert close(np.array([m.disp(r[0:3], r[3:6], r[6]) for r in rows]), ref, 1e-12)
    rows, ref = gc["g2_interp_in"], gc["g2_interp_out"]
    assert close(np.array([m.grad(r[0:3], r[3:6], r[6], r[7]) for r in rows]), ref, 1e-12)
    rows, ref = gc["g3_interp_in"], gc["g3_interp_out"]
    assert close(np.array([m.step(r[0:7], r[7], r[8]) for r in rows]), ref, 1e-11)


def run_kw(prm, del_=1e-6):
    return dict(dt0=prm[0], dtmax=prm[1], tmax=prm[2], maxerr=prm[3], minalt=prm[4], maxsteps=int(prm[5]), root=int(prm[6]),
                fixedstep=int(prm[7]), del_=del_)


@pytest.mark.parametrize("tag", ["g4_interp_fixed", "g4_interp_adaptive"])
def test_oracle_interp_trajectories_on_the_gcpm_grid(gc, oracle_interp, tag):
    ref_rows, ref_n, ref_stop = gc[tag + "_rows"], gc[tag + "_nrows"], gc[tag + "_stop"]
    rays = gc["g4_rays"][:len(ref_n)]
    rows, nrows, stop, _ = oracle_interp.trace(rays[:, :3], rays[:, 3:6], rays[:, 6], capacity=int(ref_rows.shape[1]),
                                               **run_kw(gc[tag + "_params"]))
    assert np.array_equal(nrows, ref_n) and np.array_equal(stop, ref_stop)
    for i in range(len(nrows)):
        assert close(rows[i, :nrows[i]], ref_rows[i, :nrows[i]], 1e-9), "ray %d" % i


def test_oracle_scattered_on_the_gcpm_samples(gc, gcpm_pointsfile):
    m = oracle_scattered_like_reference(gc, gcpm_pointsfile)
    assert m.search_radius() == float(gc["ref_maxnearest"]) * 1.5
    x, ref = gc["g0_scattered_x"], gc["g0_scattered_out"]
    mine = np.array([np.concatenate(m.plasma_params(p)) for p in x])
    assert np.array_equal(mine[:, 16:19], ref[:, 16:19], equal_nan=True)
    inside = np.einsum("ij,ij->i", x, x) <= wl.R_E ** 2
    assert inside.sum() >= 4 and np.array_equal(ref[inside, 4:8], np.zeros((inside.sum(), 4)))
    fit = (ref[:, 4] > 0) & (ref[:, 4] != 1)
    assert fit.sum() >= 300 and np.array_equal(mine[~fit, 4:8], ref[~fit, 4:8])
    assert rel(mine[fit, 4:8], ref[fit, 4:8]).max() <= 1e-10               # order of summation only (measured 3e-13)
    rows, ref = gc["g2_scattered_in"], gc["g2_scattered_out"]
    mine = np.array([m.grad(r[0:3], r[3:6], r[6], r[7]) for r in rows])
    assert vrel(mine[:, 0:3], ref[:, 0:3]).max() <= 1e-8
    ex = vrel(mine[:, 4:7], ref[:, 4:7])
    assert np.median(ex) <= 1e-6 and np.percentile(ex, 90) <= 1e-3         # d(ln N) over a 10 m stencil: 1e-13 / 1e-6 amplification


def test_oracle_scattered_placeholder_spacing_inside_the_earth(gc, gcpm_pointsfile):
    """scattered_..adapter.f95:171: samples below R_E never get a nearest-sample distance; their val(nspec+1) stays 1.0.
    Queries just above the surface see such samples in their window, so a build that stored true distances for them would
    move exactly those lookups -- shown here by doing that to one oracle copy."""
    m = oracle_scattered_like_reference(gc, gcpm_pointsfile)
    x, ref = gc["g0_scattered_x"], gc["g0_scattered_out"]
    fit = (ref[:, 4] > 0) & (ref[:, 4] != 1)
    low = fit & (np.linalg.norm(x, axis=1) < 1.5 * wl.R_E)
    assert low.sum() >= 40
    pts = gc["pts"]
    inside = np.where(np.einsum("ij,ij->i", pts, pts) < wl.R_E ** 2)[0]
    assert len(inside) > 100
    for i in inside[:200]:
        d = np.linalg.norm(pts - pts[i], axis=1)
        d[i] = np.inf
        m.set_spacing(pts[i], float(d.min()))
    moved = np.array([np.concatenate(m.plasma_params(p)) for p in x[low]])
    assert rel(moved[:, 4:8], ref[low, 4:8]).max() > 1e-6


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def gpu_interp(gc):
    from stanford_raytracer_amd import api

    api.init(0)
    return api.Model.interp(gc["grid_F"], gc["grid_bounds"], gc["qs"], gc["ms"], **date(gc))


@pytest.fixture(scope="module")
def gpu_scattered(gc, gcpm_pointsfile):
    from stanford_raytracer_amd import api

    api.init(0)
    return api.Model.scattered_file(gcpm_pointsfile, **date(gc))


@gpu
def test_gpu_interp_g0_on_the_gcpm_grid(gc, gpu_interp):
    x, ref = gc["g0_interp_x"], gc["g0_interp_out"]
    g = gpu_interp.plasma_params(x)
    assert np.array_equal(g[:, 0:4], ref[:, 0:4]) and np.array_equal(g[:, 8:12], ref[:, 8:12])
    fin = np.all(np.isfinite(ref[:, 16:19]), axis=1)
    assert fin.sum() >= len(x) - 1                                         # the centre of the Earth: B = NaN in the reference
    assert np.array_equal(np.isfinite(g[:, 16:19]), np.isfinite(ref[:, 16:19]))
    assert vrel(g[fin, 16:19], ref[fin, 16:19]).max() <= 2e-7
    # ln N is a sum of 64 terms of up to e^+-41 size near the surface; N = exp(ln N): relative error of N = absolute error of
    # ln N.  Bar of the analytic grid (1e-11) for the points whose cell has no node inside the Earth, 1e-9 for all
    e = rel(g[:, 4:8], ref[:, 4:8]).max(axis=1)
    far = np.linalg.norm(x, axis=1) > wl.R_E + 3.0e6
    msg = "far max %.3g (n %d), all max %.3g" % (e[far].max(), far.sum(), e.max())
    print(msg)
    assert e[far].max() <= 1e-11 and e.max() <= 1e-9, msg


@gpu
def test_gpu_interp_g1_g2_g3_on_the_gcpm_grid(gc, gpu_interp, oracle_interp):
    from conftest import G3_INTERP_BARS

    g = gpu_interp
    rows, ref = gc["g1_interp_in"], gc["g1_interp_out"]
    out = g.dispersion(rows[:, 0:3], rows[:, 3:6], rows[:, 6])
    assert rel(out[:, 1:6], ref[:, 1:6]).max() <= 1e-10
    # G2 against the reference's outputs.  Bars per sample: 10 x the larger of the analytic grid's bar and the ORACLE's own change
    # under a two-ulp shift of the state (conftest.oracle_grad_sensitivity) -- the launch set scaled by 0.78 holds states below
    # the surface, where the table is the floor ln 1e-6 (a vacuum: dF/dw ~ 1e-12 is rounding noise, the reference moves by 100 %
    # under that shift) and states in the F2 layer where F cancels to twelve digits
    from conftest import grad_errors, oracle_grad_sensitivity, within_sensitivity

    gin, ref = gc["g2_interp_in"], gc["g2_interp_out"]
    out = g.gradients(gin[:, 0:3], gin[:, 3:6], gin[:, 6], 1e-6)
    base, yard = oracle_grad_sensitivity(oracle_interp, gin[:, 0:3], gin[:, 3:6], gin[:, 6], 1e-6)
    assert np.array_equal(base, ref[:, :base.shape[1]])                    # the oracle IS the reference here
    err = grad_errors(out, ref)
    well = np.all(yard <= 1e-7, axis=1)                                    # well-conditioned states: the analytic grid's bars, as is
    assert well.sum() >= 80
    msg = "well-conditioned (%d): dFdk max %.3g; dFdw max %.3g; dFdx median %.3g p95 %.3g; dx/dt max %.3g; dk/dt median %.3g p95 %.3g" % (
        well.sum(), err[well, 0].max(), err[well, 1].max(), np.median(err[well, 2]), np.percentile(err[well, 2], 95), err[well, 3].max(),
        np.median(err[well, 4]), np.percentile(err[well, 4], 95))
    print(msg)
    assert err[well, 0].max() <= 1e-7 and err[well, 1].max() <= 1e-6, msg
    assert np.median(err[well, 2]) <= 1e-7 and np.percentile(err[well, 2], 95) <= 1e-5, msg
    assert err[well, 3].max() <= 1e-6, msg
    assert np.median(err[well, 4]) <= 1e-6 and np.percentile(err[well, 4], 95) <= 2e-5, msg
    for col, (name, floor) in enumerate((("dFdk", 1e-8), ("dFdw", 1e-7), ("dFdx", 1e-6), ("dx/dt", 1e-7), ("dk/dt", 2e-6))):
        fin = np.isfinite(yard[:, col]) & np.isfinite(err[:, col])
        ok, txt = within_sensitivity(err[fin, col], yard[fin, col], floor)
        assert ok, "%s: %s" % (name, txt)
    # G3: one RK step.  The analytic grid's bars (conftest.G3_INTERP_BARS: the reference's own sensitivity THERE) for the states
    # where the oracle moves by less than those bars under a two-ulp shift; every state within 10 x the larger of its own
    # yardstick and the bar (a step that starts under the surface crosses the 41-e-fold jump of the table: the reference's own
    # position moves by tens of per cent under that shift)
    from conftest import oracle_step_sensitivity

    sin, ref = gc["g3_interp_in"], gc["g3_interp_out"]
    out = g.rk_step(sin[:, 0:7], sin[:, 7], 1e-6)
    sbase, syard = oracle_step_sensitivity(oracle_interp, sin[:, 0:7], sin[:, 7], 1e-6)
    assert np.array_equal(sbase, ref, equal_nan=True)                      # the oracle IS the reference here
    b = G3_INTERP_BARS
    for i, o in enumerate((0, 7, 14)):
        ex, ek = vrel(out[:, o:o + 3], ref[:, o:o + 3]), vrel(out[:, o + 3:o + 6], ref[:, o + 3:o + 6])
        well = (syard[:, i, 0] <= b["pos_median"]) & (syard[:, i, 1] <= b["k_median"])
        msg = "step output %d: %d well-conditioned of %d: pos median %.3g max %.3g; k median %.3g p90 %.3g max %.3g; all: pos max %.3g k max %.3g" % (
            o, well.sum(), len(well), np.median(ex[well]), ex[well].max(), np.median(ek[well]), np.percentile(ek[well], 90), ek[well].max(),
            ex.max(), ek.max())
        print(msg)
        assert well.sum() >= 30, msg
        assert np.median(ex[well]) <= b["pos_median"] and ex[well].max() <= b["pos_max"], msg
        assert np.median(ek[well]) <= b["k_median"] and np.percentile(ek[well], 90) <= b["k_p90"] and ek[well].max() <= b["k_max"], msg
        for err, yard, floor, name in ((ex, syard[:, i, 0], b["pos_max"], "position"), (ek, syard[:, i, 1], b["k_max"], "k")):
            fin = np.isfinite(err) & np.isfinite(yard)
            ok, txt = within_sensitivity(err[fin], yard[fin], floor, outliers=0.03)
            assert ok, "step output %d, %s: %s" % (o, name, txt)


@gpu
def test_gpu_interp_fixed_step_trajectories_on_the_gcpm_grid(gc, gpu_interp, oracle_interp):
    from model_ladder import LADDER, divergence, oracle_yardstick

    tag = "g4_interp_fixed"
    ref_rows, ref_n, ref_stop = gc[tag + "_rows"], gc[tag + "_nrows"], gc[tag + "_stop"]
    rays = gc["g4_rays"][:len(ref_n)]
    kw = run_kw(gc[tag + "_params"])
    cap = int(ref_rows.shape[1])
    rows, nrows, stop, steps = gpu_interp.trace(rays[:, :3], rays[:, 3:6], rays[:, 6], outputper=1, **dict(kw, maxsteps=cap + 1))
    assert np.array_equal(nrows, ref_n) and np.array_equal(stop, ref_stop)
    assert np.array_equal(rows[:, 0, 0:4], ref_rows[:, 0, 0:4])
    rows_at = (1, 10, 50)
    _, yard = oracle_yardstick(oracle_interp, rays, dict(kw, maxsteps=cap + 1), rows_at, cap)
    for r in rows_at:
        d = divergence(rows, nrows, ref_rows, ref_n, r, slice(1, 4))
        bound = 10 * max(yard[r], LADDER.get(r, 4e-5))
        assert d <= bound, "row %d: position divergence %.2e > %.2e" % (r, d, bound)


@gpu
def test_gpu_interp_adaptive_trajectories_on_the_gcpm_grid(gc, gpu_interp, oracle_interp):
    from model_ladder import curve_distance

    tag = "g4_interp_adaptive"
    ref_rows, ref_n, ref_stop = gc[tag + "_rows"], gc[tag + "_nrows"], gc[tag + "_stop"]
    rays = gc["g4_rays"][:len(ref_n)]
    prm = gc[tag + "_params"]
    kw = run_kw(prm)
    cap = int(ref_rows.shape[1])
    rows, nrows, stop, _ = gpu_interp.trace(rays[:, :3], rays[:, 3:6], rays[:, 6], outputper=1, **kw)
    base = oracle_interp.trace(rays[:, :3], rays[:, 3:6], rays[:, 6], capacity=cap, **kw)
    assert np.array_equal(base[1], ref_n) and np.array_equal(base[2], ref_stop)     # the oracle IS the reference here
    yard_curve, yard_stop, yard_rows = 0.0, 1.0, 0
    for eps in (1e-9, -1e-9):
        pert = oracle_interp.trace(rays[:, :3] * (1 + eps), rays[:, 3:6], rays[:, 6], capacity=cap, **kw)
        yard_curve = max(yard_curve, curve_distance(pert[0], pert[1], base[0], base[1], prm[2]))
        yard_stop = min(yard_stop, float(np.mean(pert[2] == base[2])))
        yard_rows = max(yard_rows, abs(int(pert[1].sum()) - int(base[1].sum())))
    msg = "stop agreement %.3f (oracle vs itself %.3f); rows %d vs %d (oracle vs itself +-%d); curve %.3g (oracle vs itself %.3g)" % (
        np.mean(stop == ref_stop), yard_stop, nrows.sum(), ref_n.sum(), yard_rows,
        curve_distance(rows[:, :cap], np.minimum(nrows, cap), ref_rows, ref_n, prm[2]), yard_curve)
    print(msg)
    assert np.mean(stop == ref_stop) >= min(0.9, yard_stop - 1.0 / len(stop)), msg
    both = (nrows > 2) & (ref_n > 2)
    assert np.allclose(rows[both, 1, 0], prm[0]) and np.all(rows[both, 2, 0] <= 2 * prm[0] * (1 + 1e-12))
    assert abs(int(nrows.sum()) - int(ref_n.sum())) <= max(3 * yard_rows, 0.05 * ref_n.sum()), msg
    assert curve_distance(rows[:, :cap], np.minimum(nrows, cap), ref_rows, ref_n, prm[2]) <= max(3 * yard_curve, 1e-3), msg


@gpu
def test_gpu_scattered_g0_on_the_gcpm_samples(gc, gpu_scattered, gcpm_pointsfile):
    """funcPlasmaParams of modelnum 4 on the reference builder's own sample set.  The HIP path stores the true nearest-sample
    distance for the sample at the root of the reference's kd-tree (documented divergence): the lookups
    whose window holds that sample are held against the oracle with true distances, all others against the reference."""
    x, ref = gc["g0_scattered_x"], gc["g0_scattered_out"]
    g = gpu_scattered.plasma_params(x)
    assert np.array_equal(g[:, 0:4], ref[:, 0:4]) and np.array_equal(g[:, 8:12], ref[:, 8:12])
    fin = np.all(np.isfinite(ref[:, 16:19]), axis=1)
    assert vrel(g[fin, 16:19], ref[fin, 16:19]).max() <= 2e-7
    fit = (ref[:, 4] > 0) & (ref[:, 4] != 1)
    assert np.array_equal(g[~fit, 4:8], ref[~fit, 4:8])                     # inside the Earth -> 0, too few samples -> exp(0)
    radius = float(gc["ref_maxnearest"]) * 1.5
    rp = gc["ref_root_point"]
    near = (np.linalg.norm(x - rp, axis=1) < radius) & (float(rp @ rp) >= wl.R_E ** 2)
    far = fit & ~near
    e = rel(g[far, 4:8], ref[far, 4:8]).max(axis=1)
    msg = "%d lookups with a fit, %d near the reference's tree root; max %.3g, p99 %.3g, median %.3g" % (
        fit.sum(), (fit & near).sum(), e.max(), np.percentile(e, 99), np.median(e))
    print(msg)
    # the analytic fixture's bar is 1e-9; here windows hold up to thousands of ionospheric samples spanning 40 e-folds
    assert e.max() <= 1e-8 and np.percentile(e, 99) <= 1e-9, msg
    if (fit & near).any():
        o = oracle_scattered_like_reference(gc, gcpm_pointsfile, true_root=True)
        on = np.array([np.concatenate(o.plasma_params(p)) for p in x[fit & near]])
        assert rel(g[fit & near, 4:8], on[:, 4:8]).max() <= 1e-8


@gpu
def test_gpu_scattered_gradients_and_trajectories_on_the_gcpm_samples(gc, gpu_scattered, gcpm_pointsfile):
    from model_ladder import compare

    g = gpu_scattered
    o = oracle_scattered_like_reference(gc, gcpm_pointsfile, true_root=True)
    gin, ref = gc["g2_scattered_in"], gc["g2_scattered_out"]
    radius = float(gc["ref_maxnearest"]) * 1.5
    far = np.linalg.norm(gin[:, 0:3] - gc["ref_root_point"], axis=1) >= radius + 100.0
    out = g.gradients(gin[:, 0:3], gin[:, 3:6], gin[:, 6], 1e-6)
    assert far.sum() >= 30
    ex = vrel(out[far, 4:7], ref[far, 4:7])
    msg = "dFdk max %.3g; dFdw max %.3g; dFdx median %.3g p90 %.3g" % (vrel(out[far, 0:3], ref[far, 0:3]).max(),
                                                                     rel(out[far, 3], ref[far, 3]).max(), np.median(ex), np.percentile(ex, 90))
    print(msg)
    assert vrel(out[far, 0:3], ref[far, 0:3]).max() <= 1e-7 and rel(out[far, 3], ref[far, 3]).max() <= 1e-6, msg
    assert np.median(ex) <= 1e-5 and np.percentile(ex, 90) <= 1e-3, msg
    # fixed-step rows: the time grid and the fates of the reference; positions at the yardstick of the oracle against itself
    tag = "g4_scattered_fixed"
    ref_rows, ref_n, ref_stop = gc[tag + "_rows"], gc[tag + "_nrows"], gc[tag + "_stop"]
    rays = gc["g4_rays"][:len(ref_n)]
    kw = run_kw(gc[tag + "_params"])
    cap = int(ref_rows.shape[1])
    rows, nrows, stop, _ = g.trace(rays[:, :3], rays[:, 3:6], rays[:, 6], outputper=1, **dict(kw, maxsteps=cap + 1))
    assert np.array_equal(nrows, ref_n) and np.array_equal(stop, ref_stop)
    both = ref_n > 10
    d10 = vrel(rows[both, 10, 1:4], ref_rows[both, 10, 1:4]).max()
    base = o.trace(rays[:, :3], rays[:, 3:6], rays[:, 6], capacity=cap, **dict(kw, maxsteps=cap + 1))
    pert = o.trace(rays[:, :3] * (1 + 1e-9), rays[:, 3:6], rays[:, 6], capacity=cap, **dict(kw, maxsteps=cap + 1))
    y10 = vrel(pert[0][both, 10, 1:4], base[0][both, 10, 1:4]).max()
    assert d10 <= 10 * max(y10, 7e-8), "row 10: %.3g (oracle vs itself under a 1e-9 shift: %.3g)" % (d10, y10)
    # adaptive rows
    tag = "g4_scattered_adaptive"
    ref_rows, ref_n, ref_stop = gc[tag + "_rows"], gc[tag + "_nrows"], gc[tag + "_stop"]
    rays = gc["g4_rays"][:len(ref_n)]
    prm = gc[tag + "_params"]
    kw = run_kw(prm)
    cap = int(ref_rows.shape[1])
    rows, nrows, stop, _ = g.trace(rays[:, :3], rays[:, 3:6], rays[:, 6], outputper=1, **kw)
    ref = (ref_rows, ref_n, ref_stop)
    base = o.trace(rays[:, :3], rays[:, 3:6], rays[:, 6], capacity=cap, **kw)[:3]
    oref = compare(base, ref, prm[2])
    yard = None
    for eps in (1e-9, -1e-9):
        pert = o.trace(rays[:, :3] * (1 + eps), rays[:, 3:6], rays[:, 6], capacity=cap, **kw)[:3]
        c = compare(pert, base, prm[2])
        yard = c if yard is None else {k: (min if k in ("stop_agree", "same_t") else max)(yard[k], c[k]) for k in c}
    mine = compare((rows[:, :cap], np.minimum(nrows, cap), stop), ref, prm[2])
    msg = "\nGPU vs reference: %s\noracle vs reference: %s\noracle vs oracle(launch shifted 1e-9): %s" % (mine, oref, yard)
    print(msg)
    worst = {k: (min if k in ("stop_agree", "same_t") else max)(yard[k], oref[k]) for k in yard}
    n = len(ref_n)
    assert mine["curve_median"] <= 3 * max(worst["curve_median"], 7e-8), msg
    assert mine["curve_p90"] <= 3 * max(worst["curve_p90"], 4e-5), msg
    assert mine["stop_agree"] >= worst["stop_agree"] - 1.5 / n, msg
    assert mine["same_t"] >= worst["same_t"] - 2.5 / n, msg
    assert mine["rows_rel"] <= max(3 * worst["rows_rel"], 0.02), msg
