"""The parity ladder G0 .. G4 of a density model that has a golden from the real reference (modelnum 5, 6, 7) and the checks of
its builders: the one copy of every bar, shared by tests/test_gpu_{simple3d,ngo3d,at64thch}.py and the host tests of the same
models, each of which keeps its golden, its make_model, its settings and one short test per rung.  tests/test_model_ladder.py
proves on the goldens alone that these checks pass the reference and fail a sample 1 % over its bar.  Not a test module: its
asserts carry their own messages (the worst offender and its bar), because pytest rewrites asserts in test modules only.

Every bar comes with DESIGN section 4's sensitivity clause: a sample is held no tighter than 10 x what the reference itself
does to that sample under the golden's recorded shift of the inputs."""
import numpy as np

from conftest import vrel
from stanford_raytracer_amd import workloads as wl

C_LIGHT = 299792458.0
BOUNDS = np.array([1.3, 4.5, -2.0, 2.5, -1.5, 1.8]) * wl.R_E  # of the grids and sample sets built from a handle


def held(err, sens, bar):
    """err / its bar, per sample: the ladder's bar, or 10 x the reference's own recorded sensitivity of that sample where that is
    more (DESIGN section 4's sensitivity clause).  <= 1 means held."""
    return err / np.maximum(bar, 10.0 * sens)


def sens_rel(s, ref):
    """recorded absolute sensitivity of a vector -> relative to the vector"""
    return np.linalg.norm(s, axis=-1) / np.maximum(np.linalg.norm(ref, axis=-1), 1e-300)


def offender(what, err, sens, bar):
    """for an assert's message: the sample furthest over max(bar, 10 x its sensitivity)"""
    i = int(np.argmax(held(err, sens, bar)))
    return "%s: sample %d has error %.3g over its bar %.3g (fixed bar %.3g, 10 x own sensitivity %.3g); median error / bar %.3g" % (
        what, i, err[i], max(bar, 10.0 * sens[i]), bar, 10.0 * sens[i], np.median(held(err, sens, bar)))


def run_params(gold, mode):
    from stanford_raytracer_amd import api
    fixedstep, dt0, dtmax, tmax, maxerr, maxsteps, minalt, del_ = gold["run_%s_params" % mode]
    return api.make_params(dt0=dt0, dtmax=dtmax, tmax=tmax, maxerr=maxerr, maxsteps=int(maxsteps), minalt=minalt,
                           fixedstep=int(fixedstep), del_=del_, outputper=1), float(tmax)


def widen(rows7):
    """golden rows (t, pos, vgrel) -> the library's 20-column layout (only those columns filled)"""
    r = np.full(rows7.shape[:2] + (20,), np.nan)
    r[:, :, 0:4] = rows7[:, :, 0:4]
    r[:, :, 7:10] = rows7[:, :, 4:7]
    return r


def trace_golden_rays(gold, launches, mode):
    """The golden rays, one launch per (model, slice of the rays) of `launches` -> rows, nrows, stop of all of them."""
    p, _ = run_params(gold, mode)
    pos0, d, w = gold["run_pos0"], gold["run_dir0"], gold["run_w0"]
    out = [m.trace(pos0[h], d[h], w[h], params=p)[:3] for m, h in launches]
    return tuple(np.concatenate([o[k] for o in out]) for k in range(3))


# ---- trajectory comparison (also the trace tests of the other models: tests/test_gpu_trace.py, test_gpu_trajectory_stats.py,
# test_gpu_parity.py, test_gcpm_golden.py, test_root1_golden.py) ----------------------------------------------------------
def hermite(tt, t, y, v):
    idx = np.clip(np.searchsorted(t, tt, side="right") - 1, 0, len(t) - 2)
    h = t[idx + 1] - t[idx]
    u = (tt - t[idx]) / h
    h00, h10, h01, h11 = 2 * u**3 - 3 * u**2 + 1, u**3 - 2 * u**2 + u, -2 * u**3 + 3 * u**2, u**3 - u**2
    return h00[:, None] * y[idx] + (h10 * h)[:, None] * v[idx] + h01[:, None] * y[idx + 1] + (h11 * h)[:, None] * v[idx + 1]


def curve_distances(ra, na, rb, nb, tmax):
    """per ray: max relative distance between the two position curves on a common time grid (NaN: too short)."""
    out = np.full(ra.shape[0], np.nan)
    for i in range(ra.shape[0]):
        ta, tb = ra[i, :na[i], 0], rb[i, :nb[i], 0]
        if len(ta) < 3 or len(tb) < 3:
            continue
        tt = np.linspace(0, min(ta[-1], tb[-1], tmax), 20)
        pa = hermite(tt, ta, ra[i, :na[i], 1:4], ra[i, :na[i], 7:10] * C_LIGHT)
        pb = hermite(tt, tb, rb[i, :nb[i], 1:4], rb[i, :nb[i], 7:10] * C_LIGHT)
        out[i] = float(vrel(pa, pb).max())
    return out


def compare(a, b, tmax):
    """statistics of run a against run b (each = rows, nrows, stop)."""
    (ra, na, sa), (rb, nb, sb) = a, b
    d = curve_distances(ra, na, rb, nb, tmax)
    d = d[np.isfinite(d)]
    both = (na > 4) & (nb > 4)
    same_t = np.all(ra[both, 1:4, 0] == rb[both, 1:4, 0], axis=1)
    return {"curve_median": float(np.median(d)), "curve_p90": float(np.percentile(d, 90)), "curve_p99": float(np.percentile(d, 99)),
            "stop_agree": float(np.mean(sa == sb)), "same_t": float(same_t.mean()), "n_curves": int(len(d)),
            "rows_rel": abs(int(na.sum()) - int(nb.sum())) / max(int(nb.sum()), 1)}


def curve_distance(rows_a, n_a, rows_b, n_b, tmax):
    """max over rays of the relative distance between the two position curves on a common time grid (0: no ray long enough).
    Adaptive runs place their knots differently, so both curves are resampled with cubic Hermite interpolation using the
    group velocity (vgrel * c) the rows carry."""
    d = curve_distances(rows_a, n_a, rows_b, n_b, tmax)
    d = d[~np.isnan(d)]
    return float(d.max()) if len(d) else 0.0


LADDER = {1: 1.2e-10, 10: 7e-8, 100: 4e-5}  # the reference against its own FMA rebuild after 1 / 10 / 100 fixed steps (SURVEY A-9)


def divergence(ra, na, rb, nb, r, cols):
    sel = (na > r) & (nb > r)
    if not sel.any():
        return 0.0
    return float(vrel(ra[sel, r][:, cols], rb[sel, r][:, cols]).max())


def oracle_yardstick(om, rays, kw, rows_at, cap):
    base = om.trace(rays[:, :3], rays[:, 3:6], rays[:, 6], capacity=cap, **kw)
    out = {r: 0.0 for r in rows_at}
    for eps in (1e-9, -1e-9):
        pert = om.trace(rays[:, :3] * (1 + eps), rays[:, 3:6], rays[:, 6], capacity=cap, **kw)
        for r in rows_at:
            out[r] = max(out[r], divergence(pert[0], pert[1], base[0], base[1], r, slice(1, 4)))
    return base, out


# ---- G0 ----------------------------------------------------------------------------------------------------------------
def check_g0_density(got, gold, tag, floor, per_species, report=None):
    """Densities got[n, nspec] at the golden's points of setting `tag`: err <= max(floor, 10 x the reference's recorded
    sensitivity), no point skipped.  per_species: each species against its own sensitivity (modelnum 7: floor 1e-6); otherwise
    the largest error over a point's species against the point's sensitivity (modelnum 5, 6: floor 1e-11, the project's G0 bar).
    report(err): the caller's figure line, printed before anything is asserted; modelnum 7's own line without one."""
    want, sens = gold["g0_Ns_" + tag], gold["g0_sens_" + tag]
    err = np.abs(got - want) / want
    if not per_species:
        err = np.max(err, axis=1)
    bar = np.maximum(floor, 10.0 * sens)
    if report is not None:
        report(err)
    else:
        print("density %s: %d points, error max %.3g (bit-equal %.1f %%), worst error / bar %.3g" % (tag, len(want), err.max(), 100 * np.mean(err == 0), np.max(err / bar)))
    assert np.all(np.isfinite(got)), "%s: %d densities are not finite" % (tag, (~np.isfinite(got)).sum())
    assert np.all(err <= bar), "%d points over their bar, worst ratio %.3g" % ((err > bar).sum(), np.max(err / bar))


# ---- G2, G3 --------------------------------------------------------------------------------------------------------------
def check_g2(model, state, ref, sens, del_, tag):
    """srt_gradients at the golden states [x, k, w] against the reference's dFdk, dFdw, dFdx, dx/dt, dk/dt."""
    st, sn = state, sens
    g = model.gradients(st[:, 0:3], st[:, 3:6], st[:, 6], del_)
    ek, sk = vrel(g[:, 0:3], ref[:, 0:3]), sens_rel(sn[:, 0:3], ref[:, 0:3])
    ew, sw = np.abs(g[:, 3] - ref[:, 3]) / np.abs(ref[:, 3]), sn[:, 3] / np.abs(ref[:, 3])
    ex, sx = vrel(g[:, 4:7], ref[:, 4:7]), sens_rel(sn[:, 4:7], ref[:, 4:7])
    ev, sv = vrel(g[:, 7:10], ref[:, 7:10]), sens_rel(sn[:, 7:10], ref[:, 7:10])
    ed, sd = vrel(g[:, 10:13], ref[:, 10:13]), sens_rel(sn[:, 10:13], ref[:, 10:13])
    print("G2 %s: dFdk %.3g dFdw %.3g dFdx %.3g (reference's own %.3g) dx/dt %.3g dk/dt median %.3g max %.3g (own %.3g)"
          % (tag, ek.max(), ew.max(), ex.max(), sx.max(), ev.max(), np.median(ed), ed.max(), sd.max()))
    assert held(ek, sk, 1e-7).max() <= 1, offender("dFdk", ek, sk, 1e-7)
    assert held(ew, sw, 1e-6).max() <= 1, offender("dFdw", ew, sw, 1e-6)
    assert held(ex, sx, 1e-7).max() <= 1, offender("dFdx", ex, sx, 1e-7)
    assert held(ev, sv, 1e-6).max() <= 1, offender("dx/dt", ev, sv, 1e-6)
    assert np.median(held(ed, sd, 1e-6)) <= 1 and held(ed, sd, 2e-5).max() <= 1, offender("dk/dt median", ed, sd, 1e-6) + "; " + offender("dk/dt max", ed, sd, 2e-5)


def check_g3(model, state, ref, sens, dt, del_, tag):
    """One rk4 / rk45 step (the three outputs rk4, rkf45 4th and 5th order) from the golden states: position median 1e-8 and max
    1e-7, k median 1e-7 and max 1e-2, omega carried unchanged."""
    st, sn = state, sens
    g = model.rk_step(st, np.full(len(st), float(dt)), del_)
    for o in (0, 7, 14):
        ex, sx = vrel(g[:, o:o + 3], ref[:, o:o + 3]), sens_rel(sn[:, o:o + 3], ref[:, o:o + 3])
        ek, sk = vrel(g[:, o + 3:o + 6], ref[:, o + 3:o + 6]), sens_rel(sn[:, o + 3:o + 6], ref[:, o + 3:o + 6])
        print("G3 %s out %d: position median %.3g max %.3g (own %.3g), k median %.3g max %.3g (own %.3g)"
              % (tag, o // 7, np.median(ex), ex.max(), sx.max(), np.median(ek), ek.max(), sk.max()))
        assert np.median(held(ex, sx, 1e-8)) <= 1 and held(ex, sx, 1e-7).max() <= 1, \
            "out %d: %s; %s" % (o // 7, offender("position median", ex, sx, 1e-8), offender("position max", ex, sx, 1e-7))
        assert np.median(held(ek, sk, 1e-7)) <= 1 and held(ek, sk, 1e-2).max() <= 1, \
            "out %d: %s; %s" % (o // 7, offender("k median", ek, sk, 1e-7), offender("k max", ek, sk, 1e-2))
        assert np.array_equal(g[:, o + 6], st[:, 6]), "out %d: omega is not carried unchanged" % (o // 7)


# ---- G4 ------------------------------------------------------------------------------------------------------------------
def check_g4_fixed(run, gold, min_steady):
    """Fixed-step trajectories run = (rows, nrows, stop) of the golden rays: on the rays whose fate the reference itself keeps
    under its 1e-9 shift of the launch point (at least min_steady of them), the reference's row counts and stop codes, and every
    row's position within 10 x max(what that shift does to the ray, 1e-8)."""
    rows, nrows, stop = run
    ref, rn, rs = gold["run_fixed_rows"], gold["run_fixed_nrows"], gold["run_fixed_stop"]
    sh, shn, shs = gold["run_fixed_shift_rows"], gold["run_fixed_shift_nrows"], gold["run_fixed_shift_stop"]
    steady = (rn == shn) & (rs == shs)      # rays whose fate the reference itself keeps under its 1e-9 shift
    assert steady.sum() >= min_steady, "%d steady rays, %d needed" % (steady.sum(), min_steady)
    assert np.array_equal(nrows[steady], rn[steady]) and np.array_equal(stop[steady], rs[steady]), \
        "row counts differ on rays %s, stop codes on rays %s" % (np.nonzero(steady & (nrows != rn))[0], np.nonzero(steady & (stop != rs))[0])
    worst = 0.0
    for i in np.nonzero(steady & (rn > 1))[0]:
        T = rn[i]
        assert np.array_equal(rows[i, 0, 1:4], ref[i, 0, 1:4]), "ray %d: row 0 is not the launch point" % i
        e = vrel(rows[i, :T, 1:4], ref[i, :T, 1:4]).max()
        own = vrel(sh[i, :T, 1:4], ref[i, :T, 1:4]).max()
        bar = 10.0 * max(own, 1e-8)             # floor: the G3 median bar
        worst = max(worst, e / bar)
        assert e <= bar, "ray %d: error %.3g over its bar %.3g (the reference's own %.3g)" % (i, e, bar, own)
        assert np.allclose(rows[i, :T, 0], ref[i, :T, 0], rtol=1e-14, atol=0), "ray %d: time stamps differ" % i
    print("G4 fixed: worst error / bar = %.3g" % worst)


def same_t_first_rows(run, ref, stats):
    """share of rays whose rows 1 .. 3 carry the reference's time stamps: compare()'s figure"""
    return stats["same_t"]


def same_t_all_rows(run, ref, stats):
    """share of the rays with the reference's row count whose kept rows all carry the reference's time stamps"""
    full = (run[1] == ref[1]) & (ref[1] > 1)
    return np.mean([np.array_equal(run[0][i, :ref[1][i], 0], ref[0][i, :ref[1][i], 0]) for i in np.nonzero(full)[0]])


def check_g4_adaptive(run, gold, min_curves, same_t, yard_curves=None):
    """Adaptive trajectories run = (rows, nrows, stop) of the golden rays, with the reference's own movement under its 1e-9 shift
    of the launch points as the yardstick (tests/test_gpu_trajectory_stats.py).  same_t(run, ref, stats) -> share of rays with
    the reference's time stamps: same_t_first_rows or same_t_all_rows.  yard_curves: the curves the yardstick must have."""
    tmax = float(gold["run_adaptive_params"][3])
    ref = (widen(gold["run_adaptive_rows"]), gold["run_adaptive_nrows"], gold["run_adaptive_stop"])
    sh = (widen(gold["run_adaptive_shift_rows"]), gold["run_adaptive_shift_nrows"], gold["run_adaptive_shift_stop"])
    cap = ref[0].shape[1]
    mine = compare((run[0][:, :cap], run[1], run[2]), ref, tmax)
    yard = compare(sh, ref, tmax)
    msg = "\nGPU vs reference: %s\nreference vs reference (launch shifted 1e-9): %s\ncurve ratio: median %.2f p90 %.2f" % (
        mine, yard, mine["curve_median"] / yard["curve_median"], mine["curve_p90"] / yard["curve_p90"])
    print(msg)
    n = len(ref[1])
    assert mine["n_curves"] >= min_curves and yard_curves in (None, yard["n_curves"]), msg
    both = (run[1] > 1) & (ref[1] > 1)
    assert np.array_equal(run[0][both, 0, 1:4], ref[0][both, 0, 1:4]), "row 0 is not the launch point on every ray"
    # curves: no further from the reference than 2 x the reference is from itself (floors: the survey ladder's, as for the
    # other models' adaptive trajectories)
    assert mine["curve_median"] <= 2 * max(yard["curve_median"], 7e-8), msg
    assert mine["curve_p90"] <= 2 * max(yard["curve_p90"], 4e-5), msg
    # decisions: stop codes, time stamps and row counts
    assert mine["stop_agree"] >= yard["stop_agree"] - 1.5 / n, msg
    st_mine, st_yard = same_t(run, ref, mine), same_t(sh, ref, yard)
    assert st_mine >= st_yard - 2.5 / n, "same time stamps on %.4f of the rays, the reference's own %.4f%s" % (st_mine, st_yard, msg)
    assert mine["rows_rel"] <= max(2 * yard["rows_rel"], 0.02), msg


def z_axis_ray(gold, model):
    """A launch on the z axis (cos(latitude) is 6e-17, L is 1e33 or infinite, the longitude atan2(0, 0)) in lane 5 of the golden
    rays: it ends within maxsteps rows and the other 63 lanes of its wave produce the rows they produce without it.  Returns
    the axis ray's stop code, which each model's test holds to its own condition."""
    p, _ = run_params(gold, "adaptive")
    pos0, d, w = gold["run_pos0"].copy(), gold["run_dir0"], gold["run_w0"]
    base = model.trace(pos0, d, w, params=p)
    k = 5
    pos0[k] = [0.0, 0.0, 2.0 * wl.R_E]
    rows, nrows, stop, _ = model.trace(pos0, d, w, params=p)
    assert 1 <= nrows[k] <= int(gold["run_adaptive_params"][5]), "the axis ray has %d rows" % nrows[k]
    others = np.arange(len(w)) != k
    assert np.array_equal(nrows[others], base[1][others]) and np.array_equal(stop[others], base[2][others]), "the axis ray changed its neighbours' fates"
    assert np.array_equal(np.nan_to_num(rows[others]), np.nan_to_num(base[0][others])), "the axis ray changed its neighbours' rows"
    # the density there is what the layered entry point gives for the same point: finite or not, never a fault
    g = model.plasma_params(pos0[k:k + 1])
    assert g.shape == (1, 19), g.shape
    return stop[k]


# ---- builders ------------------------------------------------------------------------------------------------------------
def check_grid_from_handle(model, nx, ny, nz, bounds, compder, nspec, then_trace):
    """srt_build_grid from the handle: ln N at the nodes is the log of the handle's own plasma_params there.  then_trace: the
    model-3 handle made from the same grid traces and reproduces the nodes."""
    B = bounds
    F, D = model.build_grid(nx, ny, nz, B, compder=bool(compder))
    assert F.shape == (nz, ny, nx, nspec), F.shape
    x = np.arange(nx) * ((B[1] - B[0]) / (nx - 1.0)) + B[0]
    y = np.arange(ny) * ((B[3] - B[2]) / (ny - 1.0)) + B[2]
    z = np.arange(nz) * ((B[5] - B[4]) / (nz - 1.0)) + B[4]
    Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
    P = np.stack([X, Y, Z], axis=-1)
    mine = np.log(model.plasma_params(P.reshape(-1, 3))[:, 4:4 + nspec]).reshape(F.shape)
    assert np.all(np.isfinite(F)), "%d nodes are not finite" % (~np.isfinite(F)).sum()
    # device log vs host log of the same densities
    assert np.abs(F - mine).max() <= 2e-14, "ln N at a node is %.3g from the log of the handle's density, bar 2e-14" % np.abs(F - mine).max()
    assert (D is None) == (not compder), "derivative blocks: %s with compder = %s" % (type(D).__name__, compder)
    if compder:
        assert len(D) == 7 and all(np.all(np.isfinite(b)) for b in D), "%d derivative blocks, 7 finite ones wanted" % len(D)
    if not then_trace:
        return
    # the model-3 handle made from it traces
    t = model.to_interp(nx, ny, nz, B, compder=bool(compder))
    assert t.kind == 3, t.kind
    pos, d, w = wl.launch_set(64, 11)
    rows, nrows, stop, steps = t.trace(pos * 0.5, d, w, fixedstep=1, dt0=1e-3, dtmax=0.1, tmax=0.01, maxerr=5e-4, maxsteps=8, del_=1e-6)
    assert steps > 0 and set(np.unique(stop).tolist()) <= {0, 1, 2, 3, 5, 6, 9}, (steps, np.unique(stop))
    at_nodes = t.plasma_params(P.reshape(-1, 3))[:, 4:4 + nspec]
    e = np.abs(np.log(at_nodes) - F.reshape(-1, nspec)).max()
    assert e <= 1e-12 * np.abs(F).max(), "the model-3 handle is %.3g from its nodes, bar %.3g" % (e, 1e-12 * np.abs(F).max())


def check_sample_builder(model):
    """srt_build_samples from the handle: every record's ln N is the log of the handle's own plasma_params at its point."""
    rec, counts = model.build_samples(BOUNDS, n_initial_uniform=200, seed=3)
    assert rec.shape == (200, 7) and counts[2] == 200, (rec.shape, counts)
    want = np.log(model.plasma_params(rec[:, 0:3])[:, 4:8])
    e = np.abs(rec[:, 3:7] - want).max()
    assert e <= 2e-14, "a record's ln N is %.3g from the log of the handle's density, bar 2e-14" % e
