"""modelnum 4: the second-order weight tier of the shared stencil path (srt_scattered.hpp sf_weights, second-order tier) at
its design accuracy, and the stencils it must decline.

The tier expands every sample's weight at the six offset points about the stencil centre.  It is chosen once per stencil when
every sample of the list is at least 1e3 stencil widths from the centre (plus bounds on the window and the local spacing
that the BASELINE sets meet almost everywhere); every other stencil takes round 3's series, where a sample too close for
the series gets its weight directly.  Each stencil below is put into its class by geometry, in numpy, by brute force over
the 5 500 samples of the fixture:
    d_c = max(del |x_c|, del)     the offsets of the six points (fd_step, srt_device.hpp), dmax6 their largest
    rmin                          the distance from the centre to the nearest sample
    "sample"  rmin == 0           a sample AT the centre: the tier must decline (its expansion divides by r + 5e-16 R)
    "series"  rmin <  1e3 dmax6   the series, close samples direct
    "tier"    rmin >= 1e3 dmax6   the tier, wherever its other bounds hold
The search radius (1.5 x the largest nearest-sample distance, 8 089 km here) is larger than every distance used below.

A timing build (-DSRT_PHASE_TIMING, srt_tier_stats) showed that the cases reach the stencils they claim.  A short trace (order 2,
8 steps) from the launch states of test_tier_at_its_design_accuracy took the tier at 15 049 of its 15 080 stencils (99.8 %; the
other 31 declined on the free point of the rkf45 step).  One step from 256 sample positions declined it at all 256, on the
distance test.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR, grad_errors, oracle_grad_sensitivity, oracle_step_sensitivity, vrel, within_sensitivity
from scattered_paths import _own_list

pytestmark = pytest.mark.gpu
DEL = 1.0e-6
TIER_WIDTHS = 1.0e3                 # the tier's distance condition (sf_weights: dmax6 / (rmin + reps) <= 1e-3)
ORACLE_SEED = 2 | 0x80000000        # bit 31: the true nearest-sample distance for the tree root too (what the HIP path stores)
# per-column floors of the gradient comparison (conftest.grad_errors columns: dF/dk, dF/dw, dF/dx, dx/dt, dk/dt)
FLOORS = (1e-8, 1e-7, 3e-6, 1e-7, 3e-6)
# The tier's bars on dF/dx against the oracle.  Its CPU prototype (tools/scattered_taylor_prototype.py) has the central-difference
# gradient of ln N to 3e-8 median and 1.2e-7 p90; on the GPU test_tier_at_its_design_accuracy measured median 2.5e-8 / 5.8e-8
# and p90 1.2e-7 / 4.8e-7 at orders 2 / 3 -- the oracle's own two-ulp yardstick there has median 3.3e-8 / 1.0e-7.  The bars keep
# 3.5x (median) and 2x (p90) above the worse order; today's parity bars (median 1e-5, p90 1e-3) are 50x and 1 000x above them.
TIER_MEDIAN, TIER_P90 = 2e-7, 1e-6


@pytest.fixture(scope="module")
def samples():
    """(sample positions, the model's search radius) -- the radius as the library sets it (srt_scattered_host.cpp): 1.5 x the
    largest distance from a sample outside the Earth to its nearest other sample."""
    from stanford_raytracer_amd import workloads as wl

    pts = np.load(os.path.join(GOLDEN_DIR, "points5500.npz"))["pts"]
    nn = np.array([np.sqrt(np.partition(((pts - p) ** 2).sum(axis=1), 1)[1]) for p in pts])
    outside = np.linalg.norm(pts, axis=1) >= wl.R_E
    return pts, 1.5 * nn[outside].max()


def geometry(pts, x):
    """(dmax6, rmin) per stencil centre x[n, 3]."""
    dmax6 = np.maximum(DEL * np.abs(x), DEL).max(axis=1)
    rmin = np.array([np.sqrt(((pts - p) ** 2).sum(axis=1).min()) for p in x])
    return dmax6, rmin


def stencil_class(samples, x):
    pts, radius = samples
    dmax6, rmin = geometry(pts, x)
    assert np.all(rmin < radius)   # the nearest sample is on the list
    return np.where(rmin == 0.0, "sample", np.where(rmin < TIER_WIDTHS * dmax6, "series", "tier"))


def models(pointsfile, **kw):
    from oracle import oracle
    from stanford_raytracer_amd import api

    return api.Model.scattered_file(pointsfile, **kw), oracle.Model.scattered_file(pointsfile, perm_seed=ORACLE_SEED, **kw)


def with_roots(o, x, seed):
    """States at x with a live root (k along the launch set's directions); drops the points without one."""
    from stanford_raytracer_amd import workloads as wl

    _, d, w = wl.launch_set(len(x), seed)
    od = np.array([o.disp(p, dd, ww) for p, dd, ww in zip(x, d, w)])
    ok = od[:, 8] > 0
    return x[ok], od[ok, 8:9] * d[ok], w[ok]


def sample_centres(pts, lo=1.3, hi=4.0):
    from stanford_raytracer_amd import workloads as wl

    r = np.linalg.norm(pts, axis=1)
    return pts[(r > lo * wl.R_E) & (r < hi * wl.R_E)]


def grad_report(err, yard):
    e = err[:, 2]
    return "dF/dx vs oracle: median %.3g p90 %.3g max %.3g (yard median %.3g max %.3g); dF/dk max %.3g; dF/dw max %.3g; dk/dt max %.3g" % (
        np.median(e), np.percentile(e, 90), e.max(), np.median(yard[:, 2]), yard[:, 2].max(), err[:, 0].max(), err[:, 1].max(),
        err[:, 4].max())


def assert_within_oracle(a, o, x, k, w, tag, outliers=0.01):
    """Every output column of the gradients within 10 x max(the oracle's own two-ulp sensitivity, FLOORS) (1 % outliers);
    returns (dF/dx errors, yardstick, report)."""
    _, yard = oracle_grad_sensitivity(o, x, k, w, DEL)
    og = np.array([o.grad(p, kk, ww, DEL) for p, kk, ww in zip(x, k, w)])
    err = grad_errors(a, og)
    msg = "%s: %d stencils; %s" % (tag, len(x), grad_report(err, yard))
    print(msg)
    for col, name in enumerate(("dFdk", "dFdw", "dFdx", "dx/dt", "dk/dt")):
        ok, txt = within_sensitivity(err[:, col], yard[:, col], FLOORS[col], outliers=outliers)
        assert ok, "%s: %s -- %s" % (name, txt, msg)
    return err[:, 2], yard[:, 2], msg


# ---- a sample AT the stencil centre --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(order=0), dict(order=1), dict(order=2), dict(order=3), dict(order=4),
                                dict(exact=1, local_window_scale=2.0)],
                         ids=["order0", "order1", "order2", "order3", "order4", "exact"])
def test_gradients_at_sample_positions(samples, pointsfile, kw):
    """Stencil centres exactly on samples.  Orders 0-3 go through the cooperative stencil (sf_weights<J>), where such a
    stencil must decline the tier: pass 1's smallest distance is 0 there.  Order 4 (gen_stencil) and the exact window (no
    tier) are controls.  Against the oracle within its own sensitivity, and against the own-list path (exact weights per
    point and sample)."""
    pts, _ = samples
    g, o = models(pointsfile, **kw)
    x, k, w = with_roots(o, sample_centres(pts)[:120], 6060)
    x, k, w = x[:60], k[:60], w[:60]
    assert len(x) >= 40
    assert np.all(stencil_class(samples, x) == "sample")
    a = g.gradients(x, k, w, DEL)
    b = _own_list(lambda: g.gradients(x, k, w, DEL))
    assert np.isfinite(a).all(), "non-finite gradients at %d of %d sample positions" % ((~np.isfinite(a).all(axis=1)).sum(), len(a))
    assert np.isfinite(b).all()
    # (order 4's 35-term fit at a sample is ill-conditioned in the oracle itself: the GPU's p90 is 0.3 and its two-ulp yardstick
    # reaches 1.9.  Seven stencils differ by more than 1e-3, and the oracle moves by 0.5 or more at each of them once its
    # yardstick takes draws up to 1e-13; one of them escapes the two-ulp draws.  Order 4 keeps the median bar, with 3 % outliers.)
    gen = kw.get("order") == 4
    e, _, msg = assert_within_oracle(a, o, x, k, w, "at samples %s" % kw, outliers=0.03 if gen else 0.01)
    assert np.median(e) <= TIER_MEDIAN, msg
    assert gen or np.percentile(e, 90) <= TIER_P90, msg
    assert vrel(a[:, 0:3], b[:, 0:3]).max() <= 1e-9
    eb = vrel(a[:, 4:7], b[:, 4:7])
    assert np.median(eb) <= TIER_MEDIAN and np.percentile(eb, 90) <= TIER_P90, (np.median(eb), np.percentile(eb, 90), eb.max())


def test_rk_step_from_sample_positions(samples, gpu_models, oracle_scattered):
    """One RK step (rk4, rkf45 4th / 5th order) from states at sample positions: the first right-hand side is a stencil about
    a sample.  Every output within 10 x max(the oracle's own sensitivity, a floor), and the median error within 3 x the oracle's
    median sensitivity.  The later stages land 10-150 km from the sample, where the oracle itself is chaotic (the rkf45
    outputs' k moves by 7e-5 median under a few-ulp shift of the state): the yardstick takes 16 draws, and 5 % of the states
    may miss it (measured: 3 of 80, each within the largest yardstick of the set)."""
    pts, _ = samples
    g, o = gpu_models["scattered"], oracle_scattered
    x, k, w = with_roots(o, sample_centres(pts)[:200], 7070)
    x, k, w = x[:80], k[:80], w[:80]
    assert len(x) >= 40
    assert np.all(stencil_class(samples, x) == "sample")
    args = np.concatenate([x, k, w[:, None]], axis=1)
    dt = np.full(len(args), 1e-3)
    out = g.rk_step(args, dt, DEL)
    assert np.isfinite(out).all()
    _, syard = oracle_step_sensitivity(o, args, dt, DEL, eps=(4.0e-16, 1.5e-15, 6.0e-15, 2.4e-14))
    ref = np.array([o.step(a, d, DEL) for a, d in zip(args, dt)])
    for i, c in enumerate((0, 7, 14)):
        ex, ek = vrel(out[:, c:c + 3], ref[:, c:c + 3]), vrel(out[:, c + 3:c + 6], ref[:, c + 3:c + 6])
        msg = "step output %d: position median %.3g max %.3g (yard max %.3g); k median %.3g max %.3g (yard max %.3g)" % (
            c, np.median(ex), ex.max(), syard[:, i, 0].max(), np.median(ek), ek.max(), syard[:, i, 1].max())
        print(msg)
        for err, yard, floor, name in ((ex, syard[:, i, 0], 1e-12, "position"), (ek, syard[:, i, 1], 1e-9, "k")):
            ok, txt = within_sensitivity(err, yard, floor, outliers=0.05)
            assert ok, "%s: %s -- %s" % (name, txt, msg)
            assert np.median(err) <= 3.0 * max(np.median(yard), floor), "%s: median -- %s" % (name, msg)
        assert np.array_equal(out[:, c + 6], ref[:, c + 6])


def test_rays_launched_at_sample_positions(samples, gpu_models, oracle_scattered):
    """Short adaptive rays launched at sample positions against the oracle: row 0 the same launch; row 1 (the first accepted
    step, at dt0 under first-attempt policy 0) no further from the oracle's than the oracle moves when the launch points shift
    by 1e-9 relative, on 90 % of the rays and by a median factor of ten; stop codes agree at least as well as the oracle agrees
    with itself under that shift."""
    from stanford_raytracer_amd import workloads as wl

    pts, _ = samples
    g, o = gpu_models["scattered"], oracle_scattered
    x = sample_centres(pts)[:256]
    assert np.all(stencil_class(samples, x) == "sample")
    _, d, w = wl.launch_set(len(x), 8080)
    kw = dict(fixedstep=0, dt0=1e-3, dtmax=0.1, tmax=0.01, maxerr=5e-4, maxsteps=60, del_=DEL)
    rows, nrows, stop, _ = g.trace(x, d, w, outputper=1, **kw)
    orows, onrows, ostop, _ = o.trace(x, d, w, capacity=60, **kw)
    both = (nrows > 1) & (onrows > 1)
    assert both.sum() >= 64
    assert np.array_equal(rows[both, 0, 0:4], orows[both, 0, 0:4])                       # launch time and position
    assert vrel(rows[both, 0, 10:13], orows[both, 0, 10:13]).max() <= 1e-9             # launch refractive index
    assert (np.abs(rows[both, 0, 16:20] - orows[both, 0, 16:20]) / orows[both, 0, 16:20]).max() <= 1e-9   # densities
    assert np.all(rows[both, 1, 0] == orows[both, 1, 0])
    yard_p, yard_n, yard_stop = np.zeros(both.sum()), np.zeros(both.sum()), 1.0
    for eps in (1e-9, -1e-9):
        prow, pn, pstop, _ = o.trace(x * (1.0 + eps), d, w, capacity=60, **kw)
        assert np.all(pn[both] > 1)
        yard_p = np.maximum(yard_p, vrel(prow[both, 1, 1:4], orows[both, 1, 1:4]))
        yard_n = np.maximum(yard_n, vrel(prow[both, 1, 10:13], orows[both, 1, 10:13]))
        yard_stop = min(yard_stop, float(np.mean(pstop == ostop)))
    ep, en = vrel(rows[both, 1, 1:4], orows[both, 1, 1:4]), vrel(rows[both, 1, 10:13], orows[both, 1, 10:13])
    qp, qn = ep / yard_p, en / yard_n    # per ray: the GPU's distance from the oracle in units of the oracle's own shift
    msg = ("row 1 (%d rays): position err median %.3g max %.3g, err / yard median %.3g p95 %.3g, over the yard %.3f; "
           "n err median %.3g max %.3g, err / yard median %.3g p95 %.3g, over the yard %.3f; stop agree %.4f (oracle' %.4f)" % (
               both.sum(), np.median(ep), ep.max(), np.median(qp), np.percentile(qp, 95), np.mean(qp > 1), np.median(en), en.max(),
               np.median(qn), np.percentile(qn, 95), np.mean(qn > 1), np.mean(stop == ostop), yard_stop))
    print(msg)
    # The first step's later stages land 10-150 km from the sample, where the oracle itself is chaotic (see the step test above):
    # a few rays may sit beyond the yardstick of two draws; the bulk sits far inside it.  Measured: err / yard median 0.003
    # (position) and 0.035 (n), 0.9 % and 4.7 % of the rays over it; the unfixed tier gave medians 1.7 and 1.3, 62 % and 56 % over.
    for q in (qp, qn):
        assert np.median(q) <= 0.1 and np.mean(q > 1.0) <= 0.1, msg
    n = len(x)
    assert np.mean(stop == ostop) >= yard_stop - 3.0 * np.sqrt(max(yard_stop * (1 - yard_stop), 1e-4) / n), msg


# ---- an offset point exactly on a sample (control: the series' direct weights) ------------------------------------------
def test_offset_point_exactly_on_a_sample(samples, gpu_models, oracle_scattered):
    """Centres chosen so that x_a + d_a (or x_a - d_a) is a sample's coordinate bit for bit, the other two coordinates the
    sample's: one of the six offset points sits on the sample.  The centre is then d_a from it (a "series" stencil), and the
    sample's weight at that point is evaluated directly."""
    pts, _ = samples
    g, o = gpu_models["scattered"], oracle_scattered
    s = sample_centres(pts)[300:420]
    x, hit = s.copy(), np.zeros(len(s), bool)
    for i in range(len(x)):
        a, sign = i % 3, (1.0 if (i // 3) % 2 == 0 else -1.0)   # point 1 + 2a (x + d) or 2 + 2a (x - d) on the sample
        c = s[i, a] / (1.0 + sign * DEL * np.sign(s[i, a]))      # x + sign del |x| = s_a, then the neighbouring doubles
        for _ in range(16):
            y = c + sign * max(DEL * abs(c), DEL)
            if y == s[i, a]:
                x[i, a], hit[i] = c, True
                break
            c = np.nextafter(c, np.inf if y < s[i, a] else -np.inf)
    x = x[hit]     # (where no double lands exactly on the sample's coordinate, the sample is left out)
    assert len(x) >= 80
    assert np.all(stencil_class(samples, x) == "series")
    x, k, w = with_roots(o, x, 9090)
    assert len(x) >= 40
    a = g.gradients(x, k, w, DEL)
    b = _own_list(lambda: g.gradients(x, k, w, DEL))
    assert np.isfinite(a).all() and np.isfinite(b).all()
    e, _, msg = assert_within_oracle(a, o, x, k, w, "offset point on a sample")
    assert np.median(e) <= TIER_MEDIAN and np.percentile(e, 90) <= TIER_P90, msg
    assert vrel(a[:, 0:3], b[:, 0:3]).max() <= 1e-9


# ---- both sides of the tier's distance condition ------------------------------------------------------------------------
def test_both_sides_of_the_tier_boundary(samples, gpu_models, oracle_scattered):
    """The nearest sample at 0.5, 0.9, 1.1 and 2 x 1e3 dmax6 from the centre (the centre moved from the sample along a random
    direction): the two smaller distances are series stencils, the two larger ones tier stencils.  Each side holds the
    tier's bars, and the error does not jump across the boundary."""
    pts, _ = samples
    g, o = gpu_models["scattered"], oracle_scattered
    s = sample_centres(pts)[500:620]
    u = np.random.default_rng(11).normal(size=s.shape)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    med = {}
    for f in (0.5, 0.9, 1.1, 2.0):
        x = s.copy()
        for _ in range(3):   # dmax6 depends on the centre
            x = s - f * TIER_WIDTHS * np.maximum(DEL * np.abs(x), DEL).max(axis=1, keepdims=True) * u
        dmax6, rmin = geometry(pts, x)
        assert np.allclose(rmin / (TIER_WIDTHS * dmax6), f, rtol=1e-6)   # the moved-from sample is the nearest one
        assert np.all(stencil_class(samples, x) == ("series" if f < 1.0 else "tier"))
        xs, k, w = with_roots(o, x, 1111)
        assert len(xs) >= 40
        a = g.gradients(xs, k, w, DEL)
        assert np.isfinite(a).all()
        e, _, msg = assert_within_oracle(a, o, xs, k, w, "nearest sample at %.1f x 1e3 dmax6" % f)
        assert np.median(e) <= TIER_MEDIAN and np.percentile(e, 90) <= TIER_P90, msg
        med[f] = float(np.median(e))
    assert max(med[0.9], med[1.1]) <= 5.0 * min(med[0.9], med[1.1]), med


# ---- the tier at its design accuracy ----------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [2, 3])
def test_tier_at_its_design_accuracy(samples, pointsfile, order):
    """Launch states of the parity tests' kind (the launch set at 0.9 of its radius), every one a tier stencil by geometry:
    dF/dx against the oracle at the tier's own accuracy (TIER_MEDIAN, TIER_P90; every stencil within 10 x max(its two-ulp
    yardstick, 3e-6), 1 % outliers), far inside today's parity bars."""
    from stanford_raytracer_amd import workloads as wl

    pts, _ = samples
    g, o = models(pointsfile, order=order)
    pos, _, _ = wl.launch_set(400, 2468)
    x, k, w = with_roots(o, pos * 0.9, 1357)
    x, k, w = x[:300], k[:300], w[:300]
    assert len(x) >= 200
    assert np.all(stencil_class(samples, x) == "tier")
    a = g.gradients(x, k, w, DEL)
    assert np.isfinite(a).all()
    e, _, msg = assert_within_oracle(a, o, x, k, w, "tier stencils, order %d" % order)
    assert np.median(e) <= TIER_MEDIAN, msg
    assert np.percentile(e, 90) <= TIER_P90, msg
