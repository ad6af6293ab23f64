"""GPU (-m gpu): whole trajectories (raytracer_run batched) against the oracle / golden vectors, edge cases,
and size-independent properties at BASELINE.json's full sizes.

Trajectories are chaotic at rounding level: the reference diverges from its own FMA rebuild by 1.2e-10 /
7e-8 / 4e-5 in position after 1 / 10 / 100 fixed steps and changes adaptive step sequences within 2-22 steps
(SURVEY A-9).  The bar used here: the GPU's divergence from the oracle must not exceed 10x the oracle's
own divergence under a 1e-9 relative shift of the launch point (~1 cm), with the survey ladder x10 as floor.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import DELS, vrel
from model_ladder import LADDER, curve_distance, divergence, oracle_yardstick
from stanford_raytracer_amd import workloads as wl

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,tag,rows_at", [("ngo", "g4_ngo_fixed", (1, 10, 100)), ("interp", "g4_interp_fixed", (1, 10, 50))])
def test_fixed_step_trajectories(golden, gpu_models, oracle_models, name, tag, rows_at):
    """BASELINE config[0] shape: 16 rays, fixed RK4.  Compared with the reference's golden rows."""
    rays, prm = golden["g4_rays"], golden[tag + "_params"]
    ref_rows, ref_n, ref_stop = golden[tag + "_rows"], golden[tag + "_nrows"], golden[tag + "_stop"]
    kw = dict(dt0=prm[0], dtmax=prm[1], tmax=prm[2], maxerr=prm[3], minalt=prm[4], maxsteps=int(prm[5]),
              root=int(prm[6]), fixedstep=1, del_=DELS[name])
    cap = int(ref_rows.shape[1])
    rows, nrows, stop, steps = gpu_models[name].trace(rays[:, :3], rays[:, 3:6], rays[:, 6], outputper=1,
                                                      **dict(kw, maxsteps=cap + 1))
    assert np.array_equal(nrows, ref_n) and np.array_equal(stop, ref_stop)
    assert steps == int((ref_n - 1).sum())
    # row 0 is a pure function of the inputs
    assert np.array_equal(rows[:, 0, 0:4], ref_rows[:, 0, 0:4])
    assert vrel(rows[:, 0, 13:16], ref_rows[:, 0, 13:16]).max() <= 2e-7
    assert vrel(rows[:, 0, 10:13], ref_rows[:, 0, 10:13]).max() <= 1e-10
    assert vrel(rows[:, 0, 7:10], ref_rows[:, 0, 7:10]).max() <= 1e-6   # vgrel: pure finite differences
    _, yard = oracle_yardstick(oracle_models[name], rays, dict(kw, maxsteps=cap + 1), rows_at, cap)
    for r in rows_at:
        d = divergence(rows, nrows, ref_rows, ref_n, r, slice(1, 4))
        bound = 10 * max(yard[r], LADDER.get(r, 4e-5))
        assert d <= bound, "row %d: position divergence %.2e > %.2e" % (r, d, bound)
        assert np.allclose(rows[:, r, 0], ref_rows[:, r, 0], rtol=1e-12)  # same time grid


@pytest.mark.parametrize("name,tag", [("ngo", "g4_ngo_adaptive"), ("ngoducts", "g4_ngoducts_adaptive"),
                                      ("interp", "g4_interp_adaptive"), ("ngo", "g4_ngo_launch"),
                                      ("interp", "g4_interp_launch")])
def test_adaptive_trajectories(golden, gpu_models, oracle_models, name, tag):
    """The reference's own adaptive rows (goldens) for the 16 Appendix-B rays and the launch-set rays.  Bars: the oracle
    (bit-identical to the reference on these runs) against itself under a 1e-9 shift of the launch points, as in
    test_fixed_step_trajectories; the statistics on 1 000+ rays are in tests/test_gpu_trajectory_stats.py."""
    rays = golden["g4_launch_rays" if tag.endswith("launch") else "g4_rays"]
    prm = golden[tag + "_params"]
    ref_rows, ref_n, ref_stop = golden[tag + "_rows"], golden[tag + "_nrows"], golden[tag + "_stop"]
    kw = dict(dt0=prm[0], dtmax=prm[1], tmax=prm[2], maxerr=prm[3], minalt=prm[4], maxsteps=int(prm[5]), root=int(prm[6]),
              fixedstep=0, del_=DELS[name])
    rows, nrows, stop, _ = gpu_models[name].trace(rays[:, :3], rays[:, 3:6], rays[:, 6], outputper=1, **kw)
    om = oracle_models[name]
    cap = int(ref_rows.shape[1])
    base = om.trace(rays[:, :3], rays[:, 3:6], rays[:, 6], capacity=cap, **kw)
    assert np.array_equal(base[1], ref_n) and np.array_equal(base[2], ref_stop)     # the oracle IS the reference here
    yard_curve, yard_stop, yard_rows = 0.0, 1.0, 0
    for eps in (1e-9, -1e-9):
        pert = om.trace(rays[:, :3] * (1 + eps), rays[:, 3:6], rays[:, 6], capacity=cap, **kw)
        yard_curve = max(yard_curve, curve_distance(pert[0], pert[1], base[0], base[1], 0.1))
        yard_stop = min(yard_stop, float(np.mean(pert[2] == base[2])))
        yard_rows = max(yard_rows, abs(int(pert[1].sum()) - int(base[1].sum())))
    assert np.mean(stop == ref_stop) >= min(0.9, yard_stop - 1.0 / len(stop))
    # first attempt: always accepted at dt0 and never grown (SURVEY A-1, flang semantics); the second
    # step therefore ends at 2 dt0 at the latest
    both = (nrows > 2) & (ref_n > 2)
    assert np.allclose(rows[both, 1, 0], prm[0]) and np.all(rows[both, 2, 0] <= 2 * prm[0] * (1 + 1e-12))
    assert abs(int(nrows.sum()) - int(ref_n.sum())) <= max(3 * yard_rows, 0.05 * ref_n.sum())
    # curves: position on a common time grid over the early part of the run; no worse than 3x the oracle against itself
    # (floor: SURVEY A-9's 1e-3)
    assert curve_distance(rows, nrows, ref_rows, ref_n, 0.1) <= max(3 * yard_curve, 1e-3)


def test_field_aligned_launch(golden, gpu_models):
    """dir0 = 0 -> start along B with the radial component made positive (raytracer.f95:661-674)."""
    rays, prm = golden["g4_fa_rays"], golden["g4_ngo_fieldaligned_params"]
    ref_rows, ref_n = golden["g4_ngo_fieldaligned_rows"], golden["g4_ngo_fieldaligned_nrows"]
    rows, nrows, stop, _ = gpu_models["ngo"].trace(rays[:, :3], rays[:, 3:6], rays[:, 6], outputper=1, dt0=prm[0],
                                                   dtmax=prm[1], tmax=prm[2], maxerr=prm[3], minalt=prm[4],
                                                   maxsteps=int(prm[5]), root=2, fixedstep=0, del_=1e-4)
    assert vrel(rows[:, 0, 10:13], ref_rows[:, 0, 10:13]).max() <= 1e-9   # n0 = k0 c / w along B
    assert curve_distance(rows, nrows, ref_rows, ref_n, 0.05) <= 1e-3


def test_edge_cases(gpu_models):
    from stanford_raytracer_amd import api

    m = gpu_models["ngo"]
    pos, d, w = wl.launch_set(65, 31)
    kw = dict(fixedstep=0, dt0=1e-3, dtmax=0.1, maxerr=5e-4, tmax=0.02, del_=1e-4)
    # empty batch
    rows, nrows, stop, steps = m.trace(pos[:0], d[:0], w[:0], maxsteps=8, **kw)
    assert rows.shape[0] == 0 and steps == 0
    # maxsteps = 1: only row 0, stop code 6 unless an earlier test fires
    rows, nrows, stop, steps = m.trace(pos, d, w, maxsteps=1, **kw)
    assert np.all(nrows == 1) and steps == 0 and set(stop.tolist()) <= {1, 2, 6}
    assert np.array_equal(rows[:, 0, 1:4], pos)
    # tmax = 0: normal exit before any step
    rows, nrows, stop, _ = m.trace(pos, d, w, maxsteps=8, **dict(kw, tmax=0.0))
    assert np.all(nrows == 1) and np.all(stop == 0)
    # launch below minalt -> stop 1 on the first test
    low = pos.copy()
    low *= (wl.R_E + 50e3) / np.linalg.norm(low, axis=1, keepdims=True)
    _, nrows, stop, _ = m.trace(low, d, w, maxsteps=8, **kw)
    assert np.all(stop == 1) and np.all(nrows == 1)
    # outputper larger than the trajectory: one kept row
    rows, nrows, stop, _ = m.trace(pos, d, w, maxsteps=16, outputper=64, **kw)
    assert rows.shape[1] == 1
    # bad arguments are rejected, not run
    for bad in (dict(maxsteps=0), dict(root=3), dict(del_=0.0)):
        with pytest.raises(api.SrtError):
            m.trace(pos, d, w, **dict(dict(kw, maxsteps=8), **bad))


def test_evanescent_starts_stop_at_once(gpu_models, oracle_models):
    """Rays whose chosen root is evanescent at the launch point get k0 = Re(k) = 0 and stop with code 2 on
    the first test (raytracer.f95:690, :334); which rays those are is decided before any FD noise enters."""
    pos, d, w = wl.launch_set(2000, 77)
    kw = dict(fixedstep=0, dt0=1e-3, dtmax=0.1, maxerr=5e-4, tmax=0.004, maxsteps=6, del_=1e-4)
    _, nrows, stop, _ = gpu_models["ngo"].trace(pos, d, w, **kw)
    _, on, ostop, _ = oracle_models["ngo"].trace(pos, d, w, capacity=0, **kw)
    assert (ostop == 2).sum() > 20
    assert np.array_equal(stop == 2, ostop == 2)
    assert np.all(nrows[stop == 2] == 1)
    assert np.mean(stop == ostop) > 0.98


def test_interp_rays_outside_the_grid(gpu_models, oracle_models):
    """Rays launched beyond the grid bounds run on the clamped edge cells like the reference's."""
    g, o = gpu_models["interp"], oracle_models["interp"]
    pos, d, w = wl.launch_set(48, 55)
    pos = pos * (5.3 * wl.R_E / np.abs(pos).max(axis=1, keepdims=True))  # one coordinate beyond +-5 R_E
    kw = dict(fixedstep=1, dt0=1e-3, tmax=0.003, maxsteps=8, del_=1e-6)
    rows, nrows, stop, _ = g.trace(pos, d, w, **kw)
    orows, on, ostop, _ = o.trace(pos, d, w, capacity=8, **kw)
    assert np.array_equal(stop, ostop) and np.array_equal(nrows, on)
    sel = nrows > 1
    assert vrel(rows[sel, 1, 1:4], orows[sel, 1, 1:4]).max() <= 1e-7
    assert np.max(np.abs(rows[:, 0, 16:20] - orows[:, 0, 16:20]) / orows[:, 0, 16:20]) <= 1e-11


@pytest.mark.parametrize("name", ["ngo", "interp", "scattered"])
def test_determinism_and_lane_independence(gpu_models, name):
    """A ray's result must not depend on which lane/wave integrates it, nor on the refill policy.  (Scattered model: the
    staging records, the LDS-DMA record ring and the list compaction are shared by the wave -- a missed wait would show
    up here as a run-to-run difference.)"""
    m = gpu_models[name]
    pos, d, w = wl.launch_set(3000, 91)
    if name == "scattered":
        pos = pos * 0.9
    kw = dict(fixedstep=0, dt0=1e-3, dtmax=0.1, maxerr=5e-4, tmax=0.05, maxsteps=40, outputper=8, del_=DELS[name])
    a = m.trace(pos, d, w, **kw)
    b = m.trace(pos, d, w, **kw)
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]
    perm = np.random.default_rng(1).permutation(len(w))
    c = m.trace(pos[perm], d[perm], w[perm], **kw)
    assert np.array_equal(c[0], a[0][perm]) and np.array_equal(c[1], a[1][perm]) and np.array_equal(c[2], a[2][perm])
    e = m.trace(pos, d, w, refill_threshold=48, **kw)
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], e[:3]))


def check_invariants(pos, rows, nrows, stop, steps, p):
    slots = rows.shape[1]
    assert steps == int(nrows.astype(np.int64).sum() - len(nrows))
    assert nrows.min() >= 1 and nrows.max() <= p.maxsteps
    assert set(np.unique(stop).tolist()) <= {0, 1, 2, 3, 5, 6, 9}
    assert np.mean(stop == 9) < 0.01
    assert np.all(nrows[stop == 6] == p.maxsteps)
    assert np.array_equal(rows[:, 0, 1:4], pos) and np.all(rows[:, 0, 0] == 0)
    kept = np.minimum((nrows + p.outputper - 1) // p.outputper, slots)
    for s in range(1, slots):
        live = kept > s
        if live.any():
            assert np.all(rows[live, s, 0] > rows[live, s - 1, 0])  # time strictly increases
            assert np.all(np.isfinite(rows[live, s, 1:4]))          # non-finite states end with code 9 at once
    done = (stop == 0) & (kept >= 1)
    return done


def test_ray_order_option_changes_only_the_schedule(gpu_models):
    """srt_params.ray_order = 1 works through the launch set sorted by launch cell; every ray's rows, row count and
    stop code are bit-identical and stay at the ray's own index."""
    m = gpu_models["interp"]
    pos, d, w = wl.launch_set(5000, 31)
    kw = dict(fixedstep=0, dt0=1e-3, dtmax=0.1, tmax=0.3, maxerr=5e-4, maxsteps=64, del_=1e-6, outputper=4)
    a = m.trace(pos, d, w, **kw)
    for order in (1, 2):  # 2: the two-class order (likely-short rays last, an experiment switch)
        b = m.trace(pos, d, w, ray_order=order, **kw)
        for x, y in zip(a[:3], b[:3]):
            assert np.array_equal(x, y)
        assert a[3] == b[3]


def test_full_size_config2_ngo_100k(cfgfiles):
    """BASELINE config[1]: 100k rays, Ngo, adaptive RK45 -- size-independent properties."""
    from stanford_raytracer_amd import api

    m = api.Model.ngo(cfgfiles["ngo"])
    pos, d, w = wl.launch_set(100_000, 2)
    p = api.make_params(fixedstep=0, dt0=1e-3, dtmax=0.1, maxerr=5e-4, tmax=0.5, maxsteps=512, outputper=8, del_=1e-4,
                        minalt=wl.MINALT)
    rows, nrows, stop, steps = m.trace(pos, d, w, params=p)
    check_invariants(pos, rows, nrows, stop, steps, p)
    assert steps > 1_000_000
    # a shuffled subset reproduces the same rays bit for bit (lane independence at scale)
    idx = np.random.default_rng(5).choice(len(w), 4096, replace=False)
    r2, n2, s2, _ = m.trace(pos[idx], d[idx], w[idx], params=p)
    assert np.array_equal(r2, rows[idx]) and np.array_equal(n2, nrows[idx]) and np.array_equal(s2, stop[idx])


@pytest.fixture(scope="module")
def interp256_model():
    from stanford_raytracer_amd import api

    F, b = wl.make_grid(256, half_width=10.0 * wl.R_E)
    m = api.Model.interp(F, b, wl.QS, wl.MS)
    del F
    yield m
    m.close()


def test_full_size_config3_interp256_1m(interp256_model):
    """BASELINE config[2]: 1M rays on the 256^3 grid (34.8 GB coefficient table) -- properties only."""
    from stanford_raytracer_amd import api

    m = interp256_model
    assert m.device_bytes == 257 ** 3 * 4 * 64 * 8
    pos, d, w = wl.launch_set(1_000_000, 3)
    # (the benchmarked configuration: bench.py WORKLOADS["interp256"] -- outputper 16, launch-cell order)
    p = api.make_params(fixedstep=0, dt0=1e-3, dtmax=0.1, maxerr=5e-4, tmax=0.5, maxsteps=256, outputper=16, del_=1e-6,
                        minalt=wl.MINALT, ray_order=1)
    rows, nrows, stop, steps = m.trace(pos, d, w, params=p)
    check_invariants(pos, rows, nrows, stop, steps, p)
    assert steps > 100_000_000
    idx = np.random.default_rng(6).choice(len(w), 8192, replace=False)
    r2, n2, s2, _ = m.trace(pos[idx], d[idx], w[idx], params=p)
    assert np.array_equal(r2, rows[idx]) and np.array_equal(n2, nrows[idx]) and np.array_equal(s2, stop[idx])


@pytest.fixture(scope="module")
def oracle256():
    from oracle import oracle

    F, b = wl.make_grid(256, half_width=10.0 * wl.R_E)
    om = oracle.Model.interp(F, b, wl.QS, wl.MS)  # 8 arrays of 67 M doubles (4.3 GB), 15 s
    del F
    return om


def points_256():
    """Where the 256^3 table is probed: the launch region, the HIGHEST-index cells (cell number 256 of 0..256 on every axis:
    the far end of 34.8 GB of addressing), all six clamped faces (a point below / above the grid on one axis, inside on
    the others), edges and corners outside the grid on two / three axes, and exact node hits."""
    rng = np.random.default_rng(256)
    hw = 10.0 * wl.R_E
    h = 2.0 * hw / 255.0
    pts = [wl.launch_set(500, 256)[0]]
    pts.append(rng.uniform(-hw, hw, (200, 3)))
    pts.append(hw - h * rng.uniform(0.0, 1.0, (100, 3)))           # cell (254, 254, 254): the last interior cell
    pts.append(hw - h * rng.uniform(0.0, 2.0, (60, 3)))
    for ax in range(3):                                             # the six faces
        for sign in (-1.0, 1.0):
            q = rng.uniform(-hw, hw, (40, 3))
            q[:, ax] = sign * (hw + rng.uniform(1.0, 3.0e6, 40))
            pts.append(q)
    q = rng.uniform(-hw, hw, (60, 3))                               # edges and corners
    out = rng.integers(0, 2, (60, 3)).astype(bool)
    out[:, 0] |= ~out.any(axis=1)
    q[out] = (np.sign(q) * (hw + rng.uniform(1.0, 2.0e6, (60, 3))))[out]
    pts.append(q)
    nodes = (rng.integers(0, 256, (40, 3)) * ((2.0 * hw) / 255.0)) + (-hw)  # exact nodes (the adapter's own expression)
    pts.append(nodes)
    pts.append(np.array([[hw, hw, hw], [-hw, -hw, -hw], [hw, -hw, hw]]))
    pts = np.concatenate(pts)
    return pts[np.linalg.norm(pts, axis=1) > wl.R_E + 200e3]


def test_value_parity_on_the_256_grid(interp256_model, oracle256):
    """G0 and G2 by VALUE on the table the headline runs on (the oracle's 256^3 model is built from the same grid): densities
    at >= 1000 points incl. the highest-index cells and the clamped faces, then gradients / the right-hand side where a
    whistler-mode root exists.  Bars: those of the 16^3 tests (test_gpu_parity.py)."""
    from oracle import oracle

    g, o = interp256_model, oracle256
    pts = points_256()
    assert len(pts) >= 1000
    gp = g.plasma_params(pts)
    op = np.array([np.concatenate(o.plasma_params(p)) for p in pts])
    rel = lambda a, b: np.abs(a - b) / np.maximum(np.abs(b), 1e-300)
    assert rel(gp[:, 4:8], op[:, 4:8]).max() <= 1e-11
    assert vrel(gp[:, 16:19], op[:, 16:19]).max() <= 2e-7
    # the far corner cell really is the far end of the table
    hw = 10.0 * wl.R_E
    assert np.sum(np.all(pts > hw - 2.0 * hw / 255.0, axis=1) & np.all(pts < hw, axis=1)) >= 50
    # G2: a wave normal on root 2 at every point that has one
    rng = np.random.default_rng(257)
    kd = rng.normal(size=pts.shape)
    kd /= np.linalg.norm(kd, axis=1, keepdims=True)
    w = 2.0 * np.pi * np.exp(rng.uniform(np.log(0.5e3), np.log(10e3), len(pts)))
    kmag = np.array([o.disp(p, d, ww)[8] for p, d, ww in zip(pts, kd, w)])
    ok = np.isfinite(kmag) & (kmag > 0)
    assert ok.sum() >= 500
    x, k, w = pts[ok], kd[ok] * kmag[ok, None], w[ok]
    gg = g.gradients(x, k, w, 1e-6)
    og = np.array([o.grad(a, b, c, 1e-6) for a, b, c in zip(x, k, w)])
    # Bars per sample: 10 x the larger of a floor and the ORACLE's own change under a two-ulp shift of the state
    # (conftest.oracle_grad_sensitivity).  This point set reaches the outermost cells of the table (10 R_E, N_e four decades below
    # the launch region's), where dF/dk, dF/dw -- central differences with a 1e-8 RELATIVE step -- amplify one ulp of F by
    # 2^-53 / 1e-8 times F's cancellation (first GPU run: dF/dw worst 2.2e-4, 99 % under 4e-5).  The well-conditioned states keep
    # the 16^3 bars as they are.
    from conftest import grad_errors, oracle_grad_sensitivity, within_sensitivity

    _, yard = oracle_grad_sensitivity(o, x, k, w, 1e-6)
    err = grad_errors(gg, og)
    well = np.all(yard <= 1e-7, axis=1)
    msg = "well-conditioned %d of %d: dFdk max %.3g; dFdw max %.3g; dFdx median %.3g p95 %.3g; dx/dt max %.3g; dk/dt median %.3g p95 %.3g" % (
        well.sum(), len(well), err[well, 0].max(), err[well, 1].max(), np.median(err[well, 2]), np.percentile(err[well, 2], 95),
        err[well, 3].max(), np.median(err[well, 4]), np.percentile(err[well, 4], 95))
    print(msg)
    assert well.sum() >= 300, msg
    assert err[well, 0].max() <= 1e-7 and err[well, 1].max() <= 1e-6, msg
    assert np.median(err[well, 2]) <= 1e-7 and np.percentile(err[well, 2], 95) <= 1e-5, msg
    assert err[well, 3].max() <= 1e-6, msg
    assert np.median(err[well, 4]) <= 1e-6 and np.percentile(err[well, 4], 95) <= 2e-5, msg
    for col, (name, floor) in enumerate((("dFdk", 1e-8), ("dFdw", 1e-7), ("dFdx", 1e-6), ("dx/dt", 1e-7), ("dk/dt", 2e-6))):
        fin = np.isfinite(yard[:, col]) & np.isfinite(err[:, col])
        ok, txt = within_sensitivity(err[fin, col], yard[fin, col], floor)
        assert ok, "%s: %s" % (name, txt)


def test_full_size_config4_interp_4m_shards(interp256_model):
    """BASELINE config[3]: 4M rays (seed 4) on the 256^3 grid.  All 4M in one launch: properties; then the shard a rank of an
    8-GPU run would get (parallel.shard_bounds(4M, 5, 8)) traced on its own, with the Morton-ordered schedule: bit-identical
    to the same rays' results in the whole-set launch -- what makes the sharded run equal to the single-GPU one."""
    from stanford_raytracer_amd import api, parallel

    m = interp256_model
    pos, d, w = wl.launch_set(4_000_000, 4)
    p = api.make_params(fixedstep=0, dt0=1e-3, dtmax=0.1, maxerr=5e-4, tmax=0.5, maxsteps=256, outputper=16, del_=1e-6,
                        minalt=wl.MINALT, ray_order=1)  # (bench.py WORKLOADS["interp4m"]; 10.9 GB of rows)
    rows, nrows, stop, steps = m.trace(pos, d, w, params=p)
    check_invariants(pos, rows, nrows, stop, steps, p)
    assert steps > 500_000_000
    lo, hi = parallel.shard_bounds(4_000_000, 5, 8)
    assert hi - lo == 500_000
    r2, n2, s2, st2 = m.trace(pos[lo:hi], d[lo:hi], w[lo:hi], params=p)
    assert np.array_equal(r2, rows[lo:hi]) and np.array_equal(n2, nrows[lo:hi]) and np.array_equal(s2, stop[lo:hi])
    assert st2 == int(nrows[lo:hi].astype(np.int64).sum() - (hi - lo))


def test_full_size_config5_scattered_1m(tmp_path):
    """BASELINE config[4]: 1M rays (seed 5) against the 825 k-sample set of SURVEY 8d (200 k uniform + 600 k importance-
    sampled + 25 k shell), maxsteps 64 -- properties only (one 24 s launch), and a shuffled subset bit for bit."""
    from stanford_raytracer_amd import api

    pts, lnN = wl.make_points_config5(5)
    pf = str(tmp_path / "pts825k.bin")
    api.write_points_file(pf, np.concatenate([pts, lnN], axis=1), np.array([-10.0 * wl.R_E, 10.0 * wl.R_E] * 3), wl.QS, wl.MS, binary=True)
    m = api.Model.scattered_file(pf, window_scale=1.5, order=2, exact=0, local_window_scale=5.0)
    pos, d, w = wl.launch_set(1_000_000, 5)
    p = api.make_params(fixedstep=0, dt0=1e-3, dtmax=0.1, maxerr=5e-4, tmax=0.5, maxsteps=64, outputper=8, del_=1e-6,
                        minalt=wl.MINALT)  # (bench.py WORKLOADS["scattered825k"])
    rows, nrows, stop, steps = m.trace(pos, d, w, params=p)
    check_invariants(pos, rows, nrows, stop, steps, p)
    assert steps > 50_000_000
    idx = np.random.default_rng(7).choice(len(w), 2048, replace=False)
    r2, n2, s2, _ = m.trace(pos[idx], d[idx], w[idx], params=p)
    assert np.array_equal(r2, rows[idx]) and np.array_equal(n2, nrows[idx]) and np.array_equal(s2, stop[idx])
    m.close()


@pytest.mark.parametrize("name", ["ngo", "interp", "scattered"])
def test_adaptive_step_control_matches_the_oracle(gpu_models, oracle_models, oracle_scattered, name):
    """The controller's first decisions (accept / grow / reject: raytracer.f95:770-817) are the oracle's: the time
    stamps of rows 1-3 agree exactly on nearly all rays (later the step sequences drift apart, SURVEY A-9)."""
    g = gpu_models[name]
    o = oracle_scattered if name == "scattered" else oracle_models[name]
    pos, d, w = wl.launch_set(192, 23)
    if name != "ngo":
        pos = pos * 0.9
    kw = dict(fixedstep=0, dt0=1e-3, dtmax=0.1, tmax=0.05, maxerr=5e-4, maxsteps=30, del_=DELS[name])
    rows, nrows, stop, steps = g.trace(pos, d, w, outputper=1, **kw)
    orows, onrows, ostop, osteps = o.trace(pos, d, w, capacity=30, **kw)
    both = (nrows > 4) & (onrows > 4)
    assert both.sum() >= 80
    same_t = np.all(rows[both, 1:4, 0] == orows[both, 1:4, 0], axis=1)
    # interp / scattered (del = 1e-6): one ulp32 of difference in a B component moves dF/dx by percents (SURVEY A-8), which
    # reaches k within a step and tips grow / no-grow decisions that sit near maxerr/100: 83-85 % measured, both ways
    bar = 0.9 if name == "ngo" else 0.75
    assert same_t.mean() >= bar, "time stamps of rows 1-3 agree on only %.0f %% of the rays" % (100 * same_t.mean())
    assert np.mean(stop == ostop) >= 0.9
