"""GPU (-m gpu): the HIP path through the C ABI against the CPU oracle and the reference's golden
vectors, rung by rung (SURVEY.md A-9 ladder).  Tolerances are fp64 tolerances of THIS path:

  G0 funcPlasmaParams   Ns <= 1e-11 rel; B0 <= 2e-7 rel (the adapters round B through float32 nT, so a
                        last-bit difference before the rounding may flip one float32 ulp = 6e-8)
  G1 Stix / F / roots   <= 1e-10 rel (F: relative to the size of its cancelling terms)
  G2 FD gradients       dF/dk <= 1e-7, dF/dw <= 1e-6 (central differences with a 1e-8 relative step amplify
                        1-ulp differences by 1e8: the reference differs from its own FMA rebuild by 2e-8)
                        dF/dx: Ngo <= 1e-7; interp (del = 1e-6, float32 staircase in B, SURVEY A-8):
                        median <= 1e-7, 95th percentile <= 1e-5
  G3 one RK step        Ngo: position median <= 1e-8 of |x|, max <= 1e-7; k median <= 1e-7 of |k|.
                        interp (16^3 grid): bars of conftest.G3_INTERP_BARS = the reference's own sensitivity to a
                        1e-13 input perturbation (float32-staircase flips over the dF/dx stencil), pinned on the
                        CPU by test_oracle_golden.py::test_g3_interp_self_sensitivity
"""
import numpy as np
import pytest

from conftest import DELS, G3_INTERP_BARS, vrel
from dispersion_checks import f_scale, rel

pytestmark = pytest.mark.gpu
MODELS = ["ngo", "ngoducts", "interp"]


@pytest.mark.parametrize("name", MODELS)
def test_g0_params_vs_golden_and_oracle(golden, gpu_models, oracle_models, name):
    x, ref = golden["g0_%s_x" % name], golden["g0_%s_out" % name]
    g = gpu_models[name].plasma_params(x)
    assert np.array_equal(g[:, 0:4], ref[:, 0:4]) and np.array_equal(g[:, 8:12], ref[:, 8:12])  # qs, ms
    assert np.all(g[:, 12:16] == 0)
    assert rel(g[:, 4:8], ref[:, 4:8]).max() <= 1e-11
    assert vrel(g[:, 16:19], ref[:, 16:19]).max() <= 2e-7
    assert np.mean(vrel(g[:, 16:19], ref[:, 16:19]) < 1e-13) > 0.98
    o = np.array([np.concatenate(oracle_models[name].plasma_params(p)) for p in x])
    assert rel(g[:, 4:8], o[:, 4:8]).max() <= 1e-11


def test_g0_interp_out_of_range_and_nodes(gpu_models, oracle_models, grid16):
    """Cells below/above the grid (clamped corners, sticky derivative flags, SURVEY A-7) and exact node hits."""
    F, b, _, _ = grid16
    ax = np.arange(16) * ((b[1] - b[0]) / 15.0) + b[0]
    pts = []
    for xi in (ax[0] - 5.0, ax[0], ax[1], ax[7] + 1.0, ax[14], ax[15] - 1e-3, ax[15], ax[15] + 7.0):
        for yi in (ax[0] - 1.0, ax[3], ax[15], ax[15] + 2.0):
            for zi in (ax[0] - 9.0, ax[0], ax[8] + 3.0, ax[15], ax[15] + 1.0):
                pts.append([xi, yi, zi])
    pts = np.array(pts)
    g = gpu_models["interp"].plasma_params(pts)
    o = np.array([np.concatenate(oracle_models["interp"].plasma_params(p)) for p in pts])
    assert rel(g[:, 4:8], o[:, 4:8]).max() <= 1e-11


@pytest.mark.parametrize("name", MODELS)
def test_g1_dispersion_vs_golden(golden, gpu_models, name):
    from oracle import oracle

    rows, ref = golden["g1_%s_in" % name], golden["g1_%s_out" % name]
    g = gpu_models[name].dispersion(rows[:, 0:3], rows[:, 3:6], rows[:, 6])
    assert rel(g[:, 1:6], ref[:, 1:6]).max() <= 1e-10  # S D P R L
    sc = f_scale(rows, ref, oracle.lib().so_speed_of_light())
    assert np.max(np.abs(g[:, 0] - ref[:, 0]) / sc) <= 1e-10
    # roots: real parts, and imaginary parts up to the sign of the branch (signed zeros pick it in the
    # reference; only |Im| is ever used, raytracer.f95:891)
    for c in (6, 8):
        mag_g, mag_r = np.hypot(g[:, c], g[:, c + 1]), np.hypot(ref[:, c], ref[:, c + 1])
        assert rel(mag_g, mag_r).max() <= 1e-10
        assert np.all(np.abs(g[:, c] - ref[:, c]) <= 1e-10 * mag_r)
        assert np.all(np.abs(np.abs(g[:, c + 1]) - np.abs(ref[:, c + 1])) <= 1e-10 * mag_r)


def test_g1_is_right_handed_matches_reference(golden):
    from stanford_raytracer_amd import api

    rows, ref = golden["g1_rh_in"], golden["g1_rh_out"]
    g = api.is_right_handed(rows)
    assert np.array_equal(g.astype(float), ref)


@pytest.mark.parametrize("name", MODELS)
def test_g2_gradients(golden, gpu_models, name):
    rows, ref = golden["g2_%s_in" % name], golden["g2_%s_out" % name]
    g = gpu_models[name].gradients(rows[:, 0:3], rows[:, 3:6], rows[:, 6], DELS[name])
    assert vrel(g[:, 0:3], ref[:, 0:3]).max() <= 1e-7
    assert rel(g[:, 3], ref[:, 3]).max() <= 1e-6
    ex = vrel(g[:, 4:7], ref[:, 4:7])
    if name == "interp":
        assert np.median(ex) <= 1e-7 and np.percentile(ex, 95) <= 1e-5
    else:
        assert ex.max() <= 1e-7
    assert vrel(g[:, 7:10], ref[:, 7:10]).max() <= 1e-6  # dx/dt
    ek = vrel(g[:, 10:13], ref[:, 10:13])               # dk/dt
    assert np.median(ek) <= 1e-6 and np.percentile(ek, 95) <= 2e-5


@pytest.mark.parametrize("name", MODELS)
def test_g3_single_steps(golden, gpu_models, name):
    rows, ref = golden["g3_%s_in" % name], golden["g3_%s_out" % name]
    g = gpu_models[name].rk_step(rows[:, 0:7], rows[:, 7], DELS[name])
    for o in (0, 7, 14):
        ex = vrel(g[:, o:o + 3], ref[:, o:o + 3])
        ek = vrel(g[:, o + 3:o + 6], ref[:, o + 3:o + 6])
        if name == "interp":
            # Bars = the reference's OWN sensitivity: tests/test_oracle_golden.py::test_g3_interp_self_sensitivity
            # perturbs the step inputs by 1e-13 and finds position median 2e-8 / max 7e-6 and k median 2e-5 /
            # p90 1.4e-4 / max 6e-4, with only ~30 % of the samples untouched (<= 1e-7): a sample either sees the
            # same float32 steps of B over the dF/dx stencil (SURVEY A-8) or one step flips.
            b = G3_INTERP_BARS
            assert np.median(ex) <= b["pos_median"] and ex.max() <= b["pos_max"]
            assert np.median(ek) <= b["k_median"] and np.percentile(ek, 90) <= b["k_p90"] and ek.max() <= b["k_max"]
            assert np.mean(ek <= 1e-7) >= b["k_frac_tight"]
        else:
            assert np.median(ex) <= 1e-8 and ex.max() <= 1e-7
            assert np.median(ek) <= 1e-7
            assert ek.max() <= 1e-2
        assert np.array_equal(g[:, o + 6], ref[:, o + 6])  # omega is carried unchanged


def test_layered_entry_points_handle_ragged_sizes(gpu_models, oracle_models):
    """n not a multiple of the wave size, n = 1, n = 0."""
    from stanford_raytracer_amd import workloads as wl

    m = gpu_models["interp"]
    for n in (0, 1, 63, 65, 130):
        pos, d, w = wl.launch_set(max(n, 1), 77)
        pos = pos[:n]
        out = m.plasma_params(pos)
        assert out.shape == (n, 19)
        if n:
            o = np.array([np.concatenate(oracle_models["interp"].plasma_params(p)) for p in pos])
            assert rel(out[:, 4:8], o[:, 4:8]).max() <= 1e-11


# ---- modelnum 4: scattered samples, moving least squares (uniform-grid neighbour search on the device) ----------
@pytest.fixture(scope="module")
def scat_o3():
    import os

    from conftest import GOLDEN_DIR
    return np.load(os.path.join(GOLDEN_DIR, "scattered_o3_golden.npz"))


@pytest.mark.parametrize("key,kw", [("g0_scattered_out", {}), ("g0_scattered_o1_out", {"order": 1}),
                                    ("g0_scattered_exact_out", {"exact": 1, "local_window_scale": 2.0}),
                                    ("g0_o3_out", {"order": 3})])
def test_g0_scattered_params(golden, scat_o3, pointsfile, key, kw):
    """funcPlasmaParams of modelnum 4 against the reference's own outputs, orders 1, 2, 3 and the exact window.
    The reference stores a ZERO nearest-sample distance for the one sample at the root of its kd-tree (its
    kdtree_nearest starts from the root; which sample that is comes from the compiler's RNG).  That sample is known
    (ref_harness --mode=scatroot -> ref_root_point): exactly the lookups whose search window holds it are perturbed
    by the quirk (the CPU test shows the oracle reproduces them once the quirk is put in); the HIP path stores the
    true distance, so those lookups are held against the oracle with true distances instead."""
    from oracle import oracle
    from stanford_raytracer_amd import api

    m = api.Model.scattered_file(pointsfile, **kw)
    x, ref = golden["g0_scattered_x"], (scat_o3[key] if key == "g0_o3_out" else golden[key])
    g = m.plasma_params(x)
    assert np.array_equal(g[:, 0:4], ref[:, 0:4]) and np.array_equal(g[:, 8:12], ref[:, 8:12])
    assert vrel(g[:, 16:19], ref[:, 16:19]).max() <= 2e-7
    assert np.array_equal(g[-5:-3, 4:8], np.zeros((2, 4)))   # inside the Earth
    assert np.array_equal(g[-2:, 4:8], np.ones((2, 4)))      # too few neighbours -> exp(0)
    ok = ref[:, 4] > 0
    radius = float(scat_o3["ref_maxnearest"]) * 1.5           # maxnearest * window_scale
    near = np.linalg.norm(x - scat_o3["ref_root_point"], axis=1) < radius
    assert 0 < near.sum() < 10
    far = ok & ~near
    e = np.abs(g[far, 4:8] - ref[far, 4:8]) / ref[far, 4:8]
    assert e.max() <= 1e-9, e.max()                           # summation order only
    o = oracle.Model.scattered_file(pointsfile, perm_seed=2 | 0x80000000, **kw)   # true distance for every sample
    on = np.array([np.concatenate(o.plasma_params(p)) for p in x[near]])
    assert (np.abs(g[near, 4:8] - on[:, 4:8]) / on[:, 4:8]).max() <= 1e-9


def test_g2_scattered_order3_gradients(scat_o3, pointsfile):
    """The cooperative stencil path with the J = 20 fit (shared_fit<20>: 84 moments + 80 sums, lsinterp_mod.f95:91-99)
    against the reference's own dFdk, dFdw, dFdx; and the own-list path (SRT_SCATTERED_STAGING=0 is covered in
    tests/test_gpu_scattered_paths.py)."""
    from stanford_raytracer_amd import api

    m = api.Model.scattered_file(pointsfile, order=3)
    gin, ref = scat_o3["g2_o3_in"], scat_o3["g2_o3_out"]
    radius = float(scat_o3["ref_maxnearest"]) * 1.5
    far = np.linalg.norm(gin[:, 0:3] - scat_o3["ref_root_point"], axis=1) >= radius
    g = m.gradients(gin[:, 0:3], gin[:, 3:6], gin[:, 6], 1e-6)
    assert far.sum() >= 50
    assert vrel(g[far, 0:3], ref[far, 0:3]).max() <= 1e-7
    assert (np.abs(g[far, 3] - ref[far, 3]) / np.abs(ref[far, 3])).max() <= 1e-6
    ex = vrel(g[far, 4:7], ref[far, 4:7])   # d(ln N) over a 10 m stencil: 1e-13 / 1e-6 amplification
    assert np.median(ex) <= 1e-5 and np.percentile(ex, 90) <= 1e-3


@pytest.fixture(scope="module")
def scat_o45():
    import os

    from conftest import GOLDEN_DIR
    return np.load(os.path.join(GOLDEN_DIR, "scattered_o45_golden.npz"))


@pytest.mark.parametrize("order", [4, 5])
def test_scattered_orders_4_and_5(scat_o45, pointsfile, order):
    """The generate_monomials orders (lsinterp_mod.f95:114-164, 273-281; J = 35 / 56) through srt_scattered.hpp's gen_point: the
    layered kernels (funcPlasmaParams: one point per lane, the wave fitting them one after the other) and the stencil service of the
    gradient / trace kernels (gen_stencil), against the reference's own outputs and against the oracle where the reference's
    tree-root quirk reaches (as test_g0_scattered_params).  With the narrow window the fits that have fewer samples than monomials
    answer exp(0) = 1 like the reference's."""
    from oracle import oracle
    from stanford_raytracer_amd import api

    ws = float(scat_o45["window_scale"])
    x, rootp = scat_o45["g0_x"], scat_o45["ref_root_point"]
    for key, w in (("g0_o%d_out" % order, ws), ("g0_o%d_narrow_out" % order, 1.5)):
        ref = scat_o45[key]
        xs = x[:len(ref)]
        m = api.Model.scattered_file(pointsfile, order=order, window_scale=w)
        g = m.plasma_params(xs)
        assert np.array_equal(g[:, 0:4], ref[:, 0:4]) and np.array_equal(g[:, 8:12], ref[:, 8:12])
        near = np.linalg.norm(xs - rootp, axis=1) < float(scat_o45["ref_maxnearest"]) * w
        o = oracle.Model.scattered_file(pointsfile, perm_seed=2 | 0x80000000, order=order, window_scale=w)  # true distances
        want = ref[:, 4:8].copy()
        if near.any():
            want[near] = np.array([np.concatenate(o.plasma_params(p)) for p in xs[near]])[:, 4:8]
        assert np.array_equal(g[:, 4] == 1.0, want[:, 0] == 1.0)      # the same fits fail
        e = np.abs(g[:, 4:8] - want) / want
        assert e.max() <= (1e-9 if w == ws else 1e-6), e.max()
    m = api.Model.scattered_file(pointsfile, order=order, window_scale=ws)
    gin, ref = scat_o45["g2_in"], scat_o45["g2_o%d_out" % order]
    far = np.linalg.norm(gin[:, 0:3] - rootp, axis=1) >= float(scat_o45["ref_maxnearest"]) * ws
    assert far.sum() >= 16
    g = m.gradients(gin[:, 0:3], gin[:, 3:6], gin[:, 6], 1e-6)
    assert vrel(g[far, 0:3], ref[far, 0:3]).max() <= 1e-7
    assert (np.abs(g[far, 3] - ref[far, 3]) / np.abs(ref[far, 3])).max() <= 1e-6
    ex = vrel(g[far, 4:7], ref[far, 4:7])   # d(ln N) over a 10 m stencil: 1e-12 / 1e-6 amplification
    assert np.median(ex) <= 1e-4 and np.percentile(ex, 90) <= 1e-2, (np.median(ex), np.percentile(ex, 90))
    if order == 4:
        prm, rays = scat_o45["g4_o4_params"], scat_o45["rays"]
        rows, nrows, stop, _ = m.trace(rays[:, :3], rays[:, 3:6], rays[:, 6], outputper=1, dt0=prm[0], dtmax=prm[1], tmax=prm[2],
                                       maxerr=prm[3], minalt=prm[4], maxsteps=int(prm[5]), root=int(prm[6]), fixedstep=1, del_=1e-6)
        clear = np.array([np.linalg.norm(scat_o45["g4_o4_rows"][i, :6, 1:4] - rootp, axis=1).min() for i in range(len(rays))]) \
            >= float(scat_o45["ref_maxnearest"]) * ws
        assert clear.sum() >= 4
        assert np.array_equal(nrows, scat_o45["g4_o4_nrows"]) and np.array_equal(stop, scat_o45["g4_o4_stop"])
        ref_rows = scat_o45["g4_o4_rows"]
        assert np.array_equal(rows[:, :6, 0], ref_rows[:, :6, 0])
        assert np.allclose(rows[clear, :6, 1:4], ref_rows[clear, :6, 1:4], rtol=1e-5, atol=0)
        assert np.allclose(rows[clear, :6, 16:20], ref_rows[clear, :6, 16:20], rtol=1e-5, atol=0)


def test_scattered_orders_4_and_5_other_shapes(tmp_path, pointsfile):
    """The same path where the reference-held fixture does not go: the exact window (exact = 1: exp(r^2 / h^2) weights) at order 4,
    and a two-species sample file at order 5 (the unused right-hand sums must stay out of the answer) -- against the oracle with
    true distances, which the CPU suite holds to the reference at these orders."""
    import os

    from conftest import GOLDEN_DIR
    from oracle import oracle
    from stanford_raytracer_amd import api, workloads as wl

    pos, _, _ = wl.launch_set(160, 4242)
    pos = pos * 0.9
    m = api.Model.scattered_file(pointsfile, order=4, exact=1, local_window_scale=2.0, window_scale=2.5)
    o = oracle.Model.scattered_file(pointsfile, perm_seed=2 | 0x80000000, order=4, exact=1, local_window_scale=2.0, window_scale=2.5)
    g = m.plasma_params(pos)
    want = np.array([np.concatenate(o.plasma_params(p)) for p in pos])
    fitted = (want[:, 4] > 0) & (want[:, 4] != 1.0)
    assert fitted.sum() >= 100
    assert np.array_equal(g[:, 4] == 1.0, want[:, 4] == 1.0) and np.array_equal(g[:, 4] == 0.0, want[:, 4] == 0.0)
    e = np.abs(g[fitted, 4:8] - want[fitted, 4:8]) / want[fitted, 4:8]
    assert e.max() <= 1e-7 and np.median(e) <= 1e-11, (e.max(), np.median(e))   # the exact window's weights span 1e16: looser at the top
    g0 = np.load(os.path.join(GOLDEN_DIR, "points5500.npz"))
    two = str(tmp_path / "two_species.txt")
    wl.write_points_file(two, g0["pts"], g0["lnN"][:, :2], g0["bounds"], g0["qs"][:2], g0["ms"][:2])
    m2 = api.Model.scattered_file(two, order=5, window_scale=2.5)
    o2 = oracle.Model.scattered_file(two, perm_seed=2 | 0x80000000, order=5, window_scale=2.5)
    g2 = m2.plasma_params(pos[:64])
    w2 = np.array([np.concatenate(o2.plasma_params(p)) for p in pos[:64]])
    assert np.array_equal(g2[:, 6:8], np.zeros((64, 2))) and np.array_equal(w2[:, 6:8], np.zeros((64, 2)))
    ok = (w2[:, 4] > 0) & (w2[:, 4] != 1.0)
    assert ok.sum() >= 40 and np.array_equal(g2[:, 4] == 1.0, w2[:, 4] == 1.0)
    assert (np.abs(g2[ok, 4:6] - w2[ok, 4:6]) / w2[ok, 4:6]).max() <= 1e-9


def test_scattered_order_6_is_refused(pointsfile):
    from stanford_raytracer_amd import api

    with pytest.raises(Exception, match="orders 0..5"):
        api.Model.scattered_file(pointsfile, order=6)


def test_scattered_vs_oracle_ladder(gpu_models, oracle_scattered):
    from stanford_raytracer_amd import workloads as wl

    g, o = gpu_models["scattered"], oracle_scattered
    pos, d, w = wl.launch_set(300, 808)
    pos = pos * 0.9
    gp = g.plasma_params(pos)
    op = np.array([np.concatenate(o.plasma_params(p)) for p in pos])
    assert rel(gp[:, 4:8], op[:, 4:8]).max() <= 1e-9
    od = np.array([o.disp(p, dd, ww) for p, dd, ww in zip(pos, d, w)])
    ok = od[:, 8] > 0
    x, k, ww = pos[ok][:60], (od[ok, 8:9] * d[ok])[:60], w[ok][:60]
    gg = g.gradients(x, k, ww, 1e-6)
    og = np.array([o.grad(a, b, c, 1e-6) for a, b, c in zip(x, k, ww)])
    assert vrel(gg[:, 0:3], og[:, 0:3]).max() <= 1e-7
    ex = vrel(gg[:, 4:7], og[:, 4:7])
    assert np.median(ex) <= 1e-5 and np.percentile(ex, 90) <= 1e-3   # d(ln N) over a 10 m stencil: 1e-13 / 1e-6 amplification


def test_scattered_trajectories(golden, gpu_models, oracle_scattered, pointsfile):
    """The reference's own adaptive rows of the 24 scattered-model launch rays.  Bars: what the ORACLE does to itself under a
    1e-9 shift of the launch points (the machinery of tests/test_gpu_trajectory_stats.py), not constants -- the oracle
    (with the reference's tree-root quirk, perm_seed = 2) is first held to the reference on the same rays."""
    from oracle import oracle
    from model_ladder import compare

    rays, prm = golden["g4_scattered_rays"], golden["g4_scattered_launch_params"]
    ref_rows, ref_n, ref_stop = (golden["g4_scattered_launch_" + k] for k in ("rows", "nrows", "stop"))
    kw = dict(dt0=prm[0], dtmax=prm[1], tmax=prm[2], maxerr=prm[3], minalt=prm[4], maxsteps=int(prm[5]), root=int(prm[6]),
              fixedstep=0, del_=1e-6)
    cap = int(ref_rows.shape[1])
    rows, nrows, stop, _ = gpu_models["scattered"].trace(rays[:, :3], rays[:, 3:6], rays[:, 6], outputper=1, **kw)
    ref = (ref_rows, ref_n, ref_stop)
    # yardstick 1: the oracle built like the reference (its tree root keeps spacing 0) against the reference's rows
    oq = oracle.Model.scattered_file(pointsfile, perm_seed=2)
    oref = compare(oq.trace(rays[:, :3], rays[:, 3:6], rays[:, 6], capacity=cap, **kw)[:3], ref, prm[2])
    # yardstick 2: the oracle against itself, launch points shifted by 1e-9 (~1 cm)
    base = oracle_scattered.trace(rays[:, :3], rays[:, 3:6], rays[:, 6], capacity=cap, **kw)[:3]
    yard = None
    for eps in (1e-9, -1e-9):
        pert = oracle_scattered.trace(rays[:, :3] * (1 + eps), rays[:, 3:6], rays[:, 6], capacity=cap, **kw)[:3]
        c = compare(pert, base, prm[2])
        yard = c if yard is None else {k: (min if k in ("stop_agree", "same_t") else max)(yard[k], c[k]) for k in c}
    mine = compare((rows[:, :cap], nrows, stop), ref, prm[2])
    msg = "\nGPU vs reference: %s\noracle vs reference: %s\noracle vs oracle(launch shifted 1e-9): %s" % (mine, oref, yard)
    print(msg)
    both = (nrows > 1) & (ref_n > 1)
    assert np.array_equal(rows[both, 0, 1:4], ref_rows[both, 0, 1:4])
    e = np.abs(rows[both, 0, 16:20] - ref_rows[both, 0, 16:20]) / ref_rows[both, 0, 16:20]
    assert np.percentile(e, 90) <= 1e-9
    worst = {k: (min if k in ("stop_agree", "same_t") else max)(yard[k], oref[k]) for k in yard}
    n = len(ref_n)
    assert mine["curve_median"] <= 3 * max(worst["curve_median"], 7e-8), msg
    assert mine["curve_p90"] <= 3 * max(worst["curve_p90"], 4e-5), msg
    assert mine["stop_agree"] >= worst["stop_agree"] - 1.5 / n, msg        # at most one more ray of the 24 changes fate
    assert mine["same_t"] >= worst["same_t"] - 2.5 / n, msg
    assert mine["rows_rel"] <= max(3 * worst["rows_rel"], 0.02), msg


# ---- interp model: shapes the cubic 4-species fixture does not exercise ------------------------------------------
@pytest.mark.parametrize("nspec,dims", [(4, (9, 11, 7)), (3, (8, 8, 8)), (2, (6, 10, 9)), (1, (5, 5, 5))])
def test_interp_other_shapes_match_the_oracle(nspec, dims):
    """Non-cubic grids and fewer than four species (the LDS ring streams 4*nspec units; cell strides differ per axis):
    funcPlasmaParams, the finite-difference gradients and one RK step against the CPU oracle on the same grid."""
    from oracle import oracle
    from stanford_raytracer_amd import api, workloads as wl

    nx, ny, nz = dims
    b = np.array([-4.0, 4.5, -5.0, 4.0, -3.5, 4.2]) * wl.R_E
    ax = [np.arange(n) * ((b[2 * a + 1] - b[2 * a]) / (n - 1.0)) + b[2 * a] for a, n in enumerate((nx, ny, nz))]
    Z, Y, X = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    F = wl.analytic_lnN(np.stack([X, Y, Z], axis=-1))[..., :nspec].copy()
    qs, ms = wl.QS[:nspec], wl.MS[:nspec]
    g, o = api.Model.interp(F, b, qs, ms), oracle.Model.interp(F, b, qs, ms)
    pos, d, w = wl.launch_set(400, 99)
    pos = pos * 0.8
    pos[:8] *= 3.0                                          # a few points outside the grid (clamped cells, A-7)
    gp = g.plasma_params(pos)
    op = np.array([np.concatenate(o.plasma_params(p)) for p in pos])
    assert rel(gp[:, 4:4 + nspec], op[:, 4:4 + nspec]).max() <= 1e-11
    assert np.array_equal(gp[:, 4 + nspec:8], np.zeros((len(pos), 4 - nspec)))
    od = np.array([o.disp(p, dd, ww) for p, dd, ww in zip(pos, d, w)])
    ok = od[:, 8] > 0
    x, k, ww = pos[ok][:100], (od[ok, 8:9] * d[ok])[:100], w[ok][:100]
    gg = g.gradients(x, k, ww, 1e-6)
    og = np.array([o.grad(a, c, e, 1e-6) for a, c, e in zip(x, k, ww)])
    assert vrel(gg[:, 0:3], og[:, 0:3]).max() <= 1e-7
    ex = vrel(gg[:, 4:7], og[:, 4:7])
    assert np.median(ex) <= 1e-7 and np.percentile(ex, 95) <= 1e-4
    # a short adaptive trace: launch rows identical, fates largely agree
    kw = dict(fixedstep=0, dt0=1e-3, dtmax=0.1, tmax=0.05, maxerr=5e-4, maxsteps=400, del_=1e-6)  # tmax governs
    rows, nrows, stop, _ = g.trace(pos[8:200], d[8:200], w[8:200], outputper=1, **kw)
    orows, onrows, ostop, _ = o.trace(pos[8:200], d[8:200], w[8:200], capacity=400, **kw)
    both = (nrows > 1) & (onrows > 1)
    assert np.array_equal(rows[both, 0, 1:4], orows[both, 0, 1:4])
    pairs = sorted(set(zip(stop[stop != ostop].tolist(), ostop[stop != ostop].tolist())))
    assert np.mean(stop == ostop) >= 0.9, "fates differ: %s  n=%d/%d" % (pairs, (stop != ostop).sum(), len(stop))
    assert abs(int(nrows.sum()) - int(onrows.sum())) <= 0.1 * onrows.sum()


def test_interp_file_supplied_derivatives(grid16, golden, tmp_path):
    """A modelnum-3 grid with computederivatives = 1: the seven derivative blocks come from the file / the caller
    (interp_dens_model_adapter.f95:107-116) instead of the library's own finite differences.  funcPlasmaParams and the
    gradients against the reference's own outputs for the same file (tests/golden/make_interp_derivs_golden.py), through
    both entry points (host arrays, text file), and against the oracle."""
    import os

    from conftest import GOLDEN_DIR
    from oracle import oracle
    from stanford_raytracer_amd import api, workloads as wl

    F, b, qs, ms = grid16
    derivs = wl.synthetic_derivs(F.shape)
    gd = np.load(os.path.join(GOLDEN_DIR, "interp_derivs_golden.npz"))
    gf = str(tmp_path / "grid16_derivs.txt")
    wl.write_grid_file(gf, F, b, qs, ms, derivs=derivs)
    x, ref = golden["g0_interp_x"], gd["g0_out"]
    models = [api.Model.interp(F, b, qs, ms, derivs=derivs), api.Model.interp_file(gf)]
    outs = [m.plasma_params(x) for m in models]
    assert np.array_equal(outs[0], outs[1])
    g = outs[0]
    assert rel(g[:, 4:8], ref[:, 4:8]).max() <= 1e-11
    assert vrel(g[:, 16:19], ref[:, 16:19]).max() <= 2e-7
    assert rel(g[:, 4:8], golden["g0_interp_out"][:, 4:8]).max() > 1e-2     # not the finite-difference grid's numbers
    gin, gref = gd["g2_in"], gd["g2_out"]
    gg = models[0].gradients(gin[:, 0:3], gin[:, 3:6], gin[:, 6], 1e-6)
    assert vrel(gg[:, 0:3], gref[:, 0:3]).max() <= 1e-7
    ex = vrel(gg[:, 4:7], gref[:, 4:7])
    assert np.median(ex) <= 1e-7 and np.percentile(ex, 95) <= 1e-4          # the bars of the finite-difference grid (G2)
    o = oracle.Model.interp_file(gf)
    op = np.array([np.concatenate(o.plasma_params(p)) for p in x])
    assert rel(g[:, 4:8], op[:, 4:8]).max() <= 1e-11


@pytest.mark.parametrize("key,kw", [("g0_scattered_out", {}), ("g0_o3_out", {"order": 3})])
def test_scattered_root_switch_reproduces_the_reference_everywhere(golden, scat_o3, pointsfile, key, kw):
    """The opt-in srt_model_create_scattered_file_root (CLI --scattered_interp_root_sample): with the sample at the root of the
    REFERENCE's kd-tree named (tests/golden/scattered_o3_golden.npz: ref_root_index, asked of the reference's own tree), its
    stored spacing is 0 as in the reference (kdtree_mod.f95:386-444) and EVERY lookup agrees with the reference's output --
    including the ones whose window holds that sample, which test_g0_scattered_params has to leave to the oracle.  The search
    radius (maxnearest x window_scale) is the reference's, bit for bit."""
    from stanford_raytracer_amd import api

    root = int(scat_o3["ref_root_index"])
    m = api.Model.scattered_file(pointsfile, root_sample=root, **kw)
    x, ref = golden["g0_scattered_x"], (scat_o3[key] if key == "g0_o3_out" else golden[key])
    g = m.plasma_params(x)
    ok = ref[:, 4] > 0
    e = np.abs(g[ok, 4:8] - ref[ok, 4:8]) / ref[ok, 4:8]
    assert e.max() <= 1e-9, e.max()
    assert np.array_equal(g[~ok, 4:8], ref[~ok, 4:8])
    # ... and the default build differs from it exactly at the lookups near that sample
    d = api.Model.scattered_file(pointsfile, **kw).plasma_params(x)
    near = np.linalg.norm(x - scat_o3["ref_root_point"], axis=1) < float(scat_o3["ref_maxnearest"]) * 1.5
    moved = np.abs(d[:, 4] - g[:, 4]) > 1e-12 * np.abs(g[:, 4])
    assert moved.any() and not np.any(moved & ~near)
    with pytest.raises(api.SrtError):
        api.Model.scattered_file(pointsfile, root_sample=10 ** 7)
