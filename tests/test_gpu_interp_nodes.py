"""GPU (-m gpu): the interp model's node-table layout (api layout="nodes", csrc/srt_interp_nodes.hpp) against the expanded layout
on the same grids -- bit for bit where the arithmetic is the same source (densities, the stencil path through a probe kernel),
and on every rung of the parity ladder the suite applies to gpu_models["interp"], with the same inputs and the same bars.  Each
rung prints the share of its outputs that is bit-equal to the expanded layout's ("FIGURE ..." lines; profiles/interp_nodes/
gpu_figures.txt holds a run's).  No grid is larger than 16^3."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import DELS, G3_INTERP_BARS, vrel
from dispersion_checks import f_scale, rel
from interp_layout_cases import BOUNDS, G0_BAR, analytic_grid, axis_nodes, host_grids, oracle_Ns, oracle_model, point_families
from model_ladder import LADDER, curve_distance, divergence, oracle_yardstick
from stanford_raytracer_amd import workloads as wl

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def figure(what, a, b):
    """prints the share of a's values that are bit-equal to b's"""
    share = float(np.mean(bits(a) == bits(b))) if a.shape == b.shape else float("nan")
    print("FIGURE %s: bit-equal to the expanded layout %.4f (%d values)" % (what, share, a.size))
    return share


@pytest.fixture(scope="module")
def pair16(gpu_models, grid16):
    """(expanded, nodes) on the 16^3 fixture grid"""
    from stanford_raytracer_amd import api

    F, b, qs, ms = grid16
    n = api.Model.interp(F, b, qs, ms, layout="nodes")
    assert n.layout == 1 and n.kind == 3 and gpu_models["interp"].layout == 0
    return gpu_models["interp"], n


# ---- 1. densities ----------------------------------------------------------------------------------------------------------
OTHER_SHAPES = [(4, (9, 11, 7)), (3, (8, 8, 8)), (2, (6, 10, 9)), (1, (5, 5, 5))]  # of test_interp_other_shapes_match_the_oracle
DENSITY_GRIDS = host_grids() + [("%dx%dx%d_ns%d" % (d + (ns,)), analytic_grid(d, ns), BOUNDS, wl.QS[:ns], wl.MS[:ns], None)
                                for ns, d in OTHER_SHAPES]


@pytest.mark.parametrize("case", DENSITY_GRIDS, ids=[g[0] for g in DENSITY_GRIDS])
def test_densities_equal_the_expanded_layouts_bit_for_bit_and_the_oracle(tmp_path, case):
    from stanford_raytracer_amd import api

    name, F, b, qs, ms, derivs = case
    nz, ny, nx, ns = F.shape
    e = api.Model.interp(F, b, qs, ms, derivs=derivs)
    n = api.Model.interp(F, b, qs, ms, derivs=derivs, layout="nodes")
    assert n.device_bytes == nx * ny * nz * ns * 64 and e.device_bytes == (nx + 1) * (ny + 1) * (nz + 1) * ns * 512
    om = oracle_model(tmp_path, name, F, b, qs, ms, derivs)
    fam = point_families(b, (nx, ny, nz))
    pts = np.concatenate(list(fam.values()))
    ge, gn = e.plasma_params(pts), n.plasma_params(pts)
    want = oracle_Ns(om, pts)
    print("%s: %d points, nodes against the oracle %.3g, expanded %.3g" % (
        name, len(pts), rel(gn[:, 4:4 + ns], want[:, :ns]).max(), rel(ge[:, 4:4 + ns], want[:, :ns]).max()))
    assert same_bits(gn[:, 4:8], ge[:, 4:8]) and same_bits(gn[:, 16:19], ge[:, 16:19])  # Ns, B0
    assert same_bits(gn, ge)
    assert rel(gn[:, 4:4 + ns], want[:, :ns]).max() <= G0_BAR and rel(ge[:, 4:4 + ns], want[:, :ns]).max() <= G0_BAR
    assert np.array_equal(gn[:, 4 + ns:8], np.zeros((len(pts), 4 - ns)))


def test_small_batches_equal_the_same_points_in_a_large_one(pair16, grid16):
    _, n = pair16
    b = grid16[1]
    pts = np.concatenate(list(point_families(b, (16, 16, 16)).values()))[:130]
    pts[3::7] = np.concatenate(list(point_families(b, (16, 16, 16)).values()))[-19:]  # interior and clamped lanes in every wave
    whole = n.plasma_params(pts)
    for k in (1, 63, 65):
        assert same_bits(n.plasma_params(pts[:k]), whole[:k]), k
        assert same_bits(n.plasma_params(pts[130 - k:]), whole[130 - k:]), k


# ---- 2. the stencil path, through the probe --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe():
    from stanford_raytracer_amd import build

    L = C.CDLL(build.PROBE)
    L.inp_stencils.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def stencil_waves(b, delta):
    """dict name -> (centres[64, 3], offsets[64, 3], free points[64, 3]) on the 16^3 grid over bounds b"""
    ax = axis_nodes(b, (16, 16, 16))
    h = np.array([ax[a][1] - ax[a][0] for a in range(3)])
    lo, hi = np.array([a[0] for a in ax]), np.array([a[-1] for a in ax])
    rng = np.random.default_rng(17)

    def interior(n):  # in a random cell of the grid, at least a tenth of the cell (>= 400 km: > delta |x|) away from its faces
        return lo + (rng.integers(0, 15, (n, 3)) + 0.1 + 0.8 * rng.random((n, 3))) * h

    def finish(c, e=None):
        d = delta * np.linalg.norm(c, axis=1, keepdims=True) * np.ones((1, 3))
        return c, d, (c + 0.37 * d if e is None else e)

    out = {"interior": finish(interior(64))}
    # centres 0.3 delta above a node in 1, 2 and 3 coordinates: the minus offsets of those axes lie in the neighbouring cell
    c = interior(64)
    dn = delta * np.linalg.norm(c, axis=1)
    for i in range(64):
        for a in range(1 + i % 3):
            node = ax[a][1 + (i * 5 + a * 3) % 14]
            c[i, a] = node + 0.3 * delta * abs(node) if i % 2 else node - 0.3 * dn[i]
    out["face_edge_corner"] = finish(c)
    # clamped cells beyond every face (and beyond edges and corners)
    c = interior(64)
    for i in range(64):
        a = i % 3
        c[i, a] = lo[a] - (0.1 + i) * 0.05 * h[a] if (i // 3) % 2 else hi[a] + i * 0.05 * h[a]  # (i = 0: exactly the last node)
        if i % 7 == 0:
            c[i, (a + 1) % 3] = hi[(a + 1) % 3] + 0.5 * h[(a + 1) % 3]
        if i % 21 == 0:
            c[i, (a + 2) % 3] = lo[(a + 2) % 3] - 0.5 * h[(a + 2) % 3]
    out["clamped"] = finish(c)
    c = interior(64)
    c[1::2] = out["clamped"][0][1::2]
    out["interior_and_clamped"] = finish(c)
    c = interior(64)
    e = c + h * np.where(rng.random((64, 3)) < 0.5, -1.0, 1.0)
    e[::9] = c[::9] + 40.0 * h  # (beyond the grid)
    out["free_point_elsewhere"] = finish(c, e)
    c = interior(64)
    c[23, 1] = np.nan
    out["one_nan_lane"] = finish(c)
    return out


@pytest.mark.parametrize("delta", [1e-6, 1e-4])
def test_stencil_lookups_equal_the_expanded_layouts_bit_for_bit(pair16, probe, grid16, delta):
    from stanford_raytracer_amd import api

    e, n = pair16
    pe, pn = api.lib().srt_model_device_struct(e.h), api.lib().srt_model_device_struct(n.h)
    assert pe and pn
    waves = stencil_waves(grid16[1], delta)
    ax = axis_nodes(grid16[1], (16, 16, 16))

    def cell(p):
        return np.stack([np.searchsorted(ax[a], p[:, a], side="right") for a in range(3)], axis=1)

    for name, (c, d, x) in waves.items():
        c, d, x = (np.ascontiguousarray(v) for v in (c, d, x))
        out = np.zeros((3, 64, 8, 4))
        assert probe.inp_stencils(pe, pn, 64, c.ctypes.data, d.ctypes.data, x.ctypes.data, out.ctypes.data) == 0, name
        # the waves are what they are meant to be
        ok = ~np.isnan(c).any(axis=1)
        cc = cell(c[ok])
        clamped = ((cc < 1) | (cc > 15)).any(axis=1)
        straddle = sum((cell(c[ok] + s * d[ok] * np.eye(3)[a]) != cc).any(axis=1).astype(int) for a in range(3) for s in (1, -1))
        if name == "interior":
            assert not clamped.any() and not straddle.any()
        if name == "face_edge_corner":
            assert set(straddle.tolist()) >= {1, 2, 3}
        if name == "clamped":
            assert clamped.all() and all((cc[:, a] < 1).any() and (cc[:, a] > 15).any() for a in range(3))
        if name == "interior_and_clamped":
            assert clamped.any() and not clamped.all()
        if name == "free_point_elsewhere":
            assert (cell(x) != cc).any(axis=1).all()
        if name == "one_nan_lane":
            assert ok.sum() == 63
        print("delta %g %s: stencil == expanded %.4f, stencil == per-point form %.4f" % (
            delta, name, np.mean(bits(out[1]) == bits(out[0])), np.mean(bits(out[1]) == bits(out[2]))))
        assert same_bits(out[1], out[0]), name
        assert same_bits(out[1], out[2]), name
        assert np.all(np.isfinite(out[1][ok])) and np.all(out[1][ok] > 0)


# ---- 3. the rungs of gpu_models["interp"], on the node table ----------------------------------------------------------------
def test_g1_dispersion_vs_golden(golden, pair16):
    from oracle import oracle

    e, n = pair16
    rows, ref = golden["g1_interp_in"], golden["g1_interp_out"]
    g = n.dispersion(rows[:, 0:3], rows[:, 3:6], rows[:, 6])
    figure("G1 dispersion", g, e.dispersion(rows[:, 0:3], rows[:, 3:6], rows[:, 6]))
    assert rel(g[:, 1:6], ref[:, 1:6]).max() <= 1e-10  # S D P R L
    sc = f_scale(rows, ref, oracle.lib().so_speed_of_light())
    assert np.max(np.abs(g[:, 0] - ref[:, 0]) / sc) <= 1e-10
    for c in (6, 8):
        mag_g, mag_r = np.hypot(g[:, c], g[:, c + 1]), np.hypot(ref[:, c], ref[:, c + 1])
        assert rel(mag_g, mag_r).max() <= 1e-10
        assert np.all(np.abs(g[:, c] - ref[:, c]) <= 1e-10 * mag_r)
        assert np.all(np.abs(np.abs(g[:, c + 1]) - np.abs(ref[:, c + 1])) <= 1e-10 * mag_r)


def test_g2_gradients(golden, pair16):
    e, n = pair16
    rows, ref = golden["g2_interp_in"], golden["g2_interp_out"]
    g = n.gradients(rows[:, 0:3], rows[:, 3:6], rows[:, 6], DELS["interp"])
    figure("G2 gradients", g, e.gradients(rows[:, 0:3], rows[:, 3:6], rows[:, 6], DELS["interp"]))
    assert vrel(g[:, 0:3], ref[:, 0:3]).max() <= 1e-7
    assert rel(g[:, 3], ref[:, 3]).max() <= 1e-6
    ex = vrel(g[:, 4:7], ref[:, 4:7])
    assert np.median(ex) <= 1e-7 and np.percentile(ex, 95) <= 1e-5
    assert vrel(g[:, 7:10], ref[:, 7:10]).max() <= 1e-6  # dx/dt
    ek = vrel(g[:, 10:13], ref[:, 10:13])               # dk/dt
    assert np.median(ek) <= 1e-6 and np.percentile(ek, 95) <= 2e-5


def test_g3_single_steps(golden, pair16):
    e, n = pair16
    rows, ref = golden["g3_interp_in"], golden["g3_interp_out"]
    g = n.rk_step(rows[:, 0:7], rows[:, 7], DELS["interp"])
    figure("G3 single steps", g, e.rk_step(rows[:, 0:7], rows[:, 7], DELS["interp"]))
    b = G3_INTERP_BARS
    for o in (0, 7, 14):
        ex = vrel(g[:, o:o + 3], ref[:, o:o + 3])
        ek = vrel(g[:, o + 3:o + 6], ref[:, o + 3:o + 6])
        assert np.median(ex) <= b["pos_median"] and ex.max() <= b["pos_max"]
        assert np.median(ek) <= b["k_median"] and np.percentile(ek, 90) <= b["k_p90"] and ek.max() <= b["k_max"]
        assert np.mean(ek <= 1e-7) >= b["k_frac_tight"]
        assert np.array_equal(g[:, o + 6], ref[:, o + 6])  # omega is carried unchanged


def test_layered_entry_points_handle_ragged_sizes(pair16, oracle_models):
    e, n = pair16
    for k in (0, 1, 63, 65, 130):
        pos, d, w = wl.launch_set(max(k, 1), 77)
        pos = pos[:k]
        out = n.plasma_params(pos)
        assert out.shape == (k, 19)
        if k:
            o = np.array([np.concatenate(oracle_models["interp"].plasma_params(p)) for p in pos])
            assert rel(out[:, 4:8], o[:, 4:8]).max() <= 1e-11
            assert same_bits(out, e.plasma_params(pos))


def test_fixed_step_trajectories(golden, pair16, oracle_models):
    e, n = pair16
    tag, rows_at = "g4_interp_fixed", (1, 10, 50)
    rays, prm = golden["g4_rays"], golden[tag + "_params"]
    ref_rows, ref_n, ref_stop = golden[tag + "_rows"], golden[tag + "_nrows"], golden[tag + "_stop"]
    kw = dict(dt0=prm[0], dtmax=prm[1], tmax=prm[2], maxerr=prm[3], minalt=prm[4], maxsteps=int(prm[5]),
              root=int(prm[6]), fixedstep=1, del_=DELS["interp"])
    cap = int(ref_rows.shape[1])
    rows, nrows, stop, steps = n.trace(rays[:, :3], rays[:, 3:6], rays[:, 6], outputper=1, **dict(kw, maxsteps=cap + 1))
    er = e.trace(rays[:, :3], rays[:, 3:6], rays[:, 6], outputper=1, **dict(kw, maxsteps=cap + 1))
    figure("G4 fixed-step rows", rows, er[0])
    assert np.array_equal(nrows, ref_n) and np.array_equal(stop, ref_stop)
    assert steps == int((ref_n - 1).sum())
    assert np.array_equal(rows[:, 0, 0:4], ref_rows[:, 0, 0:4])
    assert vrel(rows[:, 0, 13:16], ref_rows[:, 0, 13:16]).max() <= 2e-7
    assert vrel(rows[:, 0, 10:13], ref_rows[:, 0, 10:13]).max() <= 1e-10
    assert vrel(rows[:, 0, 7:10], ref_rows[:, 0, 7:10]).max() <= 1e-6
    _, yard = oracle_yardstick(oracle_models["interp"], rays, dict(kw, maxsteps=cap + 1), rows_at, cap)
    for r in rows_at:
        d = divergence(rows, nrows, ref_rows, ref_n, r, slice(1, 4))
        bound = 10 * max(yard[r], LADDER.get(r, 4e-5))
        assert d <= bound, "row %d: position divergence %.2e > %.2e" % (r, d, bound)
        assert np.allclose(rows[:, r, 0], ref_rows[:, r, 0], rtol=1e-12)


@pytest.mark.parametrize("tag", ["g4_interp_adaptive", "g4_interp_launch"])
def test_adaptive_trajectories(golden, pair16, oracle_models, tag):
    e, n = pair16
    rays = golden["g4_launch_rays" if tag.endswith("launch") else "g4_rays"]
    prm = golden[tag + "_params"]
    ref_rows, ref_n, ref_stop = golden[tag + "_rows"], golden[tag + "_nrows"], golden[tag + "_stop"]
    kw = dict(dt0=prm[0], dtmax=prm[1], tmax=prm[2], maxerr=prm[3], minalt=prm[4], maxsteps=int(prm[5]), root=int(prm[6]),
              fixedstep=0, del_=DELS["interp"])
    rows, nrows, stop, _ = n.trace(rays[:, :3], rays[:, 3:6], rays[:, 6], outputper=1, **kw)
    er = e.trace(rays[:, :3], rays[:, 3:6], rays[:, 6], outputper=1, **kw)
    figure("G4 adaptive rows " + tag, rows, er[0])
    print("FIGURE G4 adaptive %s: row counts equal %s, stop codes equal %s" % (tag, np.array_equal(nrows, er[1]), np.array_equal(stop, er[2])))
    om = oracle_models["interp"]
    cap = int(ref_rows.shape[1])
    base = om.trace(rays[:, :3], rays[:, 3:6], rays[:, 6], capacity=cap, **kw)
    assert np.array_equal(base[1], ref_n) and np.array_equal(base[2], ref_stop)
    yard_curve, yard_stop, yard_rows = 0.0, 1.0, 0
    for eps in (1e-9, -1e-9):
        pert = om.trace(rays[:, :3] * (1 + eps), rays[:, 3:6], rays[:, 6], capacity=cap, **kw)
        yard_curve = max(yard_curve, curve_distance(pert[0], pert[1], base[0], base[1], 0.1))
        yard_stop = min(yard_stop, float(np.mean(pert[2] == base[2])))
        yard_rows = max(yard_rows, abs(int(pert[1].sum()) - int(base[1].sum())))
    assert np.mean(stop == ref_stop) >= min(0.9, yard_stop - 1.0 / len(stop))
    both = (nrows > 2) & (ref_n > 2)
    assert np.allclose(rows[both, 1, 0], prm[0]) and np.all(rows[both, 2, 0] <= 2 * prm[0] * (1 + 1e-12))
    assert abs(int(nrows.sum()) - int(ref_n.sum())) <= max(3 * yard_rows, 0.05 * ref_n.sum())
    assert curve_distance(rows, nrows, ref_rows, ref_n, 0.1) <= max(3 * yard_curve, 1e-3)


# ---- 4. lane independence ---------------------------------------------------------------------------------------------------
def test_a_rays_result_does_not_depend_on_its_lane(pair16):
    _, n = pair16
    pos, d, w = wl.launch_set(65, 91)
    pos[5] *= 5.3 * wl.R_E / np.abs(pos[5]).max()  # one ray in the clamped cells beside interior ones
    kw = dict(fixedstep=1, dt0=1e-3, tmax=0.02, maxsteps=12, del_=1e-6)
    a = n.trace(pos, d, w, **kw)
    sub = np.random.default_rng(3).permutation(65)[:40]
    c = n.trace(pos[sub], d[sub], w[sub], **kw)
    assert same_bits(c[0], a[0][sub]) and np.array_equal(c[1], a[1][sub]) and np.array_equal(c[2], a[2][sub])
    o = n.trace(pos, d, w, ray_order=1, **kw)  # the launch-cell order: keys from the same axes on both layouts
    assert same_bits(o[0], a[0]) and np.array_equal(o[1], a[1]) and np.array_equal(o[2], a[2])


# ---- 5. field options -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", ["igrf", "t04"])
def test_field_options(grid16, golden, field):
    """16 fixed-step rays, 4 steps.  Bar on the rows: the fixed-step trajectory bar of the rung above, 10 x the ladder's figure
    for the row (1.2e-10 after one step, 7e-8 after ten: rows 2 .. 4 take the latter)."""
    from stanford_raytracer_amd import api

    F, b, qs, ms = grid16
    pm = [2.0, -10.0, 1.0, -2.0, 0.1, 0.2, 0.1, 0.3, 0.2, 0.4]
    models = []
    for layout in ("expanded", "nodes"):
        m = api.Model.interp(F, b, qs, ms, layout=layout)
        m.set_field(use_igrf=1, use_tsyganenko=int(field == "t04"), parmod=pm if field == "t04" else None)
        models.append(m)
    rays = golden["g4_rays"]
    kw = dict(fixedstep=1, dt0=1e-3, dtmax=0.1, tmax=1.0, maxerr=5e-4, maxsteps=5, del_=1e-6)
    re_, ne, se, _ = models[0].trace(rays[:, :3], rays[:, 3:6], rays[:, 6], **kw)
    rn, nn, sn, _ = models[1].trace(rays[:, :3], rays[:, 3:6], rays[:, 6], **kw)
    figure("field option %s rows" % field, rn, re_)
    assert np.array_equal(nn, ne) and np.array_equal(sn, se) and nn.max() == 5
    for r in range(1, 5):
        bound = 10 * (LADDER[1] if r == 1 else LADDER[10])
        assert divergence(rn, nn, re_, ne, r, slice(1, 4)) <= bound, r


# ---- 6. constructors --------------------------------------------------------------------------------------------------------
def test_constructors(tmp_path, grid16, cfgfiles):
    from stanford_raytracer_amd import api

    F, b, qs, ms = grid16
    G = analytic_grid((3, 4, 5), 4)
    D = wl.synthetic_derivs(G.shape)
    pts = np.concatenate(list(point_families(BOUNDS, (3, 4, 5), nrandom=60).values()))
    # text and binary files, without and with supplied derivatives
    for binary in (False, True):
        for derivs in (None, D):
            path = str(tmp_path / ("g_%d_%d" % (binary, derivs is not None)))
            api.write_grid_file(path, G, BOUNDS, wl.QS, wl.MS, derivs=derivs, binary=binary)
            e, n = api.Model.interp_file(path), api.Model.interp_file(path, layout="nodes")
            assert (e.layout, n.layout) == (0, 1) and e.kind == n.kind == 3
            assert n.device_bytes == 3 * 4 * 5 * 4 * 64 and e.device_bytes == 4 * 5 * 6 * 4 * 512
            assert same_bits(n.plasma_params(pts), e.plasma_params(pts))
    # from a handle (the Ngo model on a 12^3 grid), compder 0 and 1
    src = api.Model.ngo(cfgfiles["ngo"])
    assert src.layout == -1
    bb = np.array([1.5, 3.5, -1.0, 1.0, -1.0, 1.0]) * wl.R_E
    q = np.concatenate(list(point_families(bb, (12, 12, 12), nrandom=60).values()))
    for compder in (False, True):
        e, n = src.to_interp(12, 12, 12, bb, compder=compder), src.to_interp(12, 12, 12, bb, compder=compder, layout="nodes")
        assert (e.layout, n.layout) == (0, 1)
        assert n.device_bytes == 12 ** 3 * 4 * 64 and e.device_bytes == 13 ** 3 * 4 * 512
        assert same_bits(n.plasma_params(q), e.plasma_params(q))
    # AUTO on a 16^3 grid: the expanded table fits
    a = api.Model.interp(F, b, qs, ms, layout="auto")
    assert a.layout == 0 and a.device_bytes == 17 ** 3 * 4 * 512
    assert api.lib().srt_model_interp_layout(a.h) == 0


# ---- 7. as a source model ---------------------------------------------------------------------------------------------------
def test_builders_from_a_node_table_handle(pair16):
    e, n = pair16
    bb = np.array([1.5, 3.5, -1.0, 1.0, -1.0, 1.0]) * wl.R_E
    Fe, De = e.build_grid(7, 6, 5, bb, compder=True)
    Fn, Dn = n.build_grid(7, 6, 5, bb, compder=True)
    assert same_bits(Fn, Fe) and all(same_bits(x, y) for x, y in zip(Dn, De))
    kw = dict(n_initial_radial=100, n_initial_uniform=200, adaptive_nmax=300, initial_tol=1.0, max_recursion=10, seed=3)
    bs = np.array([-3.0, 3.0, -3.0, 3.0, -3.0, 3.0]) * wl.R_E
    se, ce = e.build_samples(bs, **kw)
    sn, cn = n.build_samples(bs, **kw)
    assert ce == cn and len(se) > 500 and same_bits(sn, se)
