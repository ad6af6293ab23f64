"""CPU: traced rays binned onto a grid (include/srt.h) -- csrc/srt_binning.hpp's point functions, the very source the device
compiles, built for the host (tests/native/binning_host.cpp) and held against the closed-form dwell times (B1, a derived bound)
and the numpy restatement of tests/binning_cases.py (B2 .. B7, equality of integers under the precondition stated there); the
refusals, the struct layouts and the file format of the C ABI (B8)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import binning_cases as bc
import crossings_cases as cc
from conftest import ROOT


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return bc.build_host(tmp_path_factory.mktemp("bnh"))


# ---------------------------------------------------------------------------------------------- B1
@pytest.mark.parametrize("nsub", [1, 4, 16])
def test_b1_constant_velocity_through_a_cartesian_grid(host, nsub):
    offsets, rows, axes, lines = bc.b1_cartesian()
    ticks, hits, counters = bc.host_bin(host, offsets, rows, axes, nsub)
    dwell, slack = bc.b1_cartesian_truth(lines, axes)
    total = sum(t1 - t0 for _, _, t0, t1, _ in lines)
    assert dwell.sum() > 0.3 * total and np.count_nonzero(dwell) > 20  # the grid is crossed, not grazed
    bc.b1_check(ticks, hits, dwell, slack, nsub, total, label="B1 cartesian")
    bc.check_identities(ticks, hits, counters, nsub, offsets)
    assert counters[1] == 0 and counters[3] > 0  # some rays start or end outside the grid


@pytest.mark.parametrize("nsub", [1, 4, 16])
def test_b1_a_radial_ray_through_an_r_sinlat_grid(host, nsub):
    offsets, rows, axes, dwell, slack, T = bc.b1_radial()
    ticks, hits, counters = bc.host_bin(host, offsets, rows, axes, nsub)
    assert np.count_nonzero(dwell) == 6
    bc.b1_check(ticks, hits, dwell, slack, nsub, T, label="B1 radial")
    assert counters[3] == 0 and counters[2] == nsub * 7


# ---------------------------------------------------------------------------------------------- B2
@pytest.mark.parametrize("naxes", [1, 2, 3])
@pytest.mark.parametrize("kind", range(8))
def test_b2_every_kind_as_one_two_and_three_axes(host, kind, naxes):
    offsets, rows = bc.b2_rows()
    axes = bc.b2_axes(kind, naxes)
    bc.assert_clear_of_edges(offsets, rows, axes, 8)
    want = bc.reference(offsets, rows, axes, 8)
    got = bc.host_bin(host, offsets, rows, axes, 8)
    bc.assert_same(got, want, "B2 kind %d, %d axes" % (kind, naxes))
    bc.check_identities(*got, 8, offsets)
    assert got[2][2] > 0 and np.count_nonzero(got[1]) >= 2  # not vacuous: more than one cell is hit


@pytest.mark.parametrize("nsub", [1, 8, 64])
def test_b2_uneven_edges_and_every_nsub(host, nsub):
    offsets, rows = bc.b2_rows()
    axes = bc.b2_log_l()
    bc.assert_clear_of_edges(offsets, rows, axes, nsub)
    want = bc.reference(offsets, rows, axes, nsub)
    got = bc.host_bin(host, offsets, rows, axes, nsub)
    bc.assert_same(got, want, "B2 log L, nsub %d" % nsub)
    bc.check_identities(*got, nsub, offsets)
    assert np.count_nonzero(got[1]) >= 8


def test_b2_point_functions_against_numpy(host):
    rng = np.random.default_rng(2)
    x = rng.normal(size=(200, 3)) * 3.0 * bc.R_E
    for kind in range(8):
        got = np.array([host.bnh_coordinate(kind, np.ascontiguousarray(p).ctypes.data) for p in x])
        want = bc.coordinate(kind, x)
        if kind == bc.MLT:  # atan2 may differ in its last bit between two libraries
            assert np.all(np.abs(got - want) <= 1e-13 * 24.0)
        else:
            assert np.array_equal(got, want), kind
    e = np.array([-1.0, 0.0, 0.5, 3.0, 3.5])
    for c, want in ((-1.0, 0), (-1.5, -1), (0.0, 1), (-0.0, 1), (0.49, 1), (0.5, 2), (3.0, 3), (3.4999, 3), (3.5, -1), (9.0, -1),
                    (float("nan"), -1), (float("inf"), -1), (float("-inf"), -1)):
        assert host.bnh_find_cell(e.ctypes.data, 4, c) == want, c
    assert host.bnh_find_cell(e.ctypes.data, 1, -0.5) == 0 and host.bnh_find_cell(e.ctypes.data, 1, 0.0) == -1


# ---------------------------------------------------------------------------------------------- B3
def test_b3_samples_exactly_on_edges(host):
    ex = np.array([0.0, 1024.0, 2048.0, 4096.0])
    y = 8192.0
    pts = [((512.0, y, 0.0), (1536.0, y, 0.0)),      # the sample is x = 1024, an inner edge: the upper cell
           ((-512.0, y, 0.0), (512.0, y, 0.0)),       # x = 0 = edges[0]: cell 0
           ((3584.0, y, 0.0), (4608.0, y, 0.0)),      # x = 4096 = edges[n]: outside
           ((2048.0, y, 0.0), (2048.0, y, 64.0))]     # x = 2048 all along: cell 2
    offsets, rows = bc.b3_rows(pts)
    for k in range(4):
        o, r = bc.b3_rows(pts[k:k + 1])
        ticks, hits, counters = bc.host_bin(host, o, r, [(bc.X, ex)], 1)
        assert hits.tolist() == [[0, 1, 0], [1, 0, 0], [0, 0, 0], [0, 0, 1]][k], k
        assert counters.tolist() == [1, 0, 0 if k == 2 else 1, 1 if k == 2 else 0]
        assert ticks.sum() == (0 if k == 2 else 2 ** 30)  # one second in ticks of 2^-30 s
    got = bc.host_bin(host, offsets, rows, [(bc.X, ex)], 1)
    bc.assert_same(got, bc.reference(offsets, rows, [(bc.X, ex)], 1), "B3")
    assert got[1].tolist() == [1, 1, 1]
    # a one-cell grid, on each of three axes: only the ray whose sample is x = 4096 is outside
    one = [(bc.X, np.array([0.0, 4096.0])), (bc.Y, np.array([8192.0, 8193.0])), (bc.Z, np.array([0.0, 64.0]))]
    got = bc.host_bin(host, offsets, rows, one, 1)
    assert got[0].shape == (1,) and got[1].tolist() == [3] and got[2].tolist() == [4, 0, 3, 1]
    bc.assert_same(got, bc.reference(offsets, rows, one, 1), "B3 one cell")
    # a point on the z axis: outside for L (rho = 0), inside for r
    o, r = bc.b3_rows([((0.0, 0.0, 2.0 * 2 ** 23), (0.0, 0.0, 4.0 * 2 ** 23))])
    got = bc.host_bin(host, o, r, [(bc.L, np.array([1.0, 2.0, 1e300]))], 1)
    assert got[1].tolist() == [0, 0] and got[2].tolist() == [1, 0, 0, 1]
    got = bc.host_bin(host, o, r, [(bc.R, np.array([0.0, 3.0 * 2 ** 23, 5.0 * 2 ** 23]))], 1)
    assert got[1].tolist() == [0, 1] and got[2].tolist() == [1, 0, 1, 0]  # r = 3 * 2^23 exactly: the upper cell
    # the origin: outside for sinlat (r = 0)
    o, r = bc.b3_rows([((-64.0, 0.0, 0.0), (64.0, 0.0, 0.0))])
    got = bc.host_bin(host, o, r, [(bc.SINLAT, np.array([-1.0, 0.0, 1.0]))], 1)
    assert got[1].tolist() == [0, 0] and got[2].tolist() == [1, 0, 0, 1]


# ---------------------------------------------------------------------------------------------- B4
@pytest.mark.parametrize("name,col,value", [("nan_pos", 2, np.nan), ("inf_pos", 3, np.inf), ("nan_t", 0, np.nan), ("inf_t", 0, np.inf),
                                            ("nan_vgrel", 8, np.nan), ("inf_vgrel", 7, -np.inf)])
def test_b4_a_spoilt_row_skips_its_two_intervals(host, name, col, value):
    rays, axes = bc.b4_base()
    clean = bc.host_bin(host, *cc.pack(rays), axes, 4)
    assert clean[2].tolist()[:2] == [8, 0]
    rays[0] = rays[0].copy()
    rays[0][2, col] = value
    offsets, rows = cc.pack(rays)
    got = bc.host_bin(host, offsets, rows, axes, 4)
    bc.assert_same(got, bc.reference(offsets, rows, axes, 4), name)
    assert got[2].tolist()[:2] == [6, 2]
    # the other intervals are untouched: what is left is the clean map less the two intervals' own
    only = bc.host_bin(host, *cc.pack([bc.b4_base()[0][0][1:4]]), axes, 4)
    assert np.array_equal(got[0], clean[0] - only[0]) and np.array_equal(got[1], clean[1] - only[1])


def test_b4_nothing_from_nothing(host):
    rays, axes = bc.b4_base()
    r = rays[0].copy()
    r[1, 0] = r[0, 0]  # t1 == t0
    offsets, rows = cc.pack([r, rays[1]])
    got = bc.host_bin(host, offsets, rows, axes, 4)
    bc.assert_same(got, bc.reference(offsets, rows, axes, 4), "t1 == t0")
    assert got[2].tolist()[:2] == [7, 1]
    # one-row rays: no interval, not even between them
    offsets, rows = cc.pack([rays[0][:1], rays[0][1:2], rays[1][:1]])
    got = bc.host_bin(host, offsets, rows, axes, 4)
    assert not got[0].any() and not got[1].any() and got[2].tolist() == [0, 0, 0, 0]
    # an empty ray between two others
    offsets, rows = cc.pack([rays[0], np.zeros((0, 20)), rays[1]])
    got = bc.host_bin(host, offsets, rows, axes, 4)
    bc.assert_same(got, bc.host_bin(host, *cc.pack(rays), axes, 4), "empty ray")
    bc.assert_same(got, bc.reference(offsets, rows, axes, 4), "empty ray")
    # no rays at all
    got = bc.host_bin(host, np.zeros(1, dtype=np.int64), np.zeros((0, 20)), axes, 4)
    assert not got[0].any() and not got[1].any() and got[2].tolist() == [0, 0, 0, 0]


def test_b4_a_nan_weight_and_a_deposit_beyond_2_62_ticks(host):
    rays, axes = bc.b4_base()
    offsets, rows = cc.pack(rays)
    rw = np.ones(10)
    rw[2] = np.nan
    got = bc.host_bin(host, offsets, rows, axes, 4, row_weight=rw)
    bc.assert_same(got, bc.reference(offsets, rows, axes, 4, row_weight=rw), "NaN row weight")
    assert got[2].tolist()[:2] == [6, 2]
    only = bc.host_bin(host, *cc.pack([rays[0][1:4]]), axes, 4)
    clean = bc.host_bin(host, offsets, rows, axes, 4)
    assert np.array_equal(got[0], clean[0] - only[0]) and np.array_equal(got[1], clean[1] - only[1])
    yw = np.array([1.0, np.inf])
    got = bc.host_bin(host, offsets, rows, axes, 4, ray_weight=yw)
    assert got[2].tolist()[:2] == [4, 4]
    # 0.25 s / 4 / 2^-30 s = 2^26 ticks a sample: a weight of 2^36 is the first that is too much; only at ONE sample of an
    # interval (the weight rises along it) is enough to skip it whole
    for w, skipped in ((2.0 ** 36, 4), (2.0 ** 35.99, 0)):
        yw = np.array([1.0, w])
        got = bc.host_bin(host, offsets, rows, axes, 4, ray_weight=yw)
        bc.assert_same(got, bc.reference(offsets, rows, axes, 4, ray_weight=yw), "ray weight %g" % w)
        assert got[2].tolist()[:2] == [8 - skipped, skipped]
    rw = np.ones(10)
    rw[7] = 2.0 ** 37  # row 2 of ray 1: W at the sample nearest to it is (1 + 7/8 (2^37 - 1)) > 2^36
    got = bc.host_bin(host, offsets, rows, axes, 4, row_weight=rw)
    bc.assert_same(got, bc.reference(offsets, rows, axes, 4, row_weight=rw), "one heavy row")
    assert got[2].tolist()[:2] == [6, 2]
    bc.check_identities(*got, 4, offsets)


# ---------------------------------------------------------------------------------------------- B5, B6
def test_b5_weights(host):
    offsets, rows = bc.b2_rows()
    axes = bc.b2_log_l()
    bc.assert_clear_of_edges(offsets, rows, axes, 8)
    out = {}
    for name, (rw, yw) in bc.b5_weights(offsets).items():
        got = bc.host_bin(host, offsets, rows, axes, 8, row_weight=rw, ray_weight=yw)
        bc.assert_same(got, bc.reference(offsets, rows, axes, 8, row_weight=rw, ray_weight=yw), "B5 " + name)
        bc.check_identities(*got, 8, offsets)
        out[name] = got
    bc.assert_same(out["ones"], out["none"], "NULL weights are ones")
    assert np.array_equal(out["row"][1], out["none"][1]) and not np.array_equal(out["row"][0], out["none"][0])
    assert (out["negative_and_zero"][0] < 0).any()
    # linear in sigma: with w = t along a ray of constant spacing h, an interval's samples deposit h/nsub (t0 + sigma h)
    rays, axes1 = bc.b4_base()
    o, r = cc.pack(rays[:1])
    got = bc.host_bin(host, o, r, [(bc.R, np.array([0.0, 100.0 * bc.R_E]))], 8, row_weight=r[:, 0].copy())
    assert got[0][0] == 2 ** 29  # the integral of t dt over [0, 1] = 1/2 s, every deposit a whole number of ticks


def test_b6_additivity_and_permutation(host):
    offsets, rows = bc.b2_rows()
    axes = bc.b2_log_l()
    w = bc.b5_weights(offsets)["both"]
    whole = bc.host_bin(host, offsets, rows, axes, 8, row_weight=w[0], ray_weight=w[1])
    (o1, r1), (o2, r2) = bc.split_rays(offsets, rows, 4)
    k = int(offsets[4])
    acc = bc.host_bin(host, o1, r1, axes, 8, row_weight=w[0][:k], ray_weight=w[1][:4])
    acc = bc.host_bin(host, o2, r2, axes, 8, row_weight=w[0][k:], ray_weight=w[1][4:], into=acc)
    bc.assert_same(acc, whole, "two calls")
    perm = np.random.default_rng(4).permutation(len(offsets) - 1)
    o, r, rw, yw = bc.permute_rays(offsets, rows, perm, *w)
    bc.assert_same(bc.host_bin(host, o, r, axes, 8, row_weight=rw, ray_weight=yw), whole, "permuted")


# ---------------------------------------------------------------------------------------------- B7
@pytest.fixture(scope="module")
def oracle_rows(tmp_path_factory):
    """The oracle's adaptive trajectories of the 16 Appendix-B rays, packed: every row (outputper 1)."""
    from oracle import oracle
    from stanford_raytracer_amd import workloads as wl

    cfg = tmp_path_factory.mktemp("b7") / "newray.in"
    cfg.write_text(wl.NEWRAY_PLASMAPAUSE)
    pos, d, w = wl.appendix_b_rays()
    rows, nrows, stop, _ = oracle.Model.ngo(str(cfg)).trace(pos, d, w, capacity=2000, **cc.C5_TRACE)
    return cc.pack([rows[i, :nrows[i]] for i in range(len(w))])


def test_b7_the_oracles_rays(host, oracle_rows):
    offsets, rows = oracle_rows
    axes = bc.b7_r_axis()
    ticks, hits, counters = bc.host_bin(host, offsets, rows, axes, 8)
    assert counters[3] == 0 and counters[1] == 0
    T = sum(rows[offsets[r + 1] - 1, 0] - rows[offsets[r], 0] for r in range(len(offsets) - 1))
    err = abs(float(ticks.sum()) * bc.QUANTUM - T)
    bound = counters[2] * bc.QUANTUM / 2 + 1e-12 * T
    print("B7: %d rows, sum of ticks x quantum = %.9f s, sum of the rays' durations %.9f s, |difference| %.3g s, bound %.3g s"
          % (offsets[-1], float(ticks.sum()) * bc.QUANTUM, T, err, bound))
    assert err <= bound
    le, lat = bc.b7_map_axes()
    axes = [(bc.L, le), (bc.SINLAT, np.sin(lat))]
    bc.assert_clear_of_edges(offsets, rows, axes, 8)
    got = bc.host_bin(host, offsets, rows, axes, 8)
    bc.assert_same(got, bc.reference(offsets, rows, axes, 8), "B7 (L, maglat) 16 x 12")
    assert np.count_nonzero(got[1]) > 20


# ---------------------------------------------------------------------------------------------- B8: the C ABI without a GPU
def _refusals():
    from stanford_raytracer_amd import api

    ok = api.axis("x", [0.0, 1.0, 2.0])
    return [(dict(axes=[]), "naxes = 0"), (dict(axes=[ok] * 4), "naxes = 4"), (dict(axes=[ok], nsub=0), "nsub = 0"),
            (dict(axes=[ok], nsub=65), "nsub = 65"), (dict(axes=[(8, ok[1])]), "axis 0: unknown kind 8"),
            (dict(axes=[ok, (-1, ok[1])]), "axis 1: unknown kind -1"), (dict(axes=[(0, np.array([1.0]))]), "axis 0: n = 0"),
            (dict(axes=[(0, np.arange(1026.0))]), "axis 0: n = 1025"), (dict(axes=[(0, np.array([0.0, np.nan]))]), "edge 1 is not finite"),
            (dict(axes=[(0, np.array([0.0, np.inf]))]), "edge 1 is not finite"),
            (dict(axes=[(0, np.array([0.0, 1.0, 1.0]))]), "edges do not increase at edge 2"),
            (dict(axes=[(0, np.array([0.0, -1.0]))]), "edges do not increase at edge 1"),
            (dict(axes=[(6, np.array([-1.0, 0.0, 1.5]))]), "outside [-1, 1]"), (dict(axes=[(7, np.array([-0.5, 12.0]))]), "outside [0, 24]"),
            (dict(axes=[(7, np.array([0.0, 24.5]))]), "outside [0, 24]"), (dict(axes=[ok], quantum=0.0), "quantum"),
            (dict(axes=[ok], quantum=-1.0), "quantum"), (dict(axes=[ok], quantum=np.nan), "quantum"),
            (dict(axes=[ok], quantum=np.inf), "quantum")]  # (more than 2^31 - 1 cells: three axes of 1024 cells at most hold 2^30)


def test_b8_refusals_by_name_from_both_entry_points():
    from stanford_raytracer_amd import api

    L = api.lib()
    i64p = C.POINTER(C.c_int64)
    off = np.array([0, 2], dtype=np.int64)
    rows = np.zeros((2, 20))
    counters = np.zeros(4, dtype=np.int64)
    for kw, text in _refusals():
        p = api.bin_params(kw["axes"], kw.get("nsub", 8), kw.get("quantum", 2.0 ** -30))
        pt, ph = i64p(), i64p()
        rc = L.srt_bin_rays(C.byref(p), 1, off.ctypes.data_as(i64p), api._dp(rows), None, None, C.byref(pt), C.byref(ph), counters.ctypes.data_as(i64p))
        assert rc == api.SRT_EINVAL and text in L.srt_last_error().decode() and b"srt_bin_rays:" in L.srt_last_error(), (text, L.srt_last_error())
        # the device entry point says the same before it looks at any pointer
        rc = L.srt_bin_rays_device(C.byref(p), 1, None, None, None, None, None, None, None, None)
        assert rc == api.SRT_EINVAL and text in L.srt_last_error().decode() and b"srt_bin_rays_device:" in L.srt_last_error(), (text, L.srt_last_error())
        n = C.c_int64()
        assert L.srt_bin_cells(C.byref(p), C.byref(n)) == api.SRT_EINVAL and text in L.srt_last_error().decode()
    p = api.bin_params([api.axis("x", [0.0, 1.0])])  # (a null edges pointer cannot be made through bin_params)
    p.axis[0].edges = None
    n = C.c_int64()
    assert L.srt_bin_cells(C.byref(p), C.byref(n)) == api.SRT_EINVAL and b"axis 0: null edges" in L.srt_last_error()
    p = api.bin_params([api.axis("x", [0.0, 1.0, 2.0])])
    rc = L.srt_bin_rays(C.byref(p), 1, off.ctypes.data_as(i64p), api._dp(rows), None, None, None, None, counters.ctypes.data_as(i64p))
    assert rc == api.SRT_EINVAL and b"both outputs" in L.srt_last_error()
    rc = L.srt_bin_rays_device(C.byref(p), 1, None, None, None, None, None, None, None, None)
    assert rc == api.SRT_EINVAL and b"both outputs" in L.srt_last_error()
    pt, ph = i64p(), i64p()
    for bad, text in ((np.array([1, 2], dtype=np.int64), b"offsets[0] = 1"), (np.array([0, 3, 2], dtype=np.int64), b"offsets decrease at ray 1")):
        rc = L.srt_bin_rays(C.byref(p), len(bad) - 1, bad.ctypes.data_as(i64p), api._dp(np.zeros((3, 20))), None, None, C.byref(pt), C.byref(ph),
                            counters.ctypes.data_as(i64p))
        assert rc == api.SRT_EINVAL and text in L.srt_last_error()
    n = C.c_int64()
    assert L.srt_bin_cells(C.byref(api.bin_params([api.axis("L", np.arange(1.0, 9.0)), api.axis_maglat([-1.0, 0.0, 0.5, 1.0])])), C.byref(n)) == 0
    assert n.value == 21
    with pytest.raises(ValueError, match="unknown axis kind"):
        api.axis("lat", [0, 1])
    assert [api.axis(k, [0, 1])[0] for k in ("x", "y", "z", "r", "rho", "L", "sinlat", "mlt")] == list(range(8))
    k, e = api.axis_maglat([-0.5, 0.0, 0.25])
    assert k == 6 and np.array_equal(e, np.sin([-0.5, 0.0, 0.25]))


def test_b8_no_cpu_fallback():
    from stanford_raytracer_amd import api

    if api.lib().srt_init(0) == api.SRT_OK:
        pytest.skip("GPU present")
    offsets, rows = bc.b2_rows()
    axes = [api.axis("r", bc._edges(bc.R, 4))]
    with pytest.raises(api.SrtError, match="no HIP device"):
        api.bin_rays(offsets, rows, axes)
    with pytest.raises(api.SrtError, match="no HIP device"):
        api.bin_rays_padded(rows[:8].reshape(2, 4, 20), [4, 4], 1, axes, row_weight_padded=np.ones((2, 4)))


def test_b8_struct_layouts_match_the_header(tmp_path):
    from stanford_raytracer_amd import api

    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "srt.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu", '
                   'sizeof(srt_bin_axis), offsetof(srt_bin_axis, kind), offsetof(srt_bin_axis, n), offsetof(srt_bin_axis, edges), '
                   'sizeof(srt_bin_params), offsetof(srt_bin_params, naxes), offsetof(srt_bin_params, nsub), '
                   'offsetof(srt_bin_params, quantum), offsetof(srt_bin_params, axis)); return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    A, P = api.BinAxis, api.BinParams
    assert got == [C.sizeof(A), A.kind.offset, A.n.offset, A.edges.offset, C.sizeof(P), P.naxes.offset, P.nsub.offset, P.quantum.offset,
                   P.axis.offset]
    assert got[0] == C.sizeof(bc.CBinAxis) == 16 and got[4] == C.sizeof(bc.CBinParams) == 64


def test_b8_file_writer_against_a_parser_and_the_round_trip(tmp_path):
    from stanford_raytracer_amd import api

    rng = np.random.default_rng(9)
    axes = [api.axis("L", np.geomspace(1.0, 8.0, 6)), api.axis_maglat(np.deg2rad([-60.0, -10.0, 0.0, 45.0])), api.axis("mlt", [0.0, 6.5, 24.0])]
    ticks = rng.integers(-2 ** 40, 2 ** 62, size=(2, 3, 5), dtype=np.int64)
    hits = rng.integers(0, 2 ** 50, size=(2, 3, 5), dtype=np.int64)
    ticks[0, 0, 0], hits[0, 0, 0] = 0, 0
    q = 2.0 ** -20
    path = str(tmp_path / "map.txt")
    api.write_bin_file(path, axes, ticks, hits, nsub=5, quantum=q)

    def es24(v):
        mant, ex = ("%.15E" % v).split("E")
        return (mant + "E" + ex[0] + "%03d" % int(ex[1:])).rjust(24)

    lines = open(path).read().split("\n")
    assert lines[-1] == "" and len(lines) == 1 + 2 * 3 + 30 + 1
    assert lines[0] == "%10d%10d" % (3, 5) + es24(q)
    for a, (kind, e) in enumerate(axes):
        assert lines[1 + 2 * a] == "%10d%10d" % (kind, len(e) - 1)
        assert lines[2 + 2 * a] == "".join(es24(v) for v in e)
    for ln, t, h in zip(lines[7:], ticks.ravel(), hits.ravel()):
        assert ln == es24(float(t) * q) + "%20d" % h
    back = api.read_bin_file(path)
    assert back["nsub"] == 5 and back["quantum"] == q and [k for k, _ in back["axes"]] == [5, 6, 7]
    for (_, e), (_, f) in zip(axes, back["axes"]):
        assert np.allclose(f, e, rtol=6e-16, atol=0)
    assert back["sum"].shape == (2, 3, 5) and np.array_equal(back["hits"], hits)
    assert np.array_equal(back["sum"], np.array([float("%.15e" % (float(t) * q)) for t in ticks.ravel()]).reshape(2, 3, 5))
    # a second write of what was read gives the same bytes where ticks fit a double: hits only here
    api.write_bin_file(str(tmp_path / "hits.txt"), axes, None, hits, nsub=5, quantum=q)
    assert np.array_equal(api.read_bin_file(str(tmp_path / "hits.txt"))["hits"], hits)
    assert not api.read_bin_file(str(tmp_path / "hits.txt"))["sum"].any()
    # a cut file, and one with a record too many, are refused by name
    text = open(path).read()
    cut = tmp_path / "cut.txt"
    cut.write_text(text[:len(text) - 45])
    with pytest.raises(api.SrtError, match="announces 30 cells"):
        api.read_bin_file(str(cut))
    cut.write_text("\n".join(lines[:4]) + "\n")
    with pytest.raises(api.SrtError, match="cut short"):
        api.read_bin_file(str(cut))
    cut.write_text(text + lines[-2] + "\n")
    with pytest.raises(api.SrtError, match="announces 30 cells"):
        api.read_bin_file(str(cut))
    with pytest.raises(ValueError, match="holds 29 cells"):
        api.write_bin_file(path, axes, ticks.ravel()[:29], None, nsub=5, quantum=q)
    with pytest.raises(api.SrtError, match="nsub = 0"):
        api.write_bin_file(path, axes, ticks, hits, nsub=0)
