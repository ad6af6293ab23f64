"""CPU: ray-tube sections along kept rows (include/srt.h, "ray tubes") -- csrc/srt_tubes.hpp's point functions, the very source the
device compiles, built for the host (tests/native/tubes_host.cpp) and held against the numpy restatement and the truths of
tests/tubes_cases.py (T1 .. T6, T8; bars in its docstring); the refusals and the file writer of the C ABI (T7).

The host build gives the restatement's bits in every case; that is asserted.  T6 is measured with this host build on the oracle's
own fixed-step trajectories; the figures are printed by the test and recorded in profiles/tubes/."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import tubes_cases as tc
from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "tubes_host.cpp")
FLAGS = ["-x", "hip", "--cuda-host-only", "-ffp-contract=off", "-O2", "-std=c++17"]


def _hipcc():
    return shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("tbh") / "libtbh.so")
    subprocess.check_call([_hipcc()] + FLAGS + ["-shared", "-fPIC", "-o", so, SRC])
    L = C.CDLL(so)
    L.tbh_tubes.argtypes = [C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
    L.tbh_row_at_or_before.argtypes = [C.c_void_p, C.c_longlong, C.c_double]
    L.tbh_row_at_or_before.restype = C.c_longlong
    return L


def host_tubes(L, offsets, rows, nb):
    """-> section[total, 4], flag[total]; a refusal raises ValueError with the reason"""
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    rows = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, tc.ROW)
    nb = np.ascontiguousarray(nb, dtype=np.int64).reshape(-1, 2)
    total = int(offsets[-1])
    section, flag = np.full((total + 1, 4), -7.0), np.full(total + 1, -7, dtype=np.int32)
    why = C.create_string_buffer(200)
    pad = nb if len(nb) else np.zeros((1, 2), dtype=np.int64)
    rc = L.tbh_tubes(len(offsets) - 1, pad.ctypes.data, offsets.ctypes.data, rows.ctypes.data, section.ctypes.data, flag.ctypes.data, why, 200)
    if rc:
        raise ValueError(why.value.decode())
    assert np.all(section[total] == -7.0) and flag[total] == -7  # nothing is written beyond the rows
    return section[:total], flag[:total]


def host_and_reference(L, offsets, rows, nb, label):
    section, flag = host_tubes(L, offsets, rows, nb)
    tc.assert_same_bits(section, flag, *tc.reference(offsets, rows, nb), label=label)
    return section, flag


def test_t1_straight_rays_from_a_common_apex(host):
    offsets, rows, nb, vel = tc.t1_case()
    section, flag = host_and_reference(host, offsets, rows, nb, "T1 host")
    truth, geom = tc.t1_truth(offsets, rows, nb, vel)
    centre = np.nonzero(np.isfinite(truth[:, 3]))[0]
    widths = geom[centre, 1] / 2
    assert widths.min() < 1.5e3 and widths.max() > 0.9e6 and np.linalg.norm(rows[centre, 1:4], axis=1).max() > 1e7
    assert int(np.sum(flag == 0)) == len(centre) == sum(r[0] for r in tc.T1_ROWS)
    tc.check_against_truth(section, flag, truth, geom, tc.K_STRAIGHT, "T1 straight rays, host")


def test_t2_cubic_arcs_against_the_polynomials(host):
    offsets, rows, nb = tc.t2_case()
    section, flag = host_and_reference(host, offsets, rows, nb, "T2 host")
    truth, geom = tc.t2_truth(offsets, rows, nb)
    assert int(np.sum(flag == 0)) == sum(tc.T2_COUNTS)
    tc.check_against_truth(section, flag, truth, geom, tc.K_CUBIC, "T2 cubic arcs, host")
    # the chords miss the same truth by far more than the bar: the bar sees the interpolant
    chord, _ = tc.reference(offsets, rows, nb, chord=True)
    inner = np.nonzero((flag == 0) & ~np.isin(rows[:, 0], [0.0, 1.0]))[0]
    err = np.linalg.norm(chord[inner, :3] - truth[inner, :3], axis=1)
    assert np.all(err > 1e3 * tc.K_CUBIC * 2.0 ** -52 * geom[inner, 0] * geom[inner, 1])


def test_t3_exact_cases(host):
    for k in (0, 7, 40):
        offsets, rows, nb, want, wflag = tc.t3_case(k)
        section, flag = host_and_reference(host, offsets, rows, nb, "T3 host")
        assert np.array_equal(flag, wflag)
        assert np.array_equal(section[:3], want[:3]) and np.all(np.isnan(section[3:]))  # (row 2: the neighbours' last rows, exactly)
        o2, r2, nb2, want2, _ = tc.t3_case(k, swap=True)
        swapped, flag2 = host_and_reference(host, o2, r2, nb2, "T3 host, swapped")
        assert np.array_equal(flag2, wflag) and np.array_equal(swapped[:3], -section[:3]) and np.array_equal(swapped[:3], want2[:3])
    for shift, want in ((0, tc.OK), (-1, tc.NO_ROW), (1, tc.NO_ROW)):
        offsets, rows, nb, wflag = tc.t3_one_row_neighbour(shift)
        section, flag = host_and_reference(host, offsets, rows, nb, "T3 host, one-row neighbour")
        assert flag[0] == wflag == want
        if shift == 0:  # b = (4, 1, 2), c = (-1, 6, 20 + t - 16 = 4 at t = 1) from the centre
            assert section[0].tolist() == [0.5 * (1 * 4 - 2 * 6), 0.5 * (2 * -1 - 4 * 4), 0.5 * (4 * 6 + 1), 12.5]


@pytest.mark.parametrize("name", sorted(tc.t4_cases()))
def test_t4_flags_one_at_a_time_and_their_order(host, name):
    offsets, rows, nb, want = tc.t4_cases()[name]
    section, flag = host_and_reference(host, offsets, rows, nb, "T4 host, " + name)
    n0 = int(offsets[1]) if len(offsets) > 1 else 0
    if want is not None:
        assert flag[:n0].tolist() == want, (name, flag[:n0].tolist())
    else:  # the bad value sits where the search reads: the rows it spoils are few, and the others are whole
        assert tc.UNUSABLE in flag[:n0].tolist() and flag[:n0].tolist().count(0) >= 2, flag[:n0].tolist()
    assert np.all(flag[n0:] == tc.NO_TUBE)
    ok, novg = flag == tc.OK, flag == tc.NO_VG
    assert np.all(np.isfinite(section[ok])) and np.all(np.isnan(section[~ok & ~novg]))
    assert np.all(np.isfinite(section[novg, :3])) and np.all(np.isnan(section[novg, 3]))
    if name.startswith("centre_vg"):  # Sigma is what the untouched case gives
        base = host_tubes(host, *tc.t4_cases()["ok"][:3])[0]
        assert np.array_equal(section[1, :3], base[1, :3])


def test_t4_the_search_is_the_definitions(host):
    rng = np.random.default_rng(5)
    for n in (0, 1, 2, 3, 64, 1025):
        rows = np.zeros((max(n, 1), tc.ROW))
        for trial in range(3):
            times = np.sort(rng.uniform(0, 1, n)) if trial < 2 else rng.uniform(0, 1, n)  # (the last: no order at all)
            if trial == 1 and n > 2:
                times[n // 2] = np.nan
            rows[:n, 0] = times
            for t in list(times[:8]) + [-1.0, 0.5, 2.0, np.nextafter(times[0], 2.0) if n else 0.0]:
                assert host.tbh_row_at_or_before(rows.ctypes.data, n, float(t)) == tc.search(times, t), (n, trial, t)


@pytest.mark.parametrize("total", tc.T5_TOTALS)
def test_t5_launch_shapes(host, total):
    for name, (lens, nb) in tc.t5_layouts(total).items():
        offsets, rows = tc.fan(lens, seed=total)
        section, flag = host_and_reference(host, offsets, rows, nb, "T5 host %d rows, %s" % (total, name))
        if total >= 63:
            assert np.any(flag == tc.OK), name


def test_t5_search_depth_distinct_neighbours_and_permutation(host):
    # a neighbour of 1 row and one of 1025 rows
    offsets, rows = tc.fan([40, 1, 1025], seed=3)
    nb = np.array([[2, 1], [-1, -1], [0, 1]], dtype=np.int64)
    section, flag = host_and_reference(host, offsets, rows, nb, "T5 host, 1 and 1025 rows")
    assert set(flag[:40].tolist()) == {tc.NO_ROW} and np.sum(flag[41:] == tc.NO_ROW) >= 1000  # (the one-row ray's time is no one else's)
    offsets, rows = tc.fan([40, 1025, 300], seed=4)
    section, flag = host_and_reference(host, offsets, rows, tc.ring(3), "T5 host, 1025 rows")
    assert np.all(flag == tc.OK)
    # a wave whose lanes' neighbours are all different rays: 130 rays of one row at one time
    offsets, rows = tc.fan([1] * 130, seed=5, shared_time=True)
    section, flag = host_and_reference(host, offsets, rows, tc.ring(130), "T5 host, rays of one row")
    assert np.all(flag == tc.OK)
    # a permutation of the rays, the table permuted to match, gives the permuted output bit for bit
    lens = [5, 0, 9, 3, 1, 17, 8, 2, 30, 4]
    offsets, rows = tc.fan(lens, seed=6)
    nb = tc.ring(len(lens))
    nb[4] = -1
    section, flag = host_and_reference(host, offsets, rows, nb, "T5 host, before the permutation")
    perm = np.random.default_rng(9).permutation(len(lens))
    o2, r2, nb2, src = tc.permuted(offsets, rows, nb, perm)
    s2, f2 = host_and_reference(host, o2, r2, nb2, "T5 host, permuted")
    tc.assert_same_bits(s2, f2, section[src], flag[src], "T5 host, permutation")
    assert np.any(flag == tc.OK) and np.any(flag == tc.NO_ROW)


# ---------------------------------------------------------------------------------------------- T6: real trajectories
@pytest.fixture(scope="module")
def oracle_fan(tmp_path_factory):
    """The oracle's fixed-step trajectories of the 16 Appendix-B rays and their companions (api.tube_fan, 50 km), packed: every
    row (outputper 1), so that all 48 rays share their time stamps."""
    from oracle import oracle
    from stanford_raytracer_amd import api, workloads as wl

    cfg = tmp_path_factory.mktemp("t6") / "newray.in"
    cfg.write_text(wl.NEWRAY_PLASMAPAUSE)
    pos, d, w, nb = api.tube_fan(*wl.appendix_b_rays(), delta_pos=tc.T6_DELTA_POS)
    rows, nrows, stop, _ = oracle.Model.ngo(str(cfg)).trace(pos, d, w, capacity=tc.T6_TRACE["maxsteps"] + 1, **tc.T6_TRACE)
    return tc.pack([rows[i, :nrows[i]] for i in range(len(w))]) + (nb,)


def test_t6_hermite_beats_chords_on_the_oracles_trajectories(host, oracle_fan):
    offsets, rows, nb = oracle_fan
    truth, flag_full = host_and_reference(host, offsets, rows, nb, "T6 host, all rows")
    # all rays share their time stamps: every lookup is a node hit, and a centre row is out only beyond a neighbour's end
    for a in range(0, len(nb), 3):
        n = min(int(offsets[r + 1] - offsets[r]) for r in (a, a + 1, a + 2))
        assert np.all(flag_full[offsets[a]:offsets[a] + n] == tc.OK)
        assert np.array_equal(rows[offsets[a]:offsets[a] + n, 0], rows[offsets[a + 1]:offsets[a + 1] + n, 0])
    o4, r4, kept = tc.t6_thin(offsets, rows, nb)
    herm, flag_h = host_and_reference(host, o4, r4, nb, "T6 host, thinned")
    chord, flag_c = tc.reference(o4, r4, nb, chord=True)
    fig = tc.t6_figures(offsets, nb, truth, flag_full, kept, o4, herm, flag_h, chord, flag_c)
    print(tc.t6_report(fig, "T6 host build, oracle rows (%d .. %d per ray), %g km, centres keep rows 0 mod 4, b 1 mod 4, c 2 mod 4"
                       % (np.diff(offsets).min(), np.diff(offsets).max(), tc.T6_DELTA_POS / 1e3)))
    tc.t6_assert(fig)


# ---------------------------------------------------------------------------------------------- T7: the C ABI without a GPU
def _call(nb, offsets=(0, 2, 4, 6), rows=None, outputs=True, device=False):
    from stanford_raytracer_amd import api

    L = api.lib()
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    rows = np.zeros((max(int(off[-1]), 1), 20)) if rows is None else rows
    total = max(int(off[-1]), 1)
    section, flag = np.zeros((total, 4)), np.zeros(total, dtype=np.int32)
    i64p = C.POINTER(C.c_int64)
    pnb = None if nb is None else np.ascontiguousarray(nb, dtype=np.int64).ctypes.data_as(i64p)
    if device:  # (host addresses: whatever is refused here is refused before a pointer is looked at)
        rc = L.srt_tubes_device(len(off) - 1, pnb, off.ctypes.data, rows.ctypes.data, section.ctypes.data if outputs else None,
                                flag.ctypes.data if outputs else None, None)
    else:
        rc = L.srt_tubes(len(off) - 1, pnb, off.ctypes.data_as(i64p), api._dp(rows), api._dp(section) if outputs else None,
                         flag.ctypes.data_as(api.ip) if outputs else None)
    return rc, (L.srt_last_error() or b"").decode()


T7_REFUSALS = [(None, "null neighbours"),
               ([[1, -1], [-1, -1], [-1, -1]], "ray 0: neighbours 1, -1: one of a pair is -1"),
               ([[-1, 2], [-1, -1], [-1, -1]], "ray 0: neighbours -1, 2: one of a pair is -1"),
               ([[-1, -1], [0, 3], [-1, -1]], "ray 1: neighbours 0, 3: an index outside 0 .. nrays - 1 = 2"),
               ([[-1, -1], [-2, 0], [-1, -1]], "ray 1: neighbours -2, 0: an index outside"),
               ([[1, 1], [-1, -1], [-1, -1]], "ray 0: neighbours 1, 1: a tube takes three different rays"),
               ([[-1, -1], [-1, -1], [2, 1]], "ray 2: neighbours 2, 1: a tube takes three different rays"),
               ([[1, 0], [-1, -1], [-1, -1]], "ray 0: neighbours 1, 0: a tube takes three different rays")]


@pytest.mark.parametrize("device", [False, True])
def test_t7_refusals_by_name_before_the_device(device):
    from stanford_raytracer_amd import api

    who = "srt_tubes_device: " if device else "srt_tubes: "
    for nb, text in T7_REFUSALS:
        rc, msg = _call(nb, device=device)
        assert rc == api.SRT_EINVAL and msg.startswith(who) and text in msg, (text, msg)
    ok = [[1, 2], [-1, -1], [-1, -1]]
    rc, msg = _call(ok, outputs=False, device=device)
    assert rc == api.SRT_EINVAL and "both outputs" in msg, msg
    if not device:
        rc, msg = _call(ok, offsets=(0, 2, 1, 6))
        assert rc == api.SRT_EINVAL and "offsets decrease at ray 1" in msg, msg
        rc, msg = _call(ok, offsets=(1, 2, 4, 6))
        assert rc == api.SRT_EINVAL and "offsets[0] = 1" in msg, msg
    with pytest.raises(ValueError, match="2 pairs for 3 rays"):
        api.tubes([0, 2, 4, 6], np.zeros((6, 20)), [[1, 2], [-1, -1]])


def test_t7_a_valid_call_without_a_gpu_fails_with_no_hip_device():
    import torch

    from stanford_raytracer_amd import api

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    offsets, rows, nb, _ = tc.t1_case()
    with pytest.raises(api.SrtError, match="no HIP device"):
        api.tubes(offsets, rows, nb)


def test_t7_the_file_by_field_widths(host, tmp_path):
    from stanford_raytracer_amd import api

    r = [x.copy() for x in tc.t4_base()]
    r[0][1, 7:10] = 0.0      # flag 5: Sigma and a NaN
    r[0][3, 2] = np.nan      # flag 2: four NaN
    offsets, rows = tc.pack(r + [r[0][:2]])
    nb = np.array([[1, 2], [-1, -1], [-1, -1], [0, 1]], dtype=np.int64)
    section, flag = host_tubes(host, offsets, rows, nb)
    assert {0, 1, 2, 5} <= set(flag.tolist())
    raynum = np.array([7, 8, 9, 1234567890], dtype=np.int64)
    path = str(tmp_path / "tubes.txt")
    api.write_tubes_file(path, raynum, offsets, rows, section, flag)
    got = tc.parse_tubes_file(path)
    want = [(int(raynum[a]), j - int(offsets[a]) + 1, int(flag[j]), [rows[j, 0]] + section[j].tolist())
            for a in range(4) for j in range(int(offsets[a]), int(offsets[a + 1])) if flag[j] != 1]
    assert len(got) == len(want) == int(np.sum(flag != 1))
    for g, w in zip(got, want):
        assert g[:3] == w[:3]
        assert all((np.isnan(a) and np.isnan(b)) or a == tc.es24(b) for a, b in zip(g[3], w[3])), (g, w)
    assert any(np.isnan(g[3][4]) and not np.isnan(g[3][1]) for g in got) and any(np.isnan(g[3][1]) for g in got)
    text = open(path).read()
    assert text.count("NaN") == int(np.sum(flag == 5)) + 4 * int(np.sum((flag >= 2) & (flag <= 4))) >= 5
    # a ray number beyond i10 is refused, and so are offsets that decrease
    with pytest.raises(api.SrtError, match="does not fit the record's i10 field"):
        api.write_tubes_file(path, [7, 8, 9, 10 ** 10], offsets, rows, section, flag)
    with pytest.raises(api.SrtError, match="does not fit the record's i10 field"):
        api.write_tubes_file(path, [7, -8, 9, 10], offsets, rows, section, flag)
    bad = offsets.copy()
    bad[1], bad[2] = bad[2], bad[1]
    with pytest.raises(api.SrtError, match="offsets decrease"):
        api.write_tubes_file(path, raynum, bad, rows, section, flag)
    # no rows, no records
    api.write_tubes_file(path, np.zeros(0, dtype=np.int64), [0], np.zeros((0, 20)), np.zeros((0, 4)), np.zeros(0, dtype=np.int32))
    assert open(path).read() == ""


# ---------------------------------------------------------------------------------------------- T8: api.tube_fan
def test_t8_the_frame_of_tube_fan():
    from stanford_raytracer_amd import api

    rng = np.random.default_rng(2)
    dirs = np.concatenate([np.eye(3), -np.eye(3), rng.normal(size=(200, 3)) * rng.uniform(0.1, 10, (200, 1)),
                           [[1.0, 1.0, 1.0], [1e-9, 1.0, 0.0], [0.5, -0.5, 0.5]]])
    u, v = api.tube_frame(dirs)
    d = dirs / np.linalg.norm(dirs, axis=1)[:, None]
    for a, b in ((u, u), (v, v)):
        assert np.all(np.abs((a * b).sum(axis=1) - 1.0) <= 1e-15)
    for a, b in ((u, v), (u, d), (v, d)):
        assert np.all(np.abs((a * b).sum(axis=1)) <= 1e-15)
    assert np.all(np.linalg.norm(np.cross(u, v) - d, axis=1) <= 4e-15)
    u2, v2 = api.tube_frame(dirs)
    assert np.array_equal(u, u2) and np.array_equal(v, v2)  # deterministic
    with pytest.raises(ValueError, match="delta_pos"):
        api.tube_fan(np.zeros((1, 3)), np.ones((1, 3)), np.ones(1))
    # the layout: each ray, then its two companions
    pos0, dir0, w0 = rng.normal(size=(5, 3)) * 1e7, rng.normal(size=(5, 3)), np.arange(5) + 1.0
    pos, dr, w, nb = api.tube_fan(pos0, dir0, w0, delta_angle=1e-3)
    assert pos.shape == dr.shape == (15, 3) and np.array_equal(pos[0::3], pos0) and np.array_equal(pos[1::3], pos0) and np.array_equal(dr[0::3], dir0)
    assert np.array_equal(w, np.repeat(w0, 3)) and nb.dtype == np.int64
    assert nb.tolist() == [[3 * (k // 3) + 1, 3 * (k // 3) + 2] if k % 3 == 0 else [-1, -1] for k in range(15)]
    cosang = (dr[1::3] * dir0).sum(axis=1) / np.linalg.norm(dr[1::3], axis=1) / np.linalg.norm(dir0, axis=1)
    assert np.allclose(np.arccos(cosang), 1e-3, rtol=1e-6) and np.allclose(np.linalg.norm(dr[2::3], axis=1), np.linalg.norm(dir0, axis=1))


def test_t8_the_section_of_a_fan_at_launch(host):
    from stanford_raytracer_amd import api

    rng = np.random.default_rng(3)
    n, delta = 24, 50e3
    dir0 = np.concatenate([np.eye(3), rng.normal(size=(n - 3, 3))])
    pos0 = rng.normal(size=(n, 3)) * 0.8e7
    pos, dr, w, nb = api.tube_fan(pos0, dir0, np.ones(n), delta_pos=delta)
    rows = np.zeros((3 * n, tc.ROW))
    rows[:, 1:4] = pos
    rows[:, 7:10] = 0.3 * dr / np.linalg.norm(dr, axis=1)[:, None]
    offsets = np.arange(3 * n + 1, dtype=np.int64)
    section, flag = host_and_reference(host, offsets, rows, nb, "T8 host")
    d = dir0 / np.linalg.norm(dir0, axis=1)[:, None]
    truth = np.full((3 * n, 4), np.nan)
    truth[0::3, :3] = 0.5 * delta * delta * d
    truth[0::3, 3] = 0.5 * delta * delta
    geom = np.zeros((3 * n, 2))
    geom[0::3, 0] = np.linalg.norm(pos0, axis=1) + delta
    geom[0::3, 1] = 2 * delta
    # the frame is unit and perpendicular to 1e-15, which moves Sigma by up to 3e-15 |Sigma|: 14 2^-52 |Sigma| on top of the bar
    rowsel = np.arange(0, 3 * n, 3)
    err = np.linalg.norm(section[rowsel, :3] - truth[rowsel, :3], axis=1)
    bar = tc.K_STRAIGHT * 2.0 ** -52 * geom[rowsel, 0] * geom[rowsel, 1] + 14 * 2.0 ** -52 * 0.5 * delta * delta
    print("T8 host: |Sigma - 1/2 delta^2 dir0| / bar max %.3g" % (err / bar).max())
    assert np.all(flag[rowsel] == 0) and np.all(err <= bar) and np.all(np.abs(section[rowsel, 3] - truth[rowsel, 3]) <= bar)
