"""CPU: surface crossings along kept rows (include/srt.h) -- csrc/srt_crossings.hpp's point functions, the very source the device
compiles, built for the host (tests/native/crossings_host.cpp) and held against the numpy restatement and the exact truths of
tests/crossings_cases.py (C1 .. C5, bars in its docstring); the refusals, the struct layout and the file writer of the C ABI (C6).

C5, measured with this host build on the oracle's own trajectories (16 Appendix-B rays, NEWRAY_PLASMAPAUSE, adaptive, tmax 2,
maxsteps 2000, del 1e-4): the figures are printed by the test and recorded in profiles/crossings/."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import crossings_cases as cc
from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "crossings_host.cpp")
FLAGS = ["-x", "hip", "--cuda-host-only", "-ffp-contract=off", "-O2", "-std=c++17"]


def _hipcc():
    return shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


class CSurface(C.Structure):  # the test's own mirror of srt_surface (api.Surface is checked against gcc below)
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("p", C.c_double * 4)]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("cxh")
    so = str(d / "libcxh.so")
    subprocess.check_call([_hipcc()] + FLAGS + ["-shared", "-fPIC", "-o", so, SRC])
    L = C.CDLL(so)
    L.cxh_crossings.argtypes = [C.c_int, C.POINTER(CSurface), C.c_longlong, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p,
                                C.c_void_p, C.POINTER(C.c_longlong), C.c_char_p, C.c_int]
    L.cxh_light_speed.restype = C.c_double
    return L


def host_crossings(L, offsets, rows, surfaces, capacity=None):
    """-> (event_rows[min(count, capacity), 20], meta[.., 4], count)"""
    arr = (CSurface * max(len(surfaces), 1))()
    for i, (kind, p) in enumerate(surfaces):
        arr[i] = CSurface(kind, 0, (C.c_double * 4)(*[float(v) for v in p]))
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    why = C.create_string_buffer(200)
    count = C.c_longlong()
    n = len(offsets) - 1
    if capacity is None:
        assert L.cxh_crossings(len(surfaces), arr, n, offsets.ctypes.data, rows.ctypes.data, 0, None, None, C.byref(count), why, 200) == 0, why.value
        capacity = count.value
    ev = np.full((max(capacity, 1), cc.ROW), -7.0)
    meta = np.full((max(capacity, 1), 4), -7, dtype=np.int32)
    rc = L.cxh_crossings(len(surfaces), arr, n, offsets.ctypes.data, rows.ctypes.data, capacity, ev.ctypes.data, meta.ctypes.data,
                         C.byref(count), why, 200)
    assert rc == 0, why.value
    k = min(count.value, capacity)
    assert np.all(ev[k:] == -7.0) and np.all(meta[k:] == -7)  # nothing is written beyond the events kept
    return ev[:k], meta[:k], count.value


def test_the_speed_of_light_is_the_librarys(host):
    assert host.cxh_light_speed() == cc.C_LIGHT


def test_c1_exact_cubics_every_kind_both_directions(host):
    offsets, rows, surfaces = cc.c1_case()
    ev, meta, count = host_crossings(host, offsets, rows, surfaces)
    assert count == len(meta) > 0
    cc.check_against_reference(offsets, rows, surfaces, ev, meta, "C1 host")
    for si, (kind, _) in enumerate(surfaces):  # every kind, in both directions
        assert {1, -1} <= set(meta[meta[:, 1] == si, 3].tolist()), (si, kind)
    # planes: the crossing time is a root of a cubic, which owes nothing to the interpolant
    idx, sig_true = cc.c1_plane_truth(offsets, rows, surfaces, meta)
    assert len(idx) >= 8
    sig = cc.sigma_of(offsets, rows, ev, meta)[idx]
    print("C1 host: %d plane events against numpy.roots, sigma error max %.3g" % (len(idx), np.abs(sig - sig_true).max()))
    assert np.all(np.abs(sig - sig_true) <= cc.SIGMA_BAR)


def test_c2_a_row_on_the_surface_gives_one_event_per_pass(host):
    offsets, rows, surfaces = cc.c2_case()
    ev, meta, count = host_crossings(host, offsets, rows, surfaces)
    assert meta.tolist() == [[0, 0, 0, 1], [1, 0, 1, -1]]
    sig = cc.sigma_of(offsets, rows, ev, meta)
    print("C2 host: sigma* = 1 - %.3g and %.3g" % (1.0 - sig[0], sig[1]))
    assert abs(sig[0] - 1.0) <= cc.SIGMA_BAR and abs(sig[1]) <= cc.SIGMA_BAR
    cc.check_against_reference(offsets, rows, surfaces, ev, meta, "C2 host")


@pytest.mark.parametrize("name", sorted(cc.c3_cases()))
def test_c3_no_events(host, name):
    offsets, rows, surfaces = cc.c3_cases()[name]
    ev, meta, count = host_crossings(host, offsets, rows, surfaces)
    assert count == 0 and len(cc.reference(offsets, rows, surfaces)) == 0
    if name.startswith(("nan", "inf", "t1")):  # the case is not empty for another reason: the unspoilt rows have events
        base = cc.rows_on_cubic(cc.C1_COEF, np.array([0.0, 1.0]))
        assert host_crossings(host, offsets, base, surfaces)[2] == 2


def test_c3_an_empty_ray_between_two_others(host):
    offsets, rows, surfaces = cc.c3_empty_between()
    ev, meta, count = host_crossings(host, offsets, rows, surfaces)
    assert set(meta[:, 0].tolist()) == {0, 2}
    cc.check_against_reference(offsets, rows, surfaces, ev, meta, "C3 empty ray")


@pytest.mark.parametrize("nsurf", [1, 16])
def test_c4_order_counts_and_capacity(host, nsurf):
    offsets, rows, surfaces = cc.c4_case(nsurf)
    ev, meta, count = host_crossings(host, offsets, rows, surfaces)
    cc.check_against_reference(offsets, rows, surfaces, ev, meta, "C4 host, %d surfaces" % nsurf)
    keys = [(m[0], m[2], m[1]) for m in meta.tolist()]
    assert keys == sorted(keys) and len(set(keys)) == len(keys) and count >= 3
    if nsurf == 16:  # the identical surfaces 3 and 11 give identical events
        a, b = meta[:, 1] == 3, meta[:, 1] == 11
        assert a.sum() == b.sum() > 0 and np.array_equal(ev[a], ev[b]) and np.array_equal(meta[a][:, [0, 2, 3]], meta[b][:, [0, 2, 3]])
    for cap in (0, 1, count // 2, count - 1):
        e2, m2, c2 = host_crossings(host, offsets, rows, surfaces, capacity=cap)
        assert c2 == count and len(m2) == cap and np.array_equal(m2, meta[:cap]) and np.array_equal(e2, ev[:cap])


def test_the_program_prints_what_the_function_returns(host, tmp_path):
    offsets, rows, surfaces = cc.c4_case(1)
    ev, meta, count = host_crossings(host, offsets, rows, surfaces)
    exe = str(tmp_path / "crossings_host")
    subprocess.check_call([_hipcc()] + FLAGS + ["-o", exe, SRC])
    text = "%d %d %d\n" % (len(surfaces), len(offsets) - 1, count)
    text += "".join("%d %s\n" % (k, " ".join("%.17g" % v for v in p)) for k, p in surfaces)
    text += " ".join(str(int(o)) for o in offsets) + "\n" + " ".join("%.17g" % v for v in rows.ravel()) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert int(out[0]) == count
    got = np.array([[float(v) for v in ln.split()] for ln in out[1:]])
    assert np.array_equal(got[:, :4].astype(np.int32), meta) and np.array_equal(got[:, 4:], ev)


@pytest.fixture(scope="module")
def oracle_rows(tmp_path_factory):
    """The oracle's adaptive trajectories of the 16 Appendix-B rays, packed: every row (outputper 1)."""
    from oracle import oracle
    from stanford_raytracer_amd import workloads as wl

    cfg = tmp_path_factory.mktemp("c5") / "newray.in"
    cfg.write_text(wl.NEWRAY_PLASMAPAUSE)
    pos, d, w = wl.appendix_b_rays()
    rows, nrows, stop, _ = oracle.Model.ngo(str(cfg)).trace(pos, d, w, capacity=2000, **cc.C5_TRACE)
    return cc.pack([rows[i, :nrows[i]] for i in range(len(w))])


def test_c5_hermite_beats_linear_on_the_oracles_trajectories(host, oracle_rows):
    offsets, rows = oracle_rows
    surf = cc.c5_surfaces()
    full = host_crossings(host, offsets, rows, surf)[:2]
    o4, r4 = cc.thin(offsets, rows, 4)
    herm = host_crossings(host, o4, r4, surf)[:2]
    lin = cc.ref_arrays(cc.reference(o4, r4, surf, linear=True))[:2]
    fig = cc.c5_figures(full, herm, lin)
    print(cc.c5_report(fig, "C5 host build, oracle rows (%d .. %d per ray), every 4th kept" % (np.diff(offsets).min(), np.diff(offsets).max())))
    cc.c5_assert(fig)


# ---------------------------------------------------------------------------------------------- C6: the C ABI without a GPU
def _call(surfaces, offsets=(0, 2), rows=None):
    from stanford_raytracer_amd import api

    L = api.lib()
    arr, ns = api.surface_array(surfaces) if not isinstance(surfaces, tuple) else surfaces
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    rows = np.zeros((max(int(off[-1]), 1), 20)) if rows is None else rows
    n, pe, pm = C.c_int64(), api.dp(), api.ip()
    rc = L.srt_crossings(ns, arr, len(off) - 1, off.ctypes.data_as(C.POINTER(C.c_int64)), api._dp(rows), C.byref(n), C.byref(pe), C.byref(pm))
    return rc, (L.srt_last_error() or b"").decode()


def test_c6_refusals_by_name_before_the_device():
    from stanford_raytracer_amd import api

    ok = api.sphere(7e6)
    for surfaces, text in (((api.surface_array([ok])[0], 0), "nsurf = 0"), ((api.surface_array([ok] * 17)[0], 17), "nsurf = 17"),
                           ([api.Surface(4, 0, (C.c_double * 4)(1, 0, 0, 0))], "unknown kind 4"),
                           ([api.Surface(-1, 0, (C.c_double * 4)(1, 0, 0, 0))], "unknown kind -1"),
                           ([ok, api.sphere(float("nan"))], "surface 1: parameter p[0] is not finite"),
                           ([api.plane((1, 0, float("inf")), 0.0)], "p[2] is not finite"),
                           ([api.sphere(0.0)], "sphere radius 0 is not > 0"), ([api.sphere(-1.0)], "sphere radius"),
                           ([api.lshell(0.0)], "L = 0 is not > 0"), ([api.maglat(np.pi / 2)], "not below pi/2"),
                           ([api.maglat(-2.0)], "not below pi/2"), ([api.plane((0, 0, 0), 1.0)], "normal is zero")):
        rc, msg = _call(surfaces)
        assert rc == api.SRT_EINVAL and text in msg, (text, msg)
    rc, msg = _call([ok], offsets=(1, 2))
    assert rc == api.SRT_EINVAL and "offsets[0] = 1" in msg
    rc, msg = _call([ok], offsets=(0, 3, 2))
    assert rc == api.SRT_EINVAL and "offsets decrease at ray 1" in msg
    # the device entry point says the same before it looks at any pointer
    arr, ns = api.surface_array([api.lshell(-3.0)])
    rc = api.lib().srt_crossings_device(ns, arr, 1, None, None, None, None, 0, None, None)
    assert rc == api.SRT_EINVAL and b"L = -3 is not > 0" in api.lib().srt_last_error()
    arr, ns = api.surface_array([ok])
    rc = api.lib().srt_crossings_device(ns, arr, 1, None, None, None, None, 0, None, None)
    assert rc == api.SRT_EINVAL and b"null d_offsets or d_count" in api.lib().srt_last_error()


def test_c6_no_cpu_fallback():
    from stanford_raytracer_amd import api

    if api.lib().srt_init(0) == api.SRT_OK:
        pytest.skip("GPU present")
    offsets, rows, surfaces = cc.c2_case()
    with pytest.raises(api.SrtError, match="no HIP device"):
        api.crossings(offsets, rows, [api.plane((0, 0, 1), 0.0)])
    with pytest.raises(api.SrtError, match="no HIP device"):
        api.crossings_padded(rows.reshape(2, 3, 20), [3, 3], 1, [api.plane((0, 0, 1), 0.0)])


def test_c6_struct_layout_matches_header(tmp_path):
    from stanford_raytracer_amd import api

    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "srt.h"\nint main(void){printf("%zu %zu %zu %zu %d", '
                   'sizeof(srt_surface), offsetof(srt_surface, kind), offsetof(srt_surface, reserved), offsetof(srt_surface, p), '
                   'SRT_MAXSURF); return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(api.Surface), api.Surface.kind.offset, api.Surface.reserved.offset, api.Surface.p.offset, api.MAXSURF]
    assert got[0] == C.sizeof(CSurface) == 40
    s = api.plane((1, 2, 3), 4)
    assert (s.kind, list(s.p)) == (3, [1.0, 2.0, 3.0, 4.0]) and api.maglat(0.5).kind == 2 and api.lshell(2).kind == 1 and api.sphere(1).kind == 0


def test_c6_file_writer_against_a_parser(tmp_path):
    from stanford_raytracer_amd import api

    rng = np.random.default_rng(5)
    ev = rng.normal(size=(3, 20)) * 10.0 ** rng.integers(-120, 120, size=(3, 20))
    ev[1, 4] = 0.0
    ev[2, 5] = -1.5e-300
    meta = np.array([[0, 0, 0, 1], [0, 15, 6, -1], [41, 3, 1998, 1]], dtype=np.int32)
    raynum = np.array([1, 1, 9999999999], dtype=np.int64)
    path = str(tmp_path / "ev.txt")
    api.write_crossings_file(path, raynum, meta, ev)
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and len(lines) == 4
    for ln, rn, m, e in zip(lines, raynum, meta, ev):
        assert len(ln) == 40 + 20 * 24
        assert [int(ln[10 * k:10 * k + 10]) for k in range(4)] == [rn, m[1] + 1, m[2] + 1, m[3]]
        f = [ln[40 + 24 * k:64 + 24 * k] for k in range(20)]
        assert all(t[-5] == "E" and t[-4] in "+-" for t in f)
        assert np.allclose([float(t) for t in f], e, rtol=6e-16, atol=0)
        for v, t in zip(e, f):  # es24.15e3: the exponent always has three digits
            mant, ex = ("%.15E" % v).split("E")
            assert t == (mant + "E" + ex[0] + "%03d" % int(ex[1:])).rjust(24)
    with pytest.raises(api.SrtError, match="i10"):
        api.write_crossings_file(path, np.array([10 ** 10]), meta[:1], ev[:1])
    api.write_crossings_file(path, np.zeros(0, dtype=np.int64), np.zeros((0, 4), dtype=np.int32), np.zeros((0, 20)))
    assert open(path).read() == ""
