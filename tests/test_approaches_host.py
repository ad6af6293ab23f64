"""CPU: closest approaches to observer points along kept rows (include/srt.h) -- csrc/srt_approaches.hpp's point functions, the
very source the device compiles, built for the host (tests/native/approaches_host.cpp) and held against the numpy restatement and
the truths of tests/approaches_cases.py (A1 .. A6, bars in its docstring); the refusals, the struct layout and the file writer of
the C ABI (A7).

A6, measured with this host build on the oracle's own trajectories (16 Appendix-B rays, NEWRAY_PLASMAPAUSE, adaptive, tmax 2,
maxsteps 2000, del 1e-4): the figures are printed by the test and recorded in profiles/approaches/."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import approaches_cases as ac
from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "approaches_host.cpp")
FLAGS = ["-x", "hip", "--cuda-host-only", "-ffp-contract=off", "-O2", "-std=c++17"]


def _hipcc():
    return shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("aph")
    so = str(d / "libaph.so")
    subprocess.check_call([_hipcc()] + FLAGS + ["-shared", "-fPIC", "-o", so, SRC])
    L = C.CDLL(so)
    L.aph_approaches.argtypes = [C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.POINTER(C.c_longlong), C.c_char_p, C.c_int]
    for f in (L.aph_count_without_reject, L.aph_survivors):
        f.argtypes = [C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]
        f.restype = C.c_longlong
    return L


def _buffers(offsets, rows, observers):
    return (np.ascontiguousarray(offsets, dtype=np.int64), np.ascontiguousarray(rows, dtype=np.float64),
            np.ascontiguousarray(observers, dtype=np.float64).reshape(-1, 4))


def host_approaches(L, offsets, rows, observers, capacity=None):
    """-> (event_rows[min(count, capacity), 20], meta[.., 4], dist[..], count); an observer is 4 doubles, as srt_observer is"""
    offsets, rows, obs = _buffers(offsets, rows, observers)
    why = C.create_string_buffer(200)
    count = C.c_longlong()
    n = len(offsets) - 1
    if capacity is None:
        assert L.aph_approaches(len(obs), obs.ctypes.data, n, offsets.ctypes.data, rows.ctypes.data, 0, None, None, None,
                                C.byref(count), why, 200) == 0, why.value
        capacity = count.value
    ev = np.full((max(capacity, 1), ac.ROW), -7.0)
    meta = np.full((max(capacity, 1), 4), -7, dtype=np.int32)
    dist = np.full(max(capacity, 1), -7.0)
    rc = L.aph_approaches(len(obs), obs.ctypes.data, n, offsets.ctypes.data, rows.ctypes.data, capacity, ev.ctypes.data,
                          meta.ctypes.data, dist.ctypes.data, C.byref(count), why, 200)
    assert rc == 0, why.value
    k = min(count.value, capacity)
    assert np.all(ev[k:] == -7.0) and np.all(meta[k:] == -7) and np.all(dist[k:] == -7.0)  # nothing is written beyond the events kept
    return ev[:k], meta[:k], dist[:k], count.value


def test_a1_straight_rays_against_the_foot_of_the_perpendicular(host):
    offsets, rows, obs, truth = ac.a1_straight_case()
    ev, meta, dist, count = host_approaches(host, offsets, rows, obs)
    ac.check_against_reference(offsets, rows, obs, ev, meta, dist, "A1 straight, host")
    kept = [(r, m, tc, d) for r, m, tc, d, k in truth if k]
    assert count == len(kept) and [(m[0], m[1]) for m in meta.tolist()] == [(r, m) for r, m, _, _ in kept]
    t_err = np.abs(ev[:, 0] - np.array([tc for _, _, tc, _ in kept]))
    d_true = np.array([d for _, _, _, d in kept])
    h = np.diff(ac.A1_TIMES).min()
    print("A1 straight, host: %d events, foot time error max %.3g s (sigma %.3g), distance error max %.3g m"
          % (count, t_err.max(), t_err.max() / h, np.abs(dist - d_true).max()))
    assert np.all(t_err <= ac.SIGMA_BAR * np.diff(ac.A1_TIMES).max())
    assert np.all(np.abs(dist - d_true) <= ac.DIST_BAR * (d_true + 2.7e7 * 0.19))
    # an observer of one ray gives no event on another: they are 1 R_E apart and more
    assert np.array_equal(meta[:, 1] // 5, meta[:, 0])


def test_a1_arcs_against_the_quintic_and_the_count_of_a1(host):
    offsets, rows, obs = ac.a1_arc_case()
    ev, meta, dist, count = host_approaches(host, offsets, rows, obs)
    ac.check_against_reference(offsets, rows, obs, ev, meta, dist, "A1 arcs, host")
    nper = len(ac.cc.C1_TIMES)
    assert (meta[:, 0] < nper).any() and (meta[:, 0] >= nper).any()  # the outbound and the inbound arc
    everything = ac.reference(offsets, rows, obs, dropped=True)
    assert any(not e[6] for e in everything) and {e[1] for e in everything if not e[6]} == {1, 4}  # beyond their radius: dropped
    sig_true, d_true = ac.a1_arc_truth(offsets, rows, obs, meta)
    sig = ac.sigma_of(offsets, rows, ev, meta)
    print("A1 arcs, host: %d events against the quintic's root, sigma error max %.3g, distance error max %.3g m"
          % (count, np.abs(sig - sig_true).max(), np.abs(dist - d_true).max()))
    assert np.all(np.abs(sig - sig_true) <= ac.SIGMA_BAR)
    assert np.all(np.abs(dist - d_true) <= ac.DIST_BAR * (d_true + 3.0 * ac.R_E))
    straight = host_approaches(host, *ac.a1_straight_case()[:3])[3]
    assert count + straight >= 20, (count, straight)


def test_a2_a_row_at_the_closest_point_gives_one_exact_event(host):
    offsets, rows, obs = ac.a2_case()
    ev, meta, dist, count = host_approaches(host, offsets, rows, obs)
    assert meta.tolist() == [[0, 0, 0, 0], [1, 0, 0, 0]]
    for k in range(2):  # sigma = 1 of the first interval: the middle row itself, and the integer distance
        assert ev[k, 0] == 1.0 and ev[k, 1:4].tolist() == [8388608.0, 0.0, 0.0] and dist[k] == 3072.0
    assert np.array_equal(ev[0, 4:], rows[1, 4:])
    ref = ac.reference(offsets, rows, obs)
    assert [(e[0], e[1], e[2], e[3], e[4]) for e in ref] == [(0, 0, 0, 1.0, 3072.0), (1, 0, 0, 1.0, 3072.0)]
    # radius = d keeps it, the next double below drops it
    offsets, rows, obs = ac.a2_case(radius=np.nextafter(3072.0, 0.0))
    assert host_approaches(host, offsets, rows, obs)[3] == 0 and len(ac.reference(offsets, rows, obs)) == 0


@pytest.mark.parametrize("name", sorted(ac.a3_spoilt_cases()))
def test_a3_a_non_finite_value_kills_the_two_intervals_it_touches(host, name):
    offsets, rows, obs, left = ac.a3_spoilt_cases()[name]
    ev, meta, dist, count = host_approaches(host, offsets, rows, obs)
    assert meta[:, 2].tolist() == left and meta[:, 1].tolist() == left and count == 2
    assert [e[2] for e in ac.reference(offsets, rows, obs)] == left
    clean, _ = ac.a3_line()
    assert host_approaches(host, offsets, clean, obs)[1][:, 2].tolist() == [0, 1, 2, 3]


@pytest.mark.parametrize("name", sorted(ac.a3_empty_cases()))
def test_a3_no_events(host, name):
    offsets, rows, obs = ac.a3_empty_cases()[name]
    ev, meta, dist, count = host_approaches(host, offsets, rows, obs)
    assert count == 0 and len(ac.reference(offsets, rows, obs)) == 0
    if name.startswith("t1"):  # the case is not empty for another reason: the unspoilt rows have the event
        clean, _ = ac.a3_line(2)
        assert host_approaches(host, offsets, clean, obs)[3] == 1


def test_a3_an_empty_ray_between_two_others(host):
    offsets, rows, obs = ac.a3_empty_between()
    ev, meta, dist, count = host_approaches(host, offsets, rows, obs)
    assert meta[:, [0, 2]].tolist() == [[0, 0], [0, 1], [0, 2], [2, 0], [2, 1]]
    ac.check_against_reference(offsets, rows, obs, ev, meta, dist, "A3 empty ray")


NOBS = [1, 2, ac.TILE - 1, ac.TILE, ac.TILE + 1, 2 * ac.TILE + 1]


def a4_observers(nobs):
    """nobs observers; with 2, the two are identical"""
    return np.repeat(ac.zigzag_observers(1), 2, axis=0) if nobs == 2 else ac.zigzag_observers(nobs)


@pytest.mark.parametrize("total", [1, 2, 63, 64, 65, 130])
def test_a4_packed_totals_layouts_and_observer_counts(host, total):
    rows = ac.zigzag(total)
    for name, lens in ac.layouts(total).items():
        offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        where = ac.zigzag_intervals(lens)
        for nobs in NOBS:
            obs = a4_observers(nobs)
            ev, meta, dist, count = host_approaches(host, offsets, rows, obs)
            # every interval that starts at an even packed row: an event for every observer, in (ray, interval, observer) order
            want = np.array([[r, m, i, 0] for r, i in where for m in range(nobs)], dtype=np.int32).reshape(-1, 4)
            assert count == len(where) * nobs and np.array_equal(meta, want), (name, nobs)
            if nobs == 2 and count:
                assert np.array_equal(ev[0::2], ev[1::2]) and np.array_equal(dist[0::2], dist[1::2])
            if nobs <= 2 or (total == 65 and name == "boundary_in_wave"):
                ac.check_against_reference(offsets, rows, obs, ev, meta, dist, "A4 host %d rows, %s, %d observers" % (total, name, nobs))
        # approaches, but all beyond their radius; and observers no interval approaches
        assert host_approaches(host, offsets, rows, ac.zigzag_observers(3, radius=1.0))[3] == 0
        far = ac.zigzag_observers(3)
        far[:, 1] *= -1.0  # on the -y side an even row recedes
        assert host_approaches(host, offsets, rows, far)[3] == 3 * _odd_count(lens)


def _odd_count(lens):
    """intervals that start at an odd packed row: from the -y side it is those that hold the approaches"""
    n, base = 0, 0
    for k in lens:
        n += sum(1 for i in range(max(k - 1, 0)) if (base + i) % 2 == 1)
        base += k
    return n


def test_a4_every_capacity_below_the_total(host):
    lens = [37, 0, 28]
    rows = ac.zigzag(65)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    obs = ac.zigzag_observers(3)
    ev, meta, dist, count = host_approaches(host, offsets, rows, obs)
    assert count == 3 * len(ac.zigzag_intervals(lens)) > 90
    for cap in range(count):
        e2, m2, d2, c2 = host_approaches(host, offsets, rows, obs, capacity=cap)
        assert c2 == count and len(m2) == cap and np.array_equal(m2, meta[:cap]) and np.array_equal(e2, ev[:cap]) and np.array_equal(d2, dist[:cap])


def test_a5_the_reject_is_safe_on_hairpins(host):
    offsets, rows, obs, apex = ac.hairpin_case()
    ev, meta, dist, count = host_approaches(host, offsets, rows, obs)
    ac.check_against_reference(offsets, rows, obs, ev, meta, dist, "A5 hairpins, host")
    o, r, ob = _buffers(offsets, rows, obs)
    args = (len(ob), ob.ctypes.data, len(o) - 1, o.ctypes.data, r.ctypes.data)
    survivors, pairs = host.aph_survivors(*args), len(ob) * (len(o) - 1)
    assert host.aph_count_without_reject(*args) == count
    # events that owe their existence to the bulge: of an apex observer with its own interval, and none on the chord
    own = [k for k, m in enumerate(meta.tolist()) if m[1] in apex.tolist() and apex.tolist().index(m[1]) == m[0]]
    chord = ac.reference(offsets, rows, obs, chord=True)
    on_chord = {(e[0], e[1]) for e in chord}
    bulge = [k for k in own if (meta[k, 0], meta[k, 1]) not in on_chord]
    print("A5 hairpins, host: %d events, %d of them only the bulge makes (%d on chords in all); the hull test lets %d of %d pairs through"
          % (count, len(bulge), len(chord), survivors, pairs))
    assert len(bulge) >= 10
    assert count < survivors < pairs  # it rejects, and not only what has no event


def test_the_program_prints_what_the_function_returns(host, tmp_path):
    lens = [37, 0, 28]
    rows = ac.zigzag(65)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    obs = ac.zigzag_observers(ac.TILE + 1)
    ev, meta, dist, count = host_approaches(host, offsets, rows, obs)
    exe = str(tmp_path / "approaches_host")
    subprocess.check_call([_hipcc()] + FLAGS + ["-o", exe, SRC])
    out = subprocess.run([exe], input=program_input(offsets, rows, obs, count), capture_output=True, text=True, check=True).stdout.splitlines()
    assert int(out[0]) == count
    got = np.array([[float(v) for v in ln.split()] for ln in out[1:]])
    assert np.array_equal(got[:, :4].astype(np.int32), meta) and np.array_equal(got[:, 4], dist) and np.array_equal(got[:, 5:], ev)


def program_input(offsets, rows, obs, capacity):
    text = "%d %d %d\n" % (len(obs), len(offsets) - 1, capacity)
    text += "".join(" ".join("%.17g" % v for v in o) + "\n" for o in obs)
    return text + " ".join(str(int(o)) for o in offsets) + "\n" + " ".join("%.17g" % v for v in rows.ravel()) + "\n"


@pytest.fixture(scope="module")
def oracle_rows(tmp_path_factory):
    """The oracle's adaptive trajectories of the 16 Appendix-B rays, packed: every row (outputper 1)."""
    from oracle import oracle
    from stanford_raytracer_amd import workloads as wl

    cfg = tmp_path_factory.mktemp("a6") / "newray.in"
    cfg.write_text(wl.NEWRAY_PLASMAPAUSE)
    pos, d, w = wl.appendix_b_rays()
    rows, nrows, stop, _ = oracle.Model.ngo(str(cfg)).trace(pos, d, w, capacity=2000, **ac.A6_TRACE)
    return ac.pack([rows[i, :nrows[i]] for i in range(len(w))])


def test_a6_hermite_beats_chords_on_the_oracles_trajectories(host, oracle_rows):
    offsets, rows = oracle_rows
    obs, own = ac.a6_observers(offsets, rows)
    full = host_approaches(host, offsets, rows, obs)[:2]
    o4, r4 = ac.cc.thin(offsets, rows, 4)
    herm = host_approaches(host, o4, r4, obs)[:2]
    chord = ac.ref_arrays(ac.reference(o4, r4, obs, chord=True))[:2]
    fig = ac.a6_figures(own, full, herm, chord)
    print(ac.a6_report(fig, "A6 host build, oracle rows (%d .. %d per ray), %d observers, every 4th row kept"
                       % (np.diff(offsets).min(), np.diff(offsets).max(), len(obs))))
    ac.a6_assert(fig)


# ---------------------------------------------------------------------------------------------- A7: the C ABI without a GPU
def _call(observers, nobs=None, offsets=(0, 2), rows=None):
    from stanford_raytracer_amd import api

    L = api.lib()
    arr, no = api.observer_array(observers)
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    rows = np.zeros((max(int(off[-1]), 1), 20)) if rows is None else rows
    n, pe, pm, pd = C.c_int64(), api.dp(), api.ip(), api.dp()
    rc = L.srt_approaches(no if nobs is None else nobs, arr, len(off) - 1, off.ctypes.data_as(C.POINTER(C.c_int64)),
                          api._dp(rows), C.byref(n), C.byref(pe), C.byref(pm), C.byref(pd))
    return rc, (L.srt_last_error() or b"").decode()


def test_a7_refusals_by_name_before_the_device():
    from stanford_raytracer_amd import api

    ok = [1e7, 0.0, 0.0, 5e5]
    for observers, nobs, text in (([ok], 0, "nobs = 0 is outside 1 .. 65536"), ([ok], api.MAXOBS + 1, "nobs = 65537"),
                                  ([ok], -3, "nobs = -3"),
                                  ([ok, [np.nan, 0, 0, 1.0]], None, "observer 1: coordinate x[0] is not finite"),
                                  ([[0, 0, -np.inf, 1.0]], None, "observer 0: coordinate x[2] is not finite"),
                                  ([[0, 0, 0, 0.0]], None, "radius 0 is not finite and > 0"),
                                  ([[0, 0, 0, -2.0]], None, "radius -2 is not finite and > 0"),
                                  ([[0, 0, 0, np.inf]], None, "radius inf is not finite and > 0"),
                                  ([[0, 0, 0, np.nan]], None, "is not finite and > 0")):
        rc, msg = _call(observers, nobs)
        assert rc == api.SRT_EINVAL and text in msg, (text, msg)
    L = api.lib()
    off = np.array([0, 2], dtype=np.int64)
    n, pe, pm, pd = C.c_int64(), api.dp(), api.ip(), api.dp()
    rc = L.srt_approaches(1, None, 1, off.ctypes.data_as(C.POINTER(C.c_int64)), api._dp(np.zeros((2, 20))), C.byref(n), C.byref(pe),
                          C.byref(pm), C.byref(pd))
    assert rc == api.SRT_EINVAL and b"null observers" in L.srt_last_error()
    rc, msg = _call([ok], offsets=(1, 2))
    assert rc == api.SRT_EINVAL and "offsets[0] = 1" in msg
    rc, msg = _call([ok], offsets=(0, 3, 2))
    assert rc == api.SRT_EINVAL and "offsets decrease at ray 1" in msg
    # the device entry point says the same before it looks at any pointer
    arr, no = api.observer_array([[0, 0, 0, -1.0]])
    rc = L.srt_approaches_device(no, arr, 1, None, None, None, None, None, 0, None, None)
    assert rc == api.SRT_EINVAL and b"radius -1 is not finite and > 0" in L.srt_last_error()
    arr, no = api.observer_array([ok])
    assert L.srt_approaches_device(0, arr, 1, None, None, None, None, None, 0, None, None) == api.SRT_EINVAL and b"nobs = 0" in L.srt_last_error()
    assert L.srt_approaches_device(1, None, 1, None, None, None, None, None, 0, None, None) == api.SRT_EINVAL and b"null observers" in L.srt_last_error()
    rc = L.srt_approaches_device(no, arr, 1, None, None, None, None, None, 0, None, None)
    assert rc == api.SRT_EINVAL and b"null d_offsets or d_count" in L.srt_last_error()


def test_a7_no_cpu_fallback():
    from stanford_raytracer_amd import api

    if api.lib().srt_init(0) == api.SRT_OK:
        pytest.skip("GPU present")
    offsets, rows, obs = ac.a2_case()
    with pytest.raises(api.SrtError, match="no HIP device"):
        api.approaches(obs, offsets, rows)
    with pytest.raises(api.SrtError, match="no HIP device"):
        api.approaches_padded(rows.reshape(2, 3, 20), [3, 3], 1, [api.Observer((C.c_double * 3)(1e7, 0, 0), 5e5)])


def test_a7_struct_layout_matches_header(tmp_path):
    from stanford_raytracer_amd import api

    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "srt.h"\nint main(void){printf("%zu %zu %zu %d", '
                   'sizeof(srt_observer), offsetof(srt_observer, x), offsetof(srt_observer, radius), SRT_MAXOBS); return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(api.Observer), api.Observer.x.offset, api.Observer.radius.offset, api.MAXOBS] == [32, 0, 24, ac.MAXOBS]
    arr, n = api.observer_array(np.array([[1.0, 2.0, 3.0, 4.0], [5.0, 6.0, 7.0, 8.0]]))
    assert n == 2 and list(arr[1].x) == [5.0, 6.0, 7.0] and arr[1].radius == 8.0
    arr, n = api.observer_array([api.Observer((C.c_double * 3)(1, 2, 3), 4)])
    assert n == 1 and list(arr[0].x) == [1.0, 2.0, 3.0] and arr[0].radius == 4.0


def test_a7_file_writer_against_a_parser(tmp_path):
    from stanford_raytracer_amd import api

    rng = np.random.default_rng(5)
    ev = rng.normal(size=(3, 20)) * 10.0 ** rng.integers(-120, 120, size=(3, 20))
    ev[1, 4] = 0.0
    ev[2, 5] = -1.5e-300
    dist = np.array([0.0, 3072.0, 1.25e-200])
    meta = np.array([[0, 0, 0, 0], [0, 65535, 6, 0], [41, 3, 1998, 0]], dtype=np.int32)
    raynum = np.array([1, 1, 9999999999], dtype=np.int64)
    path = str(tmp_path / "ev.txt")
    api.write_approaches_file(path, raynum, meta, dist, ev)
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and len(lines) == 4
    for ln, rn, m, dd, e in zip(lines, raynum, meta, dist, ev):
        assert len(ln) == 40 + 21 * 24
        assert [int(ln[10 * k:10 * k + 10]) for k in range(4)] == [rn, m[1] + 1, m[2] + 1, 0]
        f = [ln[40 + 24 * k:64 + 24 * k] for k in range(21)]
        assert all(t[-5] == "E" and t[-4] in "+-" for t in f)
        vals = np.concatenate([[dd], e])
        assert np.allclose([float(t) for t in f], vals, rtol=6e-16, atol=0)
        for v, t in zip(vals, f):  # es24.15e3: the exponent always has three digits
            mant, ex = ("%.15E" % v).split("E")
            assert t == (mant + "E" + ex[0] + "%03d" % int(ex[1:])).rjust(24)
    with pytest.raises(api.SrtError, match="i10"):
        api.write_approaches_file(path, np.array([10 ** 10]), meta[:1], dist[:1], ev[:1])
    api.write_approaches_file(path, np.zeros(0, dtype=np.int64), np.zeros((0, 4), dtype=np.int32), np.zeros(0), np.zeros((0, 20)))
    assert open(path).read() == ""
