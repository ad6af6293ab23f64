"""GPU (-m gpu): closest approaches to observer points along kept rows on the device (include/srt.h) -- srt_approaches and
srt_approaches_device on the cases and at the bars of tests/approaches_cases.py (A1 .. A5), against the host build of the same
header (tests/native/approaches_host.cpp) and the numpy restatement; the launch shapes and observer counts at which a
row-per-lane pass over LDS tiles can go wrong; and the path trace -> pack -> approaches that never leaves the device.

Event rows, meta and distances equal the host build bit for bit: only +, -, x and sqrt with contraction off reach an event.  The
equality is asserted."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch  # before the library's first call: torch brings its own HIP runtime and must initialise it first

import approaches_cases as ac
from conftest import ROOT
from stanford_raytracer_amd import api, parallel, workloads as wl
from stanford_raytracer_amd.device_batch import DeviceBatch

pytestmark = pytest.mark.gpu
if torch.cuda.is_available():
    torch.cuda.init()

SRC = os.path.join(ROOT, "tests", "native", "approaches_host.cpp")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("aph") / "libaph.so")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-ffp-contract=off", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, SRC])
    L = C.CDLL(so)
    L.aph_approaches.argtypes = [C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.POINTER(C.c_longlong), C.c_char_p, C.c_int]
    return L


def host_approaches(L, offsets, rows, observers):
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    obs = np.ascontiguousarray(observers, dtype=np.float64).reshape(-1, 4)
    why, count = C.create_string_buffer(200), C.c_longlong()
    n = len(offsets) - 1
    assert L.aph_approaches(len(obs), obs.ctypes.data, n, offsets.ctypes.data, rows.ctypes.data, 0, None, None, None, C.byref(count), why, 200) == 0
    k = max(count.value, 1)
    ev, meta, dist = np.zeros((k, 20)), np.zeros((k, 4), dtype=np.int32), np.zeros(k)
    assert L.aph_approaches(len(obs), obs.ctypes.data, n, offsets.ctypes.data, rows.ctypes.data, count.value, ev.ctypes.data,
                            meta.ctypes.data, dist.ctypes.data, C.byref(count), why, 200) == 0
    return ev[:count.value], meta[:count.value], dist[:count.value]


def device_approaches(offsets, rows, observers, capacity=None):
    """srt_approaches_device on uploaded buffers -> (event_rows, meta, dist, count) on the host; beyond the events kept the
    outputs must be as they were handed in"""
    api.init(0)
    d_off = torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.int64)).cuda()
    d_rows = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, 20)).cuda()
    if d_rows.shape[0] == 0:
        d_rows = torch.zeros((1, 20), dtype=torch.float64, device="cuda")
    ev, meta, dist, count = parallel.approaches_device(d_rows, d_off, observers, capacity=capacity)
    torch.cuda.synchronize()
    n = int(count.item())
    if ev is None:
        return np.zeros((0, 20)), np.zeros((0, 4), dtype=np.int32), np.zeros(0), n
    k = min(n, ev.shape[0])
    assert not ev[k:].any() and not meta[k:].any() and not dist[k:].any()
    return ev[:k].cpu().numpy(), meta[:k].cpu().numpy(), dist[:k].cpu().numpy(), n


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def both_paths(host, offsets, rows, obs, label):
    """srt_approaches and srt_approaches_device give the same bits, and they are the host build's -> (ev, meta, dist)"""
    api.init(0)
    ev, meta, dist = api.approaches(obs, offsets, rows)
    ev2, meta2, dist2, n2 = device_approaches(offsets, rows, obs)
    assert n2 == len(meta) and np.array_equal(meta, meta2) and np.array_equal(bits(ev), bits(ev2)) and np.array_equal(bits(dist), bits(dist2)), label
    hev, hmeta, hdist = host_approaches(host, offsets, rows, obs)
    assert np.array_equal(meta, hmeta), label
    same = int(np.sum(np.all(bits(ev) == bits(hev), axis=1) & (bits(dist) == bits(hdist)))) if len(ev) else 0
    print("%s: %d events, %d bit-equal to the host build in row and distance" % (label, len(ev), same))
    assert same == len(ev), label
    return ev, meta, dist


def test_a1_to_a3_at_the_bars_and_bit_equal_to_the_host_build(host):
    offsets, rows, obs, truth = ac.a1_straight_case()
    ev, meta, dist = both_paths(host, offsets, rows, obs, "A1 straight, device")
    ac.check_against_reference(offsets, rows, obs, ev, meta, dist, "A1 straight, device")
    kept = [(r, m, tc, d) for r, m, tc, d, k in truth if k]
    assert [(m[0], m[1]) for m in meta.tolist()] == [(r, m) for r, m, _, _ in kept]
    d_true = np.array([d for _, _, _, d in kept])
    assert np.all(np.abs(ev[:, 0] - np.array([tc for _, _, tc, _ in kept])) <= ac.SIGMA_BAR * np.diff(ac.A1_TIMES).max())
    assert np.all(np.abs(dist - d_true) <= ac.DIST_BAR * (d_true + 2.7e7 * 0.19))
    n1 = len(meta)
    offsets, rows, obs = ac.a1_arc_case()
    ev, meta, dist = both_paths(host, offsets, rows, obs, "A1 arcs, device")
    ac.check_against_reference(offsets, rows, obs, ev, meta, dist, "A1 arcs, device")
    nper = len(ac.cc.C1_TIMES)
    assert (meta[:, 0] < nper).any() and (meta[:, 0] >= nper).any()
    sig_true, d_true = ac.a1_arc_truth(offsets, rows, obs, meta)
    sig = ac.sigma_of(offsets, rows, ev, meta)
    print("A1 arcs, device: sigma error against the quintic's root max %.3g, distance error max %.3g m" % (np.abs(sig - sig_true).max(), np.abs(dist - d_true).max()))
    assert np.all(np.abs(sig - sig_true) <= ac.SIGMA_BAR) and np.all(np.abs(dist - d_true) <= ac.DIST_BAR * (d_true + 3.0 * ac.R_E))
    assert n1 + len(meta) >= 20
    # A2: exact
    offsets, rows, obs = ac.a2_case()
    ev, meta, dist = both_paths(host, offsets, rows, obs, "A2 device")
    assert meta.tolist() == [[0, 0, 0, 0], [1, 0, 0, 0]]
    for k in range(2):
        assert ev[k, 0] == 1.0 and ev[k, 1:4].tolist() == [8388608.0, 0.0, 0.0] and dist[k] == 3072.0
    offsets, rows, obs = ac.a2_case(radius=np.nextafter(3072.0, 0.0))
    assert len(api.approaches(obs, offsets, rows)[1]) == 0 and device_approaches(offsets, rows, obs)[3] == 0
    # A3
    for name, (offsets, rows, obs, left) in sorted(ac.a3_spoilt_cases().items()):
        ev, meta, dist = both_paths(host, offsets, rows, obs, "A3 device, " + name)
        assert meta[:, 2].tolist() == left and meta[:, 1].tolist() == left, name
    for name, (offsets, rows, obs) in sorted(ac.a3_empty_cases().items()):
        ev, meta, dist = api.approaches(obs, offsets, rows)
        assert ev.shape == (0, 20) and meta.shape == (0, 4) and dist.shape == (0,), name
        assert device_approaches(offsets, rows, obs)[3] == 0, name
    offsets, rows, obs = ac.a3_empty_between()
    ev, meta, dist = both_paths(host, offsets, rows, obs, "A3 device, empty ray between two")
    assert meta[:, [0, 2]].tolist() == [[0, 0], [0, 1], [0, 2], [2, 0], [2, 1]]
    ac.check_against_reference(offsets, rows, obs, ev, meta, dist, "A3 device")


NOBS = [1, 2, ac.TILE - 1, ac.TILE, ac.TILE + 1, 2 * ac.TILE + 1]


def a4_observers(nobs):
    return np.repeat(ac.zigzag_observers(1), 2, axis=0) if nobs == 2 else ac.zigzag_observers(nobs)


@pytest.mark.parametrize("total", [1, 2, 63, 64, 65, 130])
def test_a4_packed_totals_layouts_and_observer_counts(host, total):
    rows = ac.zigzag(total)
    for name, lens in ac.layouts(total).items():
        offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        where = ac.zigzag_intervals(lens)
        for nobs in NOBS:
            obs = a4_observers(nobs)
            ev, meta, dist, n = device_approaches(offsets, rows, obs)
            hev, hmeta, hdist = host_approaches(host, offsets, rows, obs)
            want = np.array([[r, m, i, 0] for r, i in where for m in range(nobs)], dtype=np.int32).reshape(-1, 4)
            assert n == len(where) * nobs and np.array_equal(meta, want) and np.array_equal(meta, hmeta), (name, nobs)
            assert np.array_equal(bits(ev), bits(hev)) and np.array_equal(bits(dist), bits(hdist)), (name, nobs)
            if nobs == 2 and n:
                assert np.array_equal(bits(ev[0::2]), bits(ev[1::2])) and np.array_equal(bits(dist[0::2]), bits(dist[1::2]))
            if nobs <= 2:
                ac.check_against_reference(offsets, rows, obs, ev, meta, dist, "A4 device %d rows, %s, %d observers" % (total, name, nobs))
            if n and nobs in (1, ac.TILE + 1):  # half the capacity: the first events, the full count, nothing beyond
                e2, m2, d2, n2 = device_approaches(offsets, rows, obs, capacity=n // 2 + 1)
                k = n // 2 + 1
                assert n2 == n and np.array_equal(m2, hmeta[:k]) and np.array_equal(bits(e2), bits(hev[:k])) and np.array_equal(bits(d2), bits(hdist[:k]))
        # approaches, but all beyond their radius
        assert device_approaches(offsets, rows, ac.zigzag_observers(3, radius=1.0))[3] == 0, name


def test_a4_every_capacity_below_the_total(host):
    lens = [37, 0, 28]
    rows = ac.zigzag(65)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    obs = ac.zigzag_observers(3)
    hev, hmeta, hdist = host_approaches(host, offsets, rows, obs)
    count = len(hmeta)
    assert count > 90
    for cap in range(count):
        e2, m2, d2, n2 = device_approaches(offsets, rows, obs, capacity=cap)
        assert n2 == count and len(m2) == cap and np.array_equal(m2, hmeta[:cap]) and np.array_equal(bits(e2), bits(hev[:cap])) \
            and np.array_equal(bits(d2), bits(hdist[:cap])), cap


def test_a5_the_reject_is_safe_on_hairpins(host):
    offsets, rows, obs, apex = ac.hairpin_case()
    ev, meta, dist = both_paths(host, offsets, rows, obs, "A5 hairpins, device")
    ac.check_against_reference(offsets, rows, obs, ev, meta, dist, "A5 hairpins, device")
    on_chord = {(e[0], e[1]) for e in ac.reference(offsets, rows, obs, chord=True)}
    bulge = [m for m in meta.tolist() if m[1] in apex.tolist() and apex.tolist().index(m[1]) == m[0] and (m[0], m[1]) not in on_chord]
    assert len(bulge) >= 10


NGO_FIXED = dict(fixedstep=1, dt0=2e-3, tmax=0.4, maxsteps=200, del_=1e-4, outputper=4)


@pytest.fixture(scope="module")
def ngo(tmp_path_factory):
    api.init(0)
    cfg = tmp_path_factory.mktemp("ap") / "newray.in"
    cfg.write_text(wl.NEWRAY_PLASMAPAUSE)
    return api.Model.ngo(str(cfg))


def test_trace_pack_approaches_without_leaving_the_device(ngo):
    """16 Ngo rays, fixed step, outputper 4: trace -> srt_pack_rows_device -> srt_approaches_device on device buffers, observers
    beside the rays' own rows; the result is api.approaches of the downloaded rows bit for bit, approaches_padded gives the same,
    and so do the same rays through trace_packed(segment_rows = 4), segment by segment, on the intervals a segment holds."""
    pos, d, w = wl.appendix_b_rays()
    p = api.make_params(**NGO_FIXED)
    batch = DeviceBatch(ngo, p, pos, d, w, torch.device("cuda", 0))
    o = batch.launch()
    packed, offsets = parallel.pack_rows_device(o["rows"], o["nrows"], p.outputper)
    off_h = offsets.cpu().numpy()
    rows_h = packed[:int(off_h[-1])].cpu().numpy()
    # observers from the rays' own kept rows: beside the middle of three intervals of every ray, 50 km off, radius 150 km
    obs = []
    for ray in range(len(w)):
        k = int(off_h[ray + 1] - off_h[ray])
        for i in sorted({k // 6, k // 2, (5 * k) // 6} - {k - 1}):
            r0, r1 = rows_h[off_h[ray] + i], rows_h[off_h[ray] + i + 1]
            obs.append(np.concatenate([0.5 * (r0[1:4] + r1[1:4]) + ac.A6_OFFSET * ac.perpendicular(r0[7:10]), [ac.A6_RADIUS]]))
    obs = np.array(obs)
    ev, meta, dist, count = parallel.approaches_device(packed, offsets, obs)
    torch.cuda.synchronize()
    n = int(count.item())
    assert n == ev.shape[0] >= len(w)
    ev_h, meta_h, dist_h = api.approaches(obs, off_h, rows_h)
    assert np.array_equal(meta.cpu().numpy(), meta_h) and np.array_equal(bits(ev.cpu().numpy()), bits(ev_h)) \
        and np.array_equal(bits(dist.cpu().numpy()), bits(dist_h))
    assert len(set(meta_h[:, 0].tolist())) == len(w)  # every ray passes an observer of its own
    # the padded form packs on the host first
    ev_p, meta_p, dist_p = api.approaches_padded(o["rows"].cpu().numpy(), o["nrows"].cpu().numpy(), p.outputper, obs)
    assert np.array_equal(meta_p, meta_h) and np.array_equal(bits(ev_p), bits(ev_h)) and np.array_equal(bits(dist_p), bits(dist_h))
    # segmented, as one packed set
    off_s, rows_s, _, _, _ = ngo.trace_packed(pos, d, w, 4, params=p)
    assert np.array_equal(off_s, off_h)
    ev_s, meta_s, dist_s = api.approaches(obs, off_s, rows_s)
    assert np.array_equal(meta_s, meta_h) and np.array_equal(bits(ev_s), bits(ev_h)) and np.array_equal(bits(dist_s), bits(dist_h))
    # segment by segment, as trace_segments hands them out (no interval is carried across a seam): the events of the whole set
    # that lie in the intervals a segment holds
    got, start = 0, np.zeros(len(w), dtype=np.int64)
    for seg in ngo.trace_segments(pos, d, w, 4, params=p):
        lens = np.diff(seg["offsets"])
        ev_g, meta_g, dist_g = api.approaches(obs, seg["offsets"], seg["rows"])
        first, last = np.full(len(w), -1), np.full(len(w), -1)
        first[seg["ray"]], last[seg["ray"]] = start[seg["ray"]], start[seg["ray"]] + lens - 1
        inside = (meta_h[:, 2] >= first[meta_h[:, 0]]) & (meta_h[:, 2] < last[meta_h[:, 0]])
        want = meta_h[inside].copy()
        want[:, 2] -= first[want[:, 0]].astype(np.int32)
        want[:, 0] = np.searchsorted(seg["ray"], want[:, 0])
        assert np.array_equal(meta_g, want) and np.array_equal(bits(ev_g), bits(ev_h[inside])) and np.array_equal(bits(dist_g), bits(dist_h[inside]))
        got += len(meta_g)
        start[seg["ray"]] += lens
    assert np.array_equal(start, np.diff(off_h))
    seams = int(np.sum(meta_h[:, 2] % 4 == 3))
    assert got + seams == n
    print("16 Ngo rays, fixed step, outputper 4: %d kept rows, %d observers, %d events, identical through the device path, the "
          "host-buffer path, the padded path and a segmented trace; segment by segment %d events, %d lie in intervals across a seam"
          % (off_h[-1], len(obs), n, got, seams))


def test_device_entry_point_refuses_what_it_cannot_bound():
    """Host pointers, an offsets[nrays] beyond 2^31 - 2 rows, and a capacity with a null output: SRT_EINVAL, nothing launched."""
    api.init(0)
    arr, no = api.observer_array([[7e6, 0.0, 0.0, 1e5]])
    L = api.lib()
    host_off = np.array([0, 2], dtype=np.int64)
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    rows = torch.zeros((2, 20), dtype=torch.float64, device="cuda")
    rc = L.srt_approaches_device(no, arr, 1, host_off.ctypes.data, rows.data_ptr(), None, None, None, 0, count.data_ptr(), None)
    assert rc == api.SRT_EINVAL and b"not device memory" in L.srt_last_error()
    big = torch.tensor([0, 1 << 40], dtype=torch.int64, device="cuda")
    rc = L.srt_approaches_device(no, arr, 1, big.data_ptr(), rows.data_ptr(), None, None, None, 0, count.data_ptr(), None)
    assert rc == api.SRT_EINVAL and b"too many" in L.srt_last_error()
    ev = torch.zeros((1, 20), dtype=torch.float64, device="cuda")
    meta = torch.zeros((1, 4), dtype=torch.int32, device="cuda")
    rc = L.srt_approaches_device(no, arr, 1, big.data_ptr(), rows.data_ptr(), ev.data_ptr(), meta.data_ptr(), None, 1, count.data_ptr(), None)
    assert rc == api.SRT_EINVAL and b"null output" in L.srt_last_error()
