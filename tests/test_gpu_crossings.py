"""GPU (-m gpu): surface crossings along kept rows on the device (include/srt.h) -- srt_crossings and srt_crossings_device on the
cases and at the bars of tests/crossings_cases.py (C1 .. C5), against the host build of the same header
(tests/native/crossings_host.cpp) and the numpy restatement; the launch shapes at which a row-per-lane pass can go wrong; and the
path trace -> pack -> crossings that never leaves the device.

The bit-equal share of the device's event rows against the host build is printed (it is recorded in
profiles/crossings/gpu_figures.txt); it was measured as 1 on C1 .. C4 and is asserted there."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch  # before the library's first call: torch brings its own HIP runtime and must initialise it first

import crossings_cases as cc
from conftest import ROOT
from stanford_raytracer_amd import api, parallel, workloads as wl
from stanford_raytracer_amd.device_batch import DeviceBatch

pytestmark = pytest.mark.gpu
if torch.cuda.is_available():
    torch.cuda.init()

SRC = os.path.join(ROOT, "tests", "native", "crossings_host.cpp")


class CSurface(C.Structure):
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("p", C.c_double * 4)]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("cxh") / "libcxh.so")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-ffp-contract=off", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, SRC])
    L = C.CDLL(so)
    L.cxh_crossings.argtypes = [C.c_int, C.POINTER(CSurface), C.c_longlong, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p,
                                C.c_void_p, C.POINTER(C.c_longlong), C.c_char_p, C.c_int]
    return L


def host_crossings(L, offsets, rows, surfaces):
    arr = (CSurface * max(len(surfaces), 1))()
    for i, (kind, p) in enumerate(surfaces):
        arr[i] = CSurface(kind, 0, (C.c_double * 4)(*[float(v) for v in p]))
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    why, count = C.create_string_buffer(200), C.c_longlong()
    n = len(offsets) - 1
    assert L.cxh_crossings(len(surfaces), arr, n, offsets.ctypes.data, rows.ctypes.data, 0, None, None, C.byref(count), why, 200) == 0
    ev, meta = np.zeros((max(count.value, 1), 20)), np.zeros((max(count.value, 1), 4), dtype=np.int32)
    assert L.cxh_crossings(len(surfaces), arr, n, offsets.ctypes.data, rows.ctypes.data, count.value, ev.ctypes.data, meta.ctypes.data,
                           C.byref(count), why, 200) == 0
    return ev[:count.value], meta[:count.value]


def lib_surfaces(surfaces):
    return [api.Surface(k, 0, (C.c_double * 4)(*[float(v) for v in p])) for k, p in surfaces]


def device_crossings(offsets, rows, surfaces, capacity=None):
    """srt_crossings_device on uploaded buffers -> (event_rows, meta, count) on the host"""
    api.init(0)
    d_off = torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.int64)).cuda()
    d_rows = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, 20)).cuda()
    if d_rows.shape[0] == 0:
        d_rows = torch.zeros((1, 20), dtype=torch.float64, device="cuda")
    ev, meta, count = parallel.crossings_device(d_rows, d_off, lib_surfaces(surfaces), capacity=capacity)
    torch.cuda.synchronize()
    n = int(count.item())
    if ev is None:
        return np.zeros((0, 20)), np.zeros((0, 4), dtype=np.int32), n
    k = min(n, ev.shape[0])
    return ev[:k].cpu().numpy(), meta[:k].cpu().numpy(), n


def both_paths(host, offsets, rows, surfaces, label):
    """srt_crossings and srt_crossings_device give the same bits; the meta is the host build's; -> (ev, meta, bit-equal rows, rows)"""
    api.init(0)
    ev, meta = api.crossings(offsets, rows, lib_surfaces(surfaces))
    ev2, meta2, n2 = device_crossings(offsets, rows, surfaces)
    assert n2 == len(meta) and np.array_equal(meta, meta2) and np.array_equal(ev.view(np.uint64), ev2.view(np.uint64)), label
    hev, hmeta = host_crossings(host, offsets, rows, surfaces)
    assert np.array_equal(meta, hmeta), label
    same = int(np.sum(np.all(ev.view(np.uint64) == hev.view(np.uint64), axis=1))) if len(ev) else 0
    print("%s: %d events, %d event rows bit-equal to the host build (share %.4f)" % (label, len(ev), same, same / max(len(ev), 1)))
    return ev, meta, same, len(ev)


def test_c1_to_c4_at_the_bars_and_the_bit_equal_share(host):
    same = total = 0
    offsets, rows, surfaces = cc.c1_case()
    ev, meta, s, t = both_paths(host, offsets, rows, surfaces, "C1 device")
    same, total = same + s, total + t
    cc.check_against_reference(offsets, rows, surfaces, ev, meta, "C1 device")
    for si in range(len(surfaces)):
        assert {1, -1} <= set(meta[meta[:, 1] == si, 3].tolist())
    idx, sig_true = cc.c1_plane_truth(offsets, rows, surfaces, meta)
    assert len(idx) >= 8 and np.all(np.abs(cc.sigma_of(offsets, rows, ev, meta)[idx] - sig_true) <= cc.SIGMA_BAR)
    offsets, rows, surfaces = cc.c2_case()
    ev, meta, s, t = both_paths(host, offsets, rows, surfaces, "C2 device")
    same, total = same + s, total + t
    assert meta.tolist() == [[0, 0, 0, 1], [1, 0, 1, -1]]
    sig = cc.sigma_of(offsets, rows, ev, meta)
    assert abs(sig[0] - 1.0) <= cc.SIGMA_BAR and abs(sig[1]) <= cc.SIGMA_BAR
    cc.check_against_reference(offsets, rows, surfaces, ev, meta, "C2 device")
    for name, (offsets, rows, surfaces) in sorted(cc.c3_cases().items()):
        ev, meta = api.crossings(offsets, rows, lib_surfaces(surfaces))
        assert ev.shape == (0, 20) and meta.shape == (0, 4), name
        assert device_crossings(offsets, rows, surfaces)[2] == 0, name
    offsets, rows, surfaces = cc.c3_empty_between()
    ev, meta, s, t = both_paths(host, offsets, rows, surfaces, "C3 device, empty ray between two")
    same, total = same + s, total + t
    assert set(meta[:, 0].tolist()) == {0, 2}
    cc.check_against_reference(offsets, rows, surfaces, ev, meta, "C3 device")
    for nsurf in (1, 16):
        offsets, rows, surfaces = cc.c4_case(nsurf)
        ev, meta, s, t = both_paths(host, offsets, rows, surfaces, "C4 device, %d surfaces" % nsurf)
        same, total = same + s, total + t
        cc.check_against_reference(offsets, rows, surfaces, ev, meta, "C4 device")
        keys = [(m[0], m[2], m[1]) for m in meta.tolist()]
        assert keys == sorted(keys) and len(set(keys)) == len(keys)
        if nsurf == 16:
            a, b = meta[:, 1] == 3, meta[:, 1] == 11
            assert a.sum() == b.sum() > 0 and np.array_equal(ev[a], ev[b])
        for cap in (1, len(meta) // 2, len(meta) - 1):  # the first events of the order, and the full count
            e2, m2, n2 = device_crossings(offsets, rows, surfaces, capacity=cap)
            assert n2 == len(meta) and np.array_equal(m2, meta[:cap]) and np.array_equal(e2.view(np.uint64), ev[:cap].view(np.uint64))
        assert device_crossings(offsets, rows, surfaces, capacity=0)[2] == len(meta)
    print("C1 .. C4 device: bit-equal share of event rows against the host build %d / %d = %.4f" % (same, total, same / total))
    assert same == total  # measured 121 / 121 on an MI355X: the share is 1, so it is held there


def zigzag(total):
    """total rows whose z alternates between -1000 and +1000 m: every interval of consecutive rows crosses every plane z = c,
    |c| < 1000, transversally; x advances, t advances."""
    r = np.zeros((total, 20))
    i = np.arange(total)
    r[:, 0] = 0.01 * i
    r[:, 1] = 7.0e6 + 300.0 * i
    r[:, 2] = 40.0 * i
    r[:, 3] = np.where(i % 2 == 0, -1000.0, 1000.0)
    r[:, 7] = 300.0 / 0.01 / cc.C_LIGHT
    r[:, 8] = 40.0 / 0.01 / cc.C_LIGHT
    r[:, 9] = 0.0  # a turning point at every row
    r[:, 4:7] = 0.3
    r[:, 10:13] = 5.0 + 0.01 * i[:, None]
    r[:, 13:16] = 2e-5
    r[:, 16:20] = 1e9 + 1e5 * i[:, None]
    return r


PLANES16 = [(cc.PLANE, [0.0, 0.0, 1.0, -750.0 + 100.0 * k]) for k in range(16)]
FAR = [(cc.PLANE, [0.0, 0.0, 1.0, 1.0e9]), (cc.SPHERE, [1.0e3, 0, 0, 0])]


def layouts(total):
    """name -> ray lengths that sum to `total`"""
    out = {"one_ray": [total], "rays_of_2": [2] * (total // 2) + [1] * (total % 2)}
    if total > 40:  # a ray boundary inside a wave, and an empty ray at it
        out["boundary_in_wave"] = [37, 0, total - 37]
    return out


@pytest.mark.parametrize("total", [1, 2, 63, 64, 65, 130])
def test_packed_totals_and_ray_layouts(host, total):
    rows = zigzag(total)
    for name, lens in layouts(total).items():
        offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        intervals = int(sum(max(k - 1, 0) for k in lens))
        # every interval an event for all 16 surfaces
        ev, meta, n = device_crossings(offsets, rows, PLANES16)
        hev, hmeta = host_crossings(host, offsets, rows, PLANES16)
        assert n == 16 * intervals == len(hmeta), (name, n)
        assert np.array_equal(meta, hmeta), name
        if n:
            ray = np.repeat(np.arange(len(lens)), [max(k - 1, 0) for k in lens])
            iv = np.concatenate([np.arange(max(k - 1, 0)) for k in lens])
            assert np.array_equal(meta[:, 0], np.repeat(ray, 16)) and np.array_equal(meta[:, 2], np.repeat(iv, 16))
            assert np.array_equal(meta[:, 1], np.tile(np.arange(16), intervals))
            scale = np.linalg.norm(hev[:, 1:4], axis=1) + 2100.0
            assert np.all(np.linalg.norm(ev[:, 1:4] - hev[:, 1:4], axis=1) <= cc.POS_BAR * scale), name
            assert np.all(np.abs(ev[:, 3] - (-750.0 + 100.0 * meta[:, 1])) <= 1e-12 * 7.1e6), name  # on its plane
            j = offsets[meta[:, 0]] + meta[:, 2]
            assert np.all((ev[:, 0] > rows[j, 0]) & (ev[:, 0] < rows[j + 1, 0]))
        # zero events
        ev, meta, n = device_crossings(offsets, rows, FAR)
        assert n == 0 and len(meta) == 0, name
        # half the capacity: the first events, the full count
        if intervals:
            e2, m2, n2 = device_crossings(offsets, rows, PLANES16, capacity=8 * intervals)
            assert n2 == 16 * intervals and np.array_equal(m2, hmeta[:8 * intervals])


NGO_FIXED = dict(fixedstep=1, dt0=2e-3, tmax=0.4, maxsteps=200, del_=1e-4, outputper=4)


@pytest.fixture(scope="module")
def ngo(tmp_path_factory):
    api.init(0)
    cfg = tmp_path_factory.mktemp("cx") / "newray.in"
    cfg.write_text(wl.NEWRAY_PLASMAPAUSE)
    return api.Model.ngo(str(cfg))


def test_trace_pack_crossings_without_leaving_the_device(ngo):
    """16 Ngo rays, fixed step: trace -> srt_pack_rows_device -> srt_crossings_device on device buffers; the result is
    api.crossings of the downloaded rows bit for bit; the same rays through trace_packed(segment_rows = 4) give identical events."""
    pos, d, w = wl.appendix_b_rays()
    p = api.make_params(**NGO_FIXED)
    surf = lib_surfaces(cc.c5_surfaces() + [(cc.SPHERE, [1.2 * cc.R_E, 0, 0, 0]), (cc.MAGLAT, [np.deg2rad(-10.0), 0, 0, 0])])
    batch = DeviceBatch(ngo, p, pos, d, w, torch.device("cuda", 0))
    o = batch.launch()
    packed, offsets = parallel.pack_rows_device(o["rows"], o["nrows"], p.outputper)
    ev, meta, count = parallel.crossings_device(packed, offsets, surf)
    torch.cuda.synchronize()
    n = int(count.item())
    assert n == ev.shape[0] > 0
    off_h = offsets.cpu().numpy()
    rows_h = packed[:int(off_h[-1])].cpu().numpy()
    ev_h, meta_h = api.crossings(off_h, rows_h, surf)
    assert np.array_equal(meta.cpu().numpy(), meta_h) and np.array_equal(ev.cpu().numpy().view(np.uint64), ev_h.view(np.uint64))
    # the padded form packs on the host first
    ev_p, meta_p = api.crossings_padded(o["rows"].cpu().numpy(), o["nrows"].cpu().numpy(), p.outputper, surf)
    assert np.array_equal(meta_p, meta_h) and np.array_equal(ev_p.view(np.uint64), ev_h.view(np.uint64))
    # segmented
    off_s, rows_s, _, _, _ = ngo.trace_packed(pos, d, w, 4, params=p)
    assert np.array_equal(off_s, off_h)
    ev_s, meta_s = api.crossings(off_s, rows_s, surf)
    assert np.array_equal(meta_s, meta_h) and np.array_equal(ev_s.view(np.uint64), ev_h.view(np.uint64))
    print("16 Ngo rays, fixed step, outputper 4: %d kept rows, %d events, identical through the device path, the host-buffer "
          "path, the padded path and a segmented trace" % (off_h[-1], n))


def test_c5_hermite_beats_linear_on_the_devices_own_rows(ngo):
    pos, d, w = wl.appendix_b_rays()
    rows, nrows, stop, _ = ngo.trace(pos, d, w, outputper=1, **cc.C5_TRACE)
    offsets, packed = api.pack_rows(rows, nrows, 1)
    surf = cc.c5_surfaces()
    full = api.crossings(offsets, packed, lib_surfaces(surf))
    o4, r4 = cc.thin(offsets, packed, 4)
    herm = api.crossings(o4, r4, lib_surfaces(surf))
    lin = cc.ref_arrays(cc.reference(o4, r4, surf, linear=True))[:2]
    fig = cc.c5_figures(full, herm, lin)
    print(cc.c5_report(fig, "C5 device, its own adaptive rows (%d .. %d per ray), every 4th kept" % (np.diff(offsets).min(), np.diff(offsets).max())))
    cc.c5_assert(fig)
    # thinning by the library's own outputper keeps the same rows
    rows4, nrows4, _, _ = ngo.trace(pos, d, w, outputper=4, **cc.C5_TRACE)
    o4b, r4b = api.pack_rows(rows4, nrows4, 4)
    assert np.array_equal(o4b, o4) and np.array_equal(r4b.view(np.uint64), r4.view(np.uint64))


def test_device_entry_point_refuses_what_it_cannot_bound():
    """Host pointers, and an offsets[nrays] that names more rows than d_rows' allocation holds: SRT_EINVAL, nothing launched."""
    api.init(0)
    arr, ns = api.surface_array([api.sphere(7e6)])
    L = api.lib()
    host_off = np.array([0, 2], dtype=np.int64)
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    rows = torch.zeros((2, 20), dtype=torch.float64, device="cuda")
    rc = L.srt_crossings_device(ns, arr, 1, host_off.ctypes.data, rows.data_ptr(), None, None, 0, count.data_ptr(), None)
    assert rc == api.SRT_EINVAL and b"not device memory" in L.srt_last_error()
    big = torch.tensor([0, 1 << 40], dtype=torch.int64, device="cuda")
    rc = L.srt_crossings_device(ns, arr, 1, big.data_ptr(), rows.data_ptr(), None, None, 0, count.data_ptr(), None)
    assert rc == api.SRT_EINVAL and b"too many" in L.srt_last_error()
    ev = torch.zeros((1, 20), dtype=torch.float64, device="cuda")
    rc = L.srt_crossings_device(ns, arr, 1, big.data_ptr(), rows.data_ptr(), ev.data_ptr(), None, 1, count.data_ptr(), None)
    assert rc == api.SRT_EINVAL and b"null output" in L.srt_last_error()
