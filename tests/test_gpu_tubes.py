"""GPU (-m gpu): ray-tube sections along kept rows on the device (include/srt.h, "ray tubes") -- srt_tubes and srt_tubes_device on
the cases and at the bars of tests/tubes_cases.py (T1 .. T5, T8), against the host build of the same header
(tests/native/tubes_host.cpp) and the numpy restatement; the launch shapes at which a row-per-lane pass can go wrong; and the path
trace -> pack -> tubes that never leaves the device (T6).

Sections and flags equal the host build bit for bit through both entry points: only +, -, x, / and sqrt with contraction off reach
an output.  The equality is asserted in every case."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch  # before the library's first call: torch brings its own HIP runtime and must initialise it first

import tubes_cases as tc
from conftest import ROOT
from stanford_raytracer_amd import api, parallel, workloads as wl
from stanford_raytracer_amd.device_batch import DeviceBatch

pytestmark = pytest.mark.gpu
if torch.cuda.is_available():
    torch.cuda.init()

SRC = os.path.join(ROOT, "tests", "native", "tubes_host.cpp")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("tbh") / "libtbh.so")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-ffp-contract=off", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, SRC])
    L = C.CDLL(so)
    L.tbh_tubes.argtypes = [C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
    return L


def host_tubes(L, offsets, rows, nb):
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    rows = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, 20)
    nb = np.ascontiguousarray(nb, dtype=np.int64).reshape(-1, 2)
    total = int(offsets[-1])
    section, flag = np.zeros((total + 1, 4)), np.zeros(total + 1, dtype=np.int32)
    why = C.create_string_buffer(200)
    pad = nb if len(nb) else np.zeros((1, 2), dtype=np.int64)
    assert L.tbh_tubes(len(offsets) - 1, pad.ctypes.data, offsets.ctypes.data, rows.ctypes.data, section.ctypes.data, flag.ctypes.data, why, 200) == 0
    return section[:total], flag[:total]


def device_tubes(offsets, rows, nb):
    """srt_tubes_device on uploaded buffers -> (section, flag) on the host; beyond the rows the outputs must be as handed in"""
    api.init(0)
    total = int(offsets[-1])
    d_off = torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.int64)).cuda()
    d_rows = torch.zeros((total + 3, 20), dtype=torch.float64, device="cuda")
    if total:
        d_rows[:total] = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, 20)[:total]).cuda()
    section, flag = parallel.tubes_device(d_rows, d_off, nb)
    torch.cuda.synchronize()
    assert section.shape == (total + 3, 4) and torch.isnan(section[total:]).all() and (flag[total:] == 1).all()
    return section[:total].cpu().numpy(), flag[:total].cpu().numpy()


def both_paths(host, offsets, rows, nb, label):
    """srt_tubes and srt_tubes_device give the same bits, and they are the host build's -> (section, flag)"""
    api.init(0)
    section, flag = api.tubes(offsets, rows, nb)
    hs, hf = host_tubes(host, offsets, rows, nb)
    tc.assert_same_bits(section, flag, hs, hf, label + ", srt_tubes against the host build")
    s2, f2 = device_tubes(offsets, rows, nb)
    tc.assert_same_bits(s2, f2, hs, hf, label + ", srt_tubes_device against the host build")
    return section, flag


def test_t1_t2_t3_t8_at_the_bars_and_bit_equal_to_the_host_build(host):
    offsets, rows, nb, vel = tc.t1_case()
    section, flag = both_paths(host, offsets, rows, nb, "T1 device")
    tc.check_against_truth(section, flag, *tc.t1_truth(offsets, rows, nb, vel), tc.K_STRAIGHT, "T1 straight rays, device")
    offsets, rows, nb = tc.t2_case()
    section, flag = both_paths(host, offsets, rows, nb, "T2 device")
    tc.check_against_truth(section, flag, *tc.t2_truth(offsets, rows, nb), tc.K_CUBIC, "T2 cubic arcs, device")
    for k in (0, 7, 40):
        offsets, rows, nb, want, wflag = tc.t3_case(k)
        section, flag = both_paths(host, offsets, rows, nb, "T3 device")
        assert np.array_equal(flag, wflag) and np.array_equal(section[:3], want[:3]) and np.all(np.isnan(section[3:]))
        o2, r2, nb2, want2, _ = tc.t3_case(k, swap=True)
        swapped, _ = both_paths(host, o2, r2, nb2, "T3 device, swapped")
        assert np.array_equal(swapped[:3], -section[:3])
    for shift, want in ((0, tc.OK), (-1, tc.NO_ROW), (1, tc.NO_ROW)):
        offsets, rows, nb, _ = tc.t3_one_row_neighbour(shift)
        section, flag = both_paths(host, offsets, rows, nb, "T3 device, one-row neighbour")
        assert flag[0] == want and (shift != 0 or section[0].tolist() == [-4.0, -9.0, 12.5, 12.5])
    # T8: the section of a fan at launch
    rng = np.random.default_rng(3)
    n, delta = 24, 50e3
    dir0 = np.concatenate([np.eye(3), rng.normal(size=(n - 3, 3))])
    pos0 = rng.normal(size=(n, 3)) * 0.8e7
    pos, dr, w, nb = api.tube_fan(pos0, dir0, np.ones(n), delta_pos=delta)
    rows = np.zeros((3 * n, tc.ROW))
    rows[:, 1:4] = pos
    rows[:, 7:10] = 0.3 * dr / np.linalg.norm(dr, axis=1)[:, None]
    section, flag = both_paths(host, np.arange(3 * n + 1, dtype=np.int64), rows, nb, "T8 device")
    d = dir0 / np.linalg.norm(dir0, axis=1)[:, None]
    err = np.linalg.norm(section[0::3, :3] - 0.5 * delta * delta * d, axis=1)
    bar = tc.K_STRAIGHT * 2.0 ** -52 * (np.linalg.norm(pos0, axis=1) + delta) * 2 * delta + 14 * 2.0 ** -52 * 0.5 * delta * delta
    assert np.all(flag[0::3] == 0) and np.all(err <= bar)


def test_t4_flags_and_their_order(host):
    for name, (offsets, rows, nb, want) in sorted(tc.t4_cases().items()):
        section, flag = both_paths(host, offsets, rows, nb, "T4 device, " + name)
        n0 = int(offsets[1]) if len(offsets) > 1 else 0
        if want is not None:
            assert flag[:n0].tolist() == want, (name, flag[:n0].tolist())
        assert np.all(flag[n0:] == tc.NO_TUBE)
        tc.assert_same_bits(section, flag, *tc.reference(offsets, rows, nb), label="T4 device against the restatement, " + name)
    # every ray without a tube; section alone and flag alone
    offsets, rows = tc.pack(tc.t4_base())
    api.init(0)
    d_off, d_rows = torch.from_numpy(offsets).cuda(), torch.from_numpy(rows).cuda()
    L = api.lib()
    nb = np.ascontiguousarray(tc.T4_NB)
    pnb = nb.ctypes.data_as(C.POINTER(C.c_int64))
    hs, hf = host_tubes(host, offsets, rows, nb)
    sec = torch.zeros((len(rows), 4), dtype=torch.float64, device="cuda")
    flg = torch.full((len(rows),), -7, dtype=torch.int32, device="cuda")
    api._check(L.srt_tubes_device(3, pnb, d_off.data_ptr(), d_rows.data_ptr(), sec.data_ptr(), None, None))
    api._check(L.srt_tubes_device(3, pnb, d_off.data_ptr(), d_rows.data_ptr(), None, flg.data_ptr(), None))
    torch.cuda.synchronize()
    tc.assert_same_bits(sec.cpu().numpy(), flg.cpu().numpy(), hs, hf, "one output at a time")


@pytest.mark.parametrize("total", tc.T5_TOTALS)
def test_t5_launch_shapes(host, total):
    for name, (lens, nb) in tc.t5_layouts(total).items():
        offsets, rows = tc.fan(lens, seed=total)
        section, flag = both_paths(host, offsets, rows, nb, "T5 device %d rows, %s" % (total, name))
        if total >= 63:
            assert np.any(flag == tc.OK), name


def test_t5_search_depth_distinct_neighbours_and_permutation(host):
    offsets, rows = tc.fan([40, 1, 1025], seed=3)
    both_paths(host, offsets, rows, np.array([[2, 1], [-1, -1], [0, 1]], dtype=np.int64), "T5 device, 1 and 1025 rows")
    offsets, rows = tc.fan([40, 1025, 300], seed=4)
    section, flag = both_paths(host, offsets, rows, tc.ring(3), "T5 device, 1025 rows")
    assert np.all(flag == tc.OK)
    offsets, rows = tc.fan([1] * 130, seed=5, shared_time=True)
    section, flag = both_paths(host, offsets, rows, tc.ring(130), "T5 device, rays of one row")
    assert np.all(flag == tc.OK)
    lens = [5, 0, 9, 3, 1, 17, 8, 2, 30, 4]
    offsets, rows = tc.fan(lens, seed=6)
    nb = tc.ring(len(lens))
    nb[4] = -1
    section, flag = both_paths(host, offsets, rows, nb, "T5 device, before the permutation")
    perm = np.random.default_rng(9).permutation(len(lens))
    o2, r2, nb2, src = tc.permuted(offsets, rows, nb, perm)
    s2, f2 = both_paths(host, o2, r2, nb2, "T5 device, permuted")
    tc.assert_same_bits(s2, f2, section[src], flag[src], "T5 device, permutation")


@pytest.fixture(scope="module")
def ngo(tmp_path_factory):
    api.init(0)
    cfg = tmp_path_factory.mktemp("tb") / "newray.in"
    cfg.write_text(wl.NEWRAY_PLASMAPAUSE)
    return api.Model.ngo(str(cfg))


def test_t6_trace_pack_tubes_without_leaving_the_device(ngo):
    """The 16 Appendix-B rays and their companions (api.tube_fan, 50 km), fixed step, every row kept: trace -> srt_pack_rows_device
    -> srt_tubes_device on device buffers, on all rows (every lookup a node hit) and on the thinned rows of T6 (gathered on the
    device; every lookup inside an interval).  Both equal api.tubes of the downloaded rows bit for bit; tubes_padded and the same
    rays through trace_packed(segment_rows = 4) give the same; the conditions of T6 hold on the device's own trajectories."""
    pos, d, w, nb = api.tube_fan(*wl.appendix_b_rays(), delta_pos=tc.T6_DELTA_POS)
    p = api.make_params(outputper=1, **tc.T6_TRACE)
    batch = DeviceBatch(ngo, p, pos, d, w, torch.device("cuda", 0))
    o = batch.launch()
    packed, offsets = parallel.pack_rows_device(o["rows"], o["nrows"], p.outputper)
    section, flag = parallel.tubes_device(packed, offsets, nb)
    off_h = offsets.cpu().numpy()
    total = int(off_h[-1])
    # the thinned set, gathered on the device from the row counts alone
    keep, lens, kept = [], [], []
    phase = np.zeros(len(w), dtype=np.int64)
    phase[1::3], phase[2::3] = 1, 2
    for r in range(len(w)):
        idx = np.arange(phase[r], int(off_h[r + 1] - off_h[r]), tc.T6_STRIDE)
        kept.append(idx)
        keep.append(off_h[r] + idx)
        lens.append(len(idx))
    d_keep = torch.from_numpy(np.concatenate(keep)).cuda()
    o4 = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    packed4, offsets4 = packed[d_keep].contiguous(), torch.from_numpy(o4).cuda()
    section4, flag4 = parallel.tubes_device(packed4, offsets4, nb)
    torch.cuda.synchronize()
    rows_h, rows4_h = packed[:total].cpu().numpy(), packed4.cpu().numpy()
    s_h, f_h = api.tubes(off_h, rows_h, nb)
    tc.assert_same_bits(section[:total].cpu().numpy(), flag[:total].cpu().numpy(), s_h, f_h, "device path against api.tubes, all rows")
    s4_h, f4_h = api.tubes(o4, rows4_h, nb)
    tc.assert_same_bits(section4.cpu().numpy(), flag4.cpu().numpy(), s4_h, f4_h, "device path against api.tubes, thinned rows")
    o4b, r4b, keptb = tc.t6_thin(off_h, rows_h, nb)
    assert np.array_equal(o4b, o4) and np.array_equal(tc.bits(r4b), tc.bits(rows4_h))
    # the padded form packs on the host first
    s_p, f_p = api.tubes_padded(o["rows"].cpu().numpy(), o["nrows"].cpu().numpy(), p.outputper, nb)
    tc.assert_same_bits(s_p, f_p, s_h, f_h, "tubes_padded")
    # segmented, as one packed set
    off_s, rows_s, _, _, _ = ngo.trace_packed(pos, d, w, 4, params=p)
    assert np.array_equal(off_s, off_h)
    s_s, f_s = api.tubes(off_s, rows_s, nb)
    tc.assert_same_bits(s_s, f_s, s_h, f_h, "trace_packed(segment_rows = 4)")
    # the conditions of T6 on the device's trajectories
    chord, flag_c = tc.reference(o4, rows4_h, nb, chord=True)
    fig = tc.t6_figures(off_h, nb, s_h, f_h, kept, o4, s4_h, f4_h, chord, flag_c)
    print(tc.t6_report(fig, "T6 device, Ngo rows (%d .. %d per ray), %g km" % (np.diff(off_h).min(), np.diff(off_h).max(), tc.T6_DELTA_POS / 1e3)))
    tc.t6_assert(fig)


def test_device_entry_point_refuses_what_it_cannot_bound():
    """Host pointers, an offsets[nrays] beyond 2^31 - 2 rows, a row without d_rows: SRT_EINVAL, nothing launched."""
    api.init(0)
    L = api.lib()
    nb = np.array([[-1, -1]], dtype=np.int64)
    pnb = nb.ctypes.data_as(C.POINTER(C.c_int64))
    host_off = np.array([0, 2], dtype=np.int64)
    rows = torch.zeros((2, 20), dtype=torch.float64, device="cuda")
    sec = torch.zeros((2, 4), dtype=torch.float64, device="cuda")
    flg = torch.zeros(2, dtype=torch.int32, device="cuda")
    rc = L.srt_tubes_device(1, pnb, host_off.ctypes.data, rows.data_ptr(), sec.data_ptr(), flg.data_ptr(), None)
    assert rc == api.SRT_EINVAL and b"not device memory" in L.srt_last_error()
    big = torch.tensor([0, 1 << 40], dtype=torch.int64, device="cuda")
    rc = L.srt_tubes_device(1, pnb, big.data_ptr(), rows.data_ptr(), sec.data_ptr(), flg.data_ptr(), None)
    assert rc == api.SRT_EINVAL and b"too many" in L.srt_last_error()
    one = torch.tensor([0, 1], dtype=torch.int64, device="cuda")
    rc = L.srt_tubes_device(1, pnb, one.data_ptr(), None, sec.data_ptr(), flg.data_ptr(), None)
    assert rc == api.SRT_EINVAL and b"d_rows is null" in L.srt_last_error()
