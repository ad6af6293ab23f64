"""GPU (-m gpu): traced rays binned onto a grid on the device (include/srt.h) -- srt_bin_rays and srt_bin_rays_device on the cases
of tests/binning_cases.py (B2 .. B6): ticks, hits and counters EQUAL AS INTEGERS to the host build of the same header
(tests/native/binning_host.cpp) and to the numpy restatement, under the precondition stated there; the launch shapes at which a
row-per-lane pass can go wrong; both accumulation paths and the grid sizes either side of their threshold (4096 cells: a
block-private copy in LDS up to there, global atomics beyond); and the path trace -> pack -> damping -> binning that never
leaves the device."""
import ctypes as C

import numpy as np
import pytest
import torch  # before the library's first call: torch brings its own HIP runtime and must initialise it first

import binning_cases as bc
import crossings_cases as cc
from stanford_raytracer_amd import api, parallel, workloads as wl
from stanford_raytracer_amd.device_batch import DeviceBatch

pytestmark = pytest.mark.gpu
if torch.cuda.is_available():
    torch.cuda.init()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return bc.build_host(tmp_path_factory.mktemp("bnh"))


def _cuda(a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def device_bin(offsets, rows, axes, nsub, quantum=bc.QUANTUM, row_weight=None, ray_weight=None, out=None):
    """srt_bin_rays_device on uploaded buffers; `out` = a previous call's device tensors to accumulate into
    -> ((ticks, hits, counters) flat on the host, the device tensors)"""
    api.init(0)
    d_off = _cuda(offsets, np.int64)
    d_rows = _cuda(np.asarray(rows).reshape(-1, 20), np.float64)
    if d_rows.shape[0] == 0:
        d_rows = torch.zeros((1, 20), dtype=torch.float64, device="cuda")
    dev = parallel.bin_rays_device(d_rows, d_off, axes, nsub, quantum, _cuda(row_weight, np.float64), _cuda(ray_weight, np.float64), out=out)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy().ravel() for t in dev), dev


def lib_bin(offsets, rows, axes, nsub, quantum=bc.QUANTUM, row_weight=None, ray_weight=None):
    api.init(0)
    o = api.bin_rays(offsets, rows, axes, nsub, quantum, row_weight, ray_weight)
    assert o["ticks"].shape == bc.shape_of(axes) == o["hits"].shape == o["sum"].shape
    assert np.array_equal(o["sum"], o["ticks"].astype(np.float64) * quantum)
    return o["ticks"].ravel(), o["hits"].ravel(), o["counters"]


def all_four(host, offsets, rows, axes, nsub, label, quantum=bc.QUANTUM, row_weight=None, ray_weight=None, clear=True):
    """the host-buffer call, the device call, the host build and numpy give the same integers -> them"""
    if clear:
        bc.assert_clear_of_edges(offsets, rows, axes, nsub, row_weight, ray_weight)
    want = bc.reference(offsets, rows, axes, nsub, quantum, row_weight, ray_weight)
    bc.assert_same(bc.host_bin(host, offsets, rows, axes, nsub, quantum, row_weight, ray_weight), want, label + ": host build")
    bc.assert_same(lib_bin(offsets, rows, axes, nsub, quantum, row_weight, ray_weight), want, label + ": srt_bin_rays")
    bc.assert_same(device_bin(offsets, rows, axes, nsub, quantum, row_weight, ray_weight)[0], want, label + ": srt_bin_rays_device")
    bc.check_identities(*want, nsub, offsets)
    return want


def test_b2_the_definition_on_every_kind_and_every_nsub(host):
    offsets, rows = bc.b2_rows()
    for kind in range(8):
        for naxes in (1, 2, 3):
            got = all_four(host, offsets, rows, bc.b2_axes(kind, naxes), 8, "B2 kind %d, %d axes" % (kind, naxes))
            assert np.count_nonzero(got[1]) >= 2
    for nsub in (1, 8, 64):
        got = all_four(host, offsets, rows, bc.b2_log_l(), nsub, "B2 log L, nsub %d" % nsub)
        assert np.count_nonzero(got[1]) >= 8


def test_b3_samples_exactly_on_edges(host):
    ex = np.array([0.0, 1024.0, 2048.0, 4096.0])
    y = 8192.0
    pts = [((512.0, y, 0.0), (1536.0, y, 0.0)), ((-512.0, y, 0.0), (512.0, y, 0.0)), ((3584.0, y, 0.0), (4608.0, y, 0.0)),
           ((2048.0, y, 0.0), (2048.0, y, 64.0))]
    offsets, rows = bc.b3_rows(pts)
    got = all_four(host, offsets, rows, [(bc.X, ex)], 1, "B3", clear=False)  # (kinds 0 .. 2 are exact: the samples ARE on edges)
    assert got[1].tolist() == [1, 1, 1] and got[2].tolist() == [4, 0, 3, 1]
    one = [(bc.X, np.array([0.0, 4096.0])), (bc.Y, np.array([8192.0, 8193.0])), (bc.Z, np.array([0.0, 64.0]))]
    got = all_four(host, offsets, rows, one, 1, "B3 one cell", clear=False)
    assert got[1].tolist() == [3]
    o, r = bc.b3_rows([((0.0, 0.0, 2.0 * 2 ** 23), (0.0, 0.0, 4.0 * 2 ** 23))])
    got = all_four(host, o, r, [(bc.L, np.array([1.0, 2.0, 1e300]))], 1, "B3 z axis, L", clear=False)
    assert got[1].tolist() == [0, 0] and got[2].tolist() == [1, 0, 0, 1]
    got = all_four(host, o, r, [(bc.R, np.array([0.0, 3.0 * 2 ** 23, 5.0 * 2 ** 23]))], 1, "B3 z axis, r", clear=False)
    assert got[1].tolist() == [0, 1]


def test_b4_nothing_from_nothing(host):
    rays, axes = bc.b4_base()
    for name, col, value in (("nan_pos", 2, np.nan), ("inf_t", 0, np.inf), ("nan_vgrel", 8, np.nan)):
        spoilt = [rays[0].copy(), rays[1]]
        spoilt[0][2, col] = value
        got = all_four(host, *cc.pack(spoilt), axes, 4, name)
        assert got[2].tolist()[:2] == [6, 2]
    r = rays[0].copy()
    r[1, 0] = r[0, 0]
    assert all_four(host, *cc.pack([r, rays[1]]), axes, 4, "t1 == t0")[2].tolist()[:2] == [7, 1]
    got = all_four(host, *cc.pack([rays[0][:1], rays[0][1:2], rays[1][:1]]), axes, 4, "one-row rays")
    assert not got[1].any() and got[2].tolist() == [0, 0, 0, 0]
    got = all_four(host, *cc.pack([rays[0], np.zeros((0, 20)), rays[1]]), axes, 4, "empty ray between two")
    assert got[2].tolist()[:2] == [8, 0]
    got = all_four(host, np.zeros(1, dtype=np.int64), np.zeros((0, 20)), axes, 4, "nrays = 0")
    assert not got[1].any() and got[2].tolist() == [0, 0, 0, 0]
    offsets, rows = cc.pack(rays)
    rw = np.ones(10)
    rw[2] = np.nan
    assert all_four(host, offsets, rows, axes, 4, "NaN row weight", row_weight=rw)[2].tolist()[:2] == [6, 2]
    for w, skipped in ((2.0 ** 36, 4), (2.0 ** 35.99, 0), (np.inf, 4)):
        got = all_four(host, offsets, rows, axes, 4, "ray weight %g" % w, ray_weight=np.array([1.0, w]))
        assert got[2].tolist()[:2] == [8 - skipped, skipped]
    rw = np.ones(10)
    rw[7] = 2.0 ** 37
    assert all_four(host, offsets, rows, axes, 4, "one heavy row", row_weight=rw)[2].tolist()[:2] == [6, 2]


def test_b5_weights_and_b6_additivity(host):
    offsets, rows = bc.b2_rows()
    axes = bc.b2_log_l()
    out = {}
    for name, (rw, yw) in bc.b5_weights(offsets).items():
        out[name] = all_four(host, offsets, rows, axes, 8, "B5 " + name, row_weight=rw, ray_weight=yw)
    bc.assert_same(out["ones"], out["none"], "NULL weights are ones")
    assert (out["negative_and_zero"][0] < 0).any()
    # B6: two calls into the same device buffers equal one call; so does a permutation of the rays
    rw, yw = bc.b5_weights(offsets)["both"]
    (o1, r1), (o2, r2) = bc.split_rays(offsets, rows, 4)
    k = int(offsets[4])
    _, dev = device_bin(o1, r1, axes, 8, row_weight=rw[:k], ray_weight=yw[:4])
    got, _ = device_bin(o2, r2, axes, 8, row_weight=rw[k:], ray_weight=yw[4:], out=dev)
    bc.assert_same(got, out["both"], "two calls")
    perm = np.random.default_rng(4).permutation(len(offsets) - 1)
    o, r, prw, pyw = bc.permute_rays(offsets, rows, perm, rw, yw)
    bc.assert_same(device_bin(o, r, axes, 8, row_weight=prw, ray_weight=pyw)[0], out["both"], "permuted")
    # either output may be absent
    api.init(0)
    p = api.bin_params(axes, 8)
    d_off, d_rows = _cuda(offsets, np.int64), _cuda(rows, np.float64)
    for which in (0, 1):
        t = torch.zeros(60, dtype=torch.int64, device="cuda")
        c = torch.zeros(4, dtype=torch.int64, device="cuda")
        rc = api.lib().srt_bin_rays_device(C.byref(p), len(offsets) - 1, d_off.data_ptr(), d_rows.data_ptr(), None, None,
                                           t.data_ptr() if which == 0 else None, t.data_ptr() if which == 1 else None, c.data_ptr(), None)
        torch.cuda.synchronize()
        assert rc == 0 and np.array_equal(t.cpu().numpy(), out["none"][which]) and np.array_equal(c.cpu().numpy(), out["none"][2])


def zigzag(total):
    """total rows 0.01 s and 300 m of x apart, z alternating between -1000 and +1000 m with a turning point at every row"""
    r = np.zeros((total, 20))
    i = np.arange(total)
    r[:, 0] = 0.01 * i
    r[:, 1] = 7.0e6 + 300.0 * i
    r[:, 2] = 40.0 * i
    r[:, 3] = np.where(i % 2 == 0, -1000.0, 1000.0)
    r[:, 7] = 300.0 / 0.01 / cc.C_LIGHT
    r[:, 8] = 40.0 / 0.01 / cc.C_LIGHT
    r[:, 16:20] = 1e9
    return r


def layouts(total):
    """name -> ray lengths that sum to `total`"""
    out = {"one_ray": [total], "rays_of_2": [2] * (total // 2) + [1] * (total % 2)}
    if total > 40:  # a ray boundary inside a wave, and an empty ray at it
        out["boundary_in_wave"] = [37, 0, total - 37]
    return out


# every lane of a wave in the same cell / every lane in a different cell (an interval covers 300 m of x: cells of 300 m, their
# edges 37 m off the rows, hold one interval's samples each but for the piece that straddles)
SAME_CELL = [(bc.X, np.array([0.0, 1.0e9])), (bc.Z, np.array([-2000.0, 2000.0]))]
OWN_CELL = [(bc.X, 7.0e6 - 37.0 + 300.0 * np.arange(0, 133))]


@pytest.mark.parametrize("total", [1, 2, 63, 64, 65, 130])
def test_packed_totals_and_ray_layouts(host, total):
    rows = zigzag(total)
    for name, lens in layouts(total).items():
        offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        intervals = int(sum(max(k - 1, 0) for k in lens))
        for axes, label in ((SAME_CELL, "same cell"), (OWN_CELL, "own cells")):
            want = bc.reference(offsets, rows, axes, 8)
            got, _ = device_bin(offsets, rows, axes, 8)
            bc.assert_same(got, want, "%d rows, %s, %s" % (total, name, label))
            bc.assert_same(bc.host_bin(host, offsets, rows, axes, 8), want, "host build")
            assert got[2].tolist() == [intervals, 0, 8 * intervals, 0]
        assert got[1].max() <= 8 and np.count_nonzero(got[1]) >= intervals  # own cells: an interval's samples in its own cell(s)
        rw = np.linspace(0.5, 1.5, total)
        bc.assert_same(device_bin(offsets, rows, SAME_CELL, 3, row_weight=rw)[0], bc.reference(offsets, rows, SAME_CELL, 3, row_weight=rw), name)


def test_both_accumulation_paths_and_the_threshold_between_them(host):
    """4096 cells (64 x 64) go through the block-private LDS copy, 4097 (17 x 241) and 8192 (64 x 64 x 2) through global atomics;
    more than one block on either path (more than 256 rows).  The 64 x 64 x 2 grid's upper z cells hold nothing and its lower
    ones are the 64 x 64 map cell for cell."""
    offsets, rows, _, _ = bc.b1_cartesian(seed=8, nlines=80)
    assert offsets[-1] > 512
    ex, ey = np.linspace(-4.03, 3.91, 65) * bc.R_E, np.linspace(-3.07, 5.02, 65) * bc.R_E
    rw = np.random.default_rng(1).uniform(0.1, 2.0, int(offsets[-1]))
    lds = [(bc.X, ex), (bc.Y, ey)]
    over = [(bc.X, np.linspace(-4.03, 3.91, 18) * bc.R_E), (bc.Y, np.linspace(-3.07, 5.02, 242) * bc.R_E)]
    extra = lds + [(bc.Z, np.array([-1.5, 1.5, 40.0]) * bc.R_E)]
    assert [int(np.prod(bc.shape_of(a))) for a in (lds, over, extra)] == [4096, 4097, 8192]
    a = all_four(host, offsets, rows, lds, 8, "4096 cells, LDS path", row_weight=rw)
    b = all_four(host, offsets, rows, over, 8, "4097 cells, global path", row_weight=rw)
    c = all_four(host, offsets, rows, extra, 8, "8192 cells, global path", row_weight=rw)
    assert np.array_equal(c[0][:4096], a[0]) and np.array_equal(c[1][:4096], a[1]) and not c[0][4096:].any() and not c[1][4096:].any()
    assert np.array_equal(a[2], c[2]) and a[0].sum() == b[0].sum() == c[0].sum() and np.count_nonzero(a[1]) > 300
    # the small end: one cell, and a grid whose axes fill the LDS path's edge budget (1024 x 4)
    all_four(host, offsets, rows, [(bc.R, np.array([0.0, 100.0 * bc.R_E]))], 8, "one cell")
    all_four(host, offsets, rows, [(bc.X, np.linspace(-4.03, 3.91, 1025) * bc.R_E), (bc.Y, np.linspace(-3.07, 5.02, 5) * bc.R_E)], 8, "1024 x 4")
    # the large end of the global path's edges: 1024 x 1024
    big = [(bc.X, np.linspace(-4.03, 3.91, 1025) * bc.R_E), (bc.Y, np.linspace(-3.07, 5.02, 1025) * bc.R_E)]
    bc.assert_same(device_bin(offsets, rows, big, 8)[0], bc.reference(offsets, rows, big, 8), "1024 x 1024")


NGO_FIXED = dict(fixedstep=1, dt0=2e-3, tmax=0.4, maxsteps=200, del_=1e-4, outputper=4)


@pytest.fixture(scope="module")
def ngo(tmp_path_factory):
    api.init(0)
    cfg = tmp_path_factory.mktemp("bn") / "newray.in"
    cfg.write_text(wl.NEWRAY_PLASMAPAUSE)
    return api.Model.ngo(str(cfg))


def test_trace_pack_damp_bin_without_leaving_the_device(ngo):
    """16 Ngo rays, fixed step, outputper 4: trace -> srt_pack_rows_device -> srt_damping_device -> magnitude^2 packed as the
    row weight -> srt_bin_rays_device, all on device buffers; integer-equal to api.bin_rays of the downloaded rows and weights,
    to bin_rays_padded, and to the same rays through trace_packed(segment_rows = 4)."""
    pos, d, w = wl.appendix_b_rays()
    p = api.make_params(**NGO_FIXED)
    le, lat = bc.b7_map_axes()
    axes = [api.axis("L", le), api.axis_maglat(lat)]
    dev = torch.device("cuda", 0)
    batch = DeviceBatch(ngo, p, pos, d, w, dev)
    o = batch.launch()
    packed, offsets = parallel.pack_rows_device(o["rows"], o["nrows"], p.outputper)
    n, slots = o["rows"].shape[:2]
    qs, ms = ngo.species()
    mag, rate = torch.empty((n, slots), dtype=torch.float64, device=dev), torch.empty((n, slots), dtype=torch.float64, device=dev)
    flag = torch.empty((n, slots), dtype=torch.int32, device=dev)
    d_w0 = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64)).to(dev)
    dpar = api.damping_params()
    st = torch.cuda.current_stream(dev)
    api._check(api.lib().srt_damping_device(C.byref(dpar), len(qs), api._dp(api._f64(qs)), api._dp(api._f64(ms)), slots, p.outputper, n,
                                            o["rows"].data_ptr(), o["nrows"].data_ptr(), d_w0.data_ptr(), rate.data_ptr(), mag.data_ptr(),
                                            flag.data_ptr(), st.cuda_stream))
    kept = offsets[1:] - offsets[:-1]
    roww = (mag * mag)[torch.arange(slots, device=dev)[None, :] < kept[:, None]].contiguous()
    yw = torch.linspace(0.5, 2.0, n, dtype=torch.float64, device=dev)
    ticks, hits, counters = parallel.bin_rays_device(packed, offsets, axes, 8, row_weight=roww, ray_weight=yw)
    torch.cuda.synchronize()
    assert ticks.shape == (12, 16) and int(counters[0]) > 0 and int(hits.sum()) == int(counters[2]) > 0
    got = (ticks.cpu().numpy().ravel(), hits.cpu().numpy().ravel(), counters.cpu().numpy())
    off_h = offsets.cpu().numpy()
    rows_h = packed[:int(off_h[-1])].cpu().numpy()
    a = api.bin_rays(off_h, rows_h, axes, 8, row_weight=roww.cpu().numpy(), ray_weight=yw.cpu().numpy())
    bc.assert_same(got, (a["ticks"], a["hits"], a["counters"]), "api.bin_rays of the downloaded rows")
    mag_h = mag.cpu().numpy()
    b = api.bin_rays_padded(o["rows"].cpu().numpy(), o["nrows"].cpu().numpy(), p.outputper, axes, 8, row_weight_padded=mag_h * mag_h,
                            ray_weight=yw.cpu().numpy())
    bc.assert_same(got, (b["ticks"], b["hits"], b["counters"]), "bin_rays_padded")
    off_s, rows_s, _, _, _ = ngo.trace_packed(pos, d, w, 4, params=p)
    assert np.array_equal(off_s, off_h)
    s = api.bin_rays(off_s, rows_s, axes, 8, row_weight=roww.cpu().numpy(), ray_weight=yw.cpu().numpy())
    bc.assert_same(got, (s["ticks"], s["hits"], s["counters"]), "segmented trace")
    # and the numpy restatement, where the inputs meet its precondition
    ax = [(bc.L, le), (bc.SINLAT, np.sin(lat))]
    bc.assert_clear_of_edges(off_h, rows_h, ax, 8)
    bc.assert_same(got, bc.reference(off_h, rows_h, ax, 8, row_weight=roww.cpu().numpy(), ray_weight=yw.cpu().numpy()), "numpy")
    print("16 Ngo rays, fixed step, outputper 4: %d kept rows, counters %s, identical through the device path, the host-buffer "
          "path, the padded path, a segmented trace and numpy" % (off_h[-1], got[2].tolist()))


def test_device_entry_point_refuses_what_it_cannot_bound():
    """Host pointers, an offsets[nrays] that names more rows than d_rows' allocation holds, and both outputs NULL: SRT_EINVAL,
    nothing launched."""
    api.init(0)
    p = api.bin_params([api.axis("x", [0.0, 1.0, 2.0])])
    L = api.lib()
    host_off = np.array([0, 2], dtype=np.int64)
    out = torch.zeros(8, dtype=torch.int64, device="cuda")
    rows = torch.zeros((2, 20), dtype=torch.float64, device="cuda")
    t, h, c = out.data_ptr(), out.data_ptr() + 16, out.data_ptr() + 32
    rc = L.srt_bin_rays_device(C.byref(p), 1, host_off.ctypes.data, rows.data_ptr(), None, None, t, h, c, None)
    assert rc == api.SRT_EINVAL and b"not device memory" in L.srt_last_error()
    big = torch.tensor([0, 1 << 40], dtype=torch.int64, device="cuda")
    rc = L.srt_bin_rays_device(C.byref(p), 1, big.data_ptr(), rows.data_ptr(), None, None, t, h, c, None)
    assert rc == api.SRT_EINVAL and b"too many" in L.srt_last_error()
    # (the allocation is the runtime's: a caching allocator hands out parts of larger ones, so only a count beyond any is told)
    some = torch.tensor([0, 1 << 28], dtype=torch.int64, device="cuda")
    rc = L.srt_bin_rays_device(C.byref(p), 1, some.data_ptr(), rows.data_ptr(), None, None, t, h, c, None)
    assert rc == api.SRT_EINVAL and b"more than the allocation of d_rows holds" in L.srt_last_error()
    rc = L.srt_bin_rays_device(C.byref(p), 1, some.data_ptr(), rows.data_ptr(), None, None, None, None, c, None)
    assert rc == api.SRT_EINVAL and b"both outputs" in L.srt_last_error()
    torch.cuda.synchronize()
    assert not out.cpu().numpy().any()  # nothing was launched
