"""GPU (-m gpu): the trace in segments (include/srt.h).  A launch set traced as a sequence of launches that keep N rows per ray
each, pausing and resuming the rays in between, gives the rows, row counts and stop codes of Model.trace BIT FOR BIT: equality
below is array_equal on the uint64 view of the rows.  The one exception is the scattered model, whose defined behaviour is
tested at the end."""
import ctypes as C

import numpy as np
import pytest
import torch  # before the library's first call: torch brings its own HIP runtime and must initialise it first (test_primitive)

import model_ladder as ml
from conftest import DELS
from stanford_raytracer_amd import api, workloads as wl

pytestmark = pytest.mark.gpu
if torch.cuda.is_available():
    torch.cuda.init()

PARMOD = [3.0, -25.0, 1.5, -4.0, 0.4, 0.5, 0.3, 0.3, 0.4, 0.6]
# the issue's mix of outcomes on the interp model: oracle stop codes {0: 51, 1: 7, 2: 4, 3: 1, 6: 67}, 22 distinct row counts
MIX = dict(fixedstep=0, dt0=1e-3, dtmax=0.1, maxerr=5e-4, tmax=0.05, maxsteps=40, del_=1e-6)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def kept_of(nrows, outputper, slots):
    return np.minimum((nrows + outputper - 1) // outputper, slots)


def packed_of(rows, nrows, outputper):
    """Model.trace's padded result -> offsets, packed rows"""
    kept = kept_of(nrows, outputper, rows.shape[1])
    off = np.concatenate([[0], np.cumsum(kept)]).astype(np.int64)
    return off, np.concatenate([rows[i, :kept[i]] for i in range(len(kept))]) if len(kept) else np.zeros((0, 20))


def assert_same(model, rays, N, **kw):
    """trace_packed with segment_rows = N against trace of the same inputs -> (the unsegmented result, segments seen)"""
    pos, d, w = rays
    p = api.make_params(**kw)
    base = model.trace(pos, d, w, params=p)
    off, rows = packed_of(base[0], base[1], p.outputper)
    segs = list(model.trace_segments(pos, d, w, N, params=p))
    assert len(segs) <= api.trace_segment_count(p, N)
    got = api.assemble_segments(len(w), segs)  # (what trace_packed does with them)
    assert np.array_equal(got[2], base[1]), "nrows differ on rays %s" % np.nonzero(got[2] != base[1])[0][:8]
    assert np.array_equal(got[3], base[2]), "stop codes differ on rays %s" % np.nonzero(got[3] != base[2])[0][:8]
    assert np.array_equal(got[0], off)
    assert np.array_equal(bits(got[1]), bits(rows)), "%d of %d rows differ" % (np.any(bits(got[1]) != bits(rows), axis=1).sum(), len(rows))
    assert got[4] == base[3] == sum(s["steps"] for s in segs)
    return base, segs


@pytest.fixture(scope="module")
def rays130():
    return wl.launch_set(130, 31)


@pytest.mark.parametrize("policy", [0, 1])
@pytest.mark.parametrize("N", [8, 1, 40])
def test_mix_of_outcomes_is_bit_equal(gpu_models, rays130, N, policy):
    base, segs = assert_same(gpu_models["interp"], rays130, N, first_attempt_policy=policy, **MIX)
    stops = set(np.unique(base[2]).tolist())
    assert {0, 6} <= stops and len(stops) >= 3 and len(np.unique(base[1])) >= 9, (stops, np.unique(base[1]))
    assert len(segs) == {8: 5, 1: 40, 40: 1}[N]
    if N == 40:
        assert np.all(segs[0]["stopcond"] != api.RUNNING)  # one segment, no pause
    if N == 1:  # every row a boundary: a ray that does not stop at its launch point pauses there, its first attempt still to come
        assert np.all(segs[0]["nrows"] == 1) and segs[0]["steps"] == 0
        assert np.array_equal(segs[0]["stopcond"] == api.RUNNING, base[1] > 1)


def test_ray_order_and_fixed_step_are_bit_equal(gpu_models, rays130):
    assert_same(gpu_models["interp"], rays130, 8, ray_order=1, **MIX)
    base, _ = assert_same(gpu_models["interp"], rays130, 8, **dict(MIX, fixedstep=1))
    assert {1, 6} <= set(np.unique(base[2]).tolist())


@pytest.mark.parametrize("outputper,N,nseg", [(3, 4, 4), (64, 1, 1)])
def test_ragged_outputper(gpu_models, rays130, outputper, N, nseg):
    """outputper 3, N 4: S = 12, 14 slots, a last segment of 4 row indices; outputper 64: one kept row."""
    _, segs = assert_same(gpu_models["interp"], rays130, N, outputper=outputper, **MIX)
    assert len(segs) == nseg


@pytest.mark.parametrize("name", ["ngo", "ngoducts"])
@pytest.mark.parametrize("fixedstep", [0, 1])
def test_ngo_kernels(gpu_models, rays130, name, fixedstep):
    assert_same(gpu_models[name], rays130, 8, **dict(MIX, fixedstep=fixedstep, del_=DELS[name]))


@pytest.mark.parametrize("field", ["igrf", "t04"])
def test_ngo_field_options(cfgfiles, rays130, field):
    m = api.Model.ngo(cfgfiles["ngo"])
    if field == "igrf":
        m.set_field(use_igrf=1)
    else:
        m.set_field(use_igrf=0, use_tsyganenko=1, parmod=PARMOD)
    rays = tuple(a[:64] for a in rays130)
    assert_same(m, rays, 8, **dict(MIX, del_=1e-4))


def test_node_table_layout(grid16, rays130):
    F, b, qs, ms = grid16
    assert_same(api.Model.interp(F, b, qs, ms, layout="nodes"), rays130, 8, **MIX)


@pytest.mark.parametrize("kind", ["ngo3d", "simple3d"])
def test_models_5_and_6(cfgfiles, kind):
    m = api.Model.ngo3d(cfgfiles["ngo"], 4.0) if kind == "ngo3d" else api.Model.simple3d(4.0)
    assert_same(m, wl.launch_set(64, 31), 8, **MIX)


def test_model_7():
    m = api.Model.at64thch(4, PARMOD)
    assert_same(m, wl.launch_set(4, 31), 1, **dict(MIX, fixedstep=1, maxsteps=3, del_=1e-4))


def test_lane_independence(gpu_models, rays130):
    """the segmented run on permuted rays is the permuted result"""
    m = gpu_models["interp"]
    pos, d, w = rays130
    a = m.trace_packed(pos, d, w, 8, **MIX)
    perm = np.random.default_rng(1).permutation(len(w))
    b = m.trace_packed(pos[perm], d[perm], w[perm], 8, **MIX)
    assert np.array_equal(b[2], a[2][perm]) and np.array_equal(b[3], a[3][perm])
    want = np.concatenate([a[1][a[0][i]:a[0][i + 1]] for i in perm])
    assert np.array_equal(bits(b[1]), bits(want))


def test_primitive(gpu_models, rays130):
    """srt_trace_segment_device and srt_running_rays_device by hand: what a segment leaves behind."""
    m = gpu_models["interp"]
    L = api.lib()
    pos, d, w = rays130
    n, N = len(w), 8
    p = api.make_params(outputper=1, **MIX)
    S = N * p.outputper
    nseg = api.trace_segment_count(p, N)
    base = m.trace(pos, d, w, params=p)
    dev = torch.device("cuda:0")
    d_pos = torch.from_numpy(np.ascontiguousarray(pos.T)).to(dev)
    d_dir = torch.from_numpy(np.ascontiguousarray(d.T)).to(dev)
    d_w = torch.from_numpy(np.ascontiguousarray(w)).to(dev)
    state = torch.zeros((n, api.STATE), dtype=torch.float64, device=dev)
    rows = torch.zeros((n, N, api.ROW), dtype=torch.float64, device=dev)
    nrows = torch.full((n,), -7, dtype=torch.int32, device=dev)
    stop = torch.full((n,), -7, dtype=torch.int32, device=dev)
    cnt = torch.zeros(4, dtype=torch.int64, device=dev)
    queue = torch.zeros(n, dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    steps, nq, ids = 0, n, np.arange(n)
    for s in range(nseg + 1):  # one segment beyond the count: it must find no work
        before = (nrows.cpu().numpy().copy(), stop.cpu().numpy().copy(), state.cpu().numpy().copy())
        api._check(L.srt_trace_segment_device(m.h, C.byref(p), n, d_pos.data_ptr(), d_dir.data_ptr(), d_w.data_ptr(), N, s,
                                              queue.data_ptr() if s else None, nq, state.data_ptr(), rows.data_ptr(),
                                              nrows.data_ptr(), stop.data_ptr(), cnt.data_ptr(), None))
        api._check(L.srt_running_rays_device(n, stop.data_ptr(), queue.data_ptr(), count.data_ptr(), None))
        torch.cuda.synchronize()
        h_n, h_s = nrows.cpu().numpy(), stop.cpu().numpy()
        outside = np.setdiff1d(np.arange(n), ids)
        assert np.array_equal(h_n[outside], before[0][outside]) and np.array_equal(h_s[outside], before[1][outside])
        assert np.array_equal(bits(state.cpu().numpy()[outside]), bits(before[2][outside]))
        paused = h_s == api.RUNNING
        assert np.all(paused[outside] == False)  # noqa: E712  (rays outside the queue stopped earlier)
        assert np.all(h_n[paused] == (s + 1) * S)
        assert np.all(h_s[ids][~paused[ids]] >= 0) and np.all(h_n[ids][~paused[ids]] <= (s + 1) * S)
        steps += int(cnt.cpu().numpy()[1])
        nq = int(count.cpu().numpy()[0])
        ids = queue.cpu().numpy()[:nq].copy()
        assert np.array_equal(ids, np.nonzero(paused)[0])  # ascending
        if s >= nseg - 1:
            assert nq == 0, "segment %d of %d leaves %d rays running" % (s, nseg, nq)
    assert steps == base[3]
    assert np.array_equal(nrows.cpu().numpy(), base[1]) and np.array_equal(stop.cpu().numpy(), base[2])


def test_scattered_defined_behaviour(gpu_models, oracle_scattered):
    """The scattered model forgets a lane's candidate block at a claim, and the block orders its sums: segment 0 is bit-equal;
    behind the first pause the positions stay within what the ORACLE itself does under a 1e-9 shift of the launch points (the
    bar is that figure once: the disturbance, a reordered sum, lies six orders below that shift); nrows and stopcond are equal.
    The figures of this run are printed before they are asserted."""
    m = gpu_models["scattered"]
    pos, d, w = wl.launch_set(64, 31)
    pos = pos * 0.9
    kw = dict(fixedstep=1, dt0=1e-3, dtmax=0.1, maxerr=5e-4, tmax=0.05, maxsteps=13, del_=DELS["scattered"])
    N, at = 4, (5, 9, 12)
    p = api.make_params(**kw)
    base = m.trace(pos, d, w, params=p)
    got = m.trace_packed(pos, d, w, N, params=p)
    off, rows = packed_of(base[0], base[1], 1)
    assert np.array_equal(got[2], base[1]) and np.array_equal(got[3], base[2]) and np.array_equal(got[0], off)
    padded = np.zeros_like(base[0])
    for i in range(len(w)):
        padded[i, :off[i + 1] - off[i]] = got[1][off[i]:off[i + 1]]
    assert np.array_equal(bits(padded[:, :N]), bits(base[0][:, :N])), "segment 0 is not bit-equal"
    rays = np.concatenate([pos, d, w[:, None]], axis=1)
    _, yard = ml.oracle_yardstick(oracle_scattered, rays, kw, at, 13)
    mine = {r: ml.divergence(padded, got[2], base[0], base[1], r, slice(1, 4)) for r in at}
    print("scattered, segmented against unsegmented, position divergence at rows %s: %s; the oracle's own under a 1e-9 shift: %s"
          % (at, ["%.3g" % mine[r] for r in at], ["%.3g" % yard[r] for r in at]))
    for r in at:
        assert mine[r] <= yard[r], "row %d: %.3g over the oracle's own %.3g" % (r, mine[r], yard[r])
