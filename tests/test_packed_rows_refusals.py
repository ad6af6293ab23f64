"""What a packed row set (offsets[nrays + 1], rows[offsets[nrays]][20]) must satisfy, asked of every entry point that takes one:
srt_crossings, srt_approaches, srt_bin_rays and their _device forms (include/srt.h).  Every refusal is SRT_EINVAL, names its entry
point in front of a colon, and says what is wrong.

The CPU part holds the refusals that are made before a device is looked for.  The GPU part holds the ones that need a device
pointer to judge: one ray, rows[2, 20], offsets int64[2]; no case launches a kernel on bad data."""
import ctypes as C

import numpy as np
import pytest

from stanford_raytracer_amd import api

i64p = C.POINTER(C.c_int64)
HOST = ("srt_crossings", "srt_approaches", "srt_bin_rays")
DEVICE = ("srt_crossings_device", "srt_approaches_device", "srt_bin_rays_device")


def _what(name):
    """The valid leading arguments of entry point `name`: one surface, one observer, or one 2-cell x axis."""
    if "crossings" in name:
        arr, n = api.surface_array([api.sphere(7.0e6)])
        return (n, arr), arr
    if "approaches" in name:
        arr, n = api.observer_array(np.array([[7.0e6, 0.0, 0.0, 1.0e5]]))
        return (n, arr), arr
    p = api.bin_params([api.axis("x", [0.0, 1.0, 2.0])])
    return (C.byref(p),), p


def _host_call(name, nrays, offsets, rows):
    """-> (rc, message) of the host entry point on offsets (a list or None) and rows (an array or None)."""
    L = api.lib()
    lead, keep = _what(name)
    off = None if offsets is None else np.array(offsets, dtype=np.int64)
    po = None if off is None else off.ctypes.data_as(i64p)
    pr = None if rows is None else api._dp(rows)
    n, pe, pm, pd = C.c_int64(), api.dp(), api.ip(), api.dp()
    if name == "srt_crossings":
        rc = L.srt_crossings(*lead, nrays, po, pr, C.byref(n), C.byref(pe), C.byref(pm))
    elif name == "srt_approaches":
        rc = L.srt_approaches(*lead, nrays, po, pr, C.byref(n), C.byref(pe), C.byref(pm), C.byref(pd))
    else:
        pt, ph = i64p(), i64p()
        counters = np.zeros(4, dtype=np.int64)
        rc = L.srt_bin_rays(*lead, nrays, po, pr, None, None, C.byref(pt), C.byref(ph), counters.ctypes.data_as(i64p))
        assert not pt and not ph
    assert not pe and not pm and not pd and n.value == 0  # a refused call hands nothing over
    del keep
    return rc, L.srt_last_error()


def _device_call(name, nrays, d_offsets, d_rows, outputs, capacity=0):
    """-> (rc, message) of the device entry point; outputs = the addresses after d_rows, in the order of include/srt.h, with the
    capacity of the two event calls put where it belongs."""
    L = api.lib()
    lead, keep = _what(name)
    if name == "srt_bin_rays_device":
        rc = L.srt_bin_rays_device(*lead, nrays, d_offsets, d_rows, None, None, *outputs, None)
    else:
        fn = getattr(L, name)
        rc = fn(*lead, nrays, d_offsets, d_rows, *outputs[:-1], capacity, outputs[-1], None)
    del keep
    return rc, L.srt_last_error()


def _refused(name, rc, msg, want):
    assert rc == api.SRT_EINVAL, (name, rc, msg)
    assert msg.startswith(name.encode() + b":"), msg
    assert want in msg, (want, msg)


HOST_CASES = {
    "negative_nrays": (-1, [0], None, b"nrays = -1 is negative"),
    "null_offsets": (1, None, np.zeros((2, 20)), b"null offsets"),
    "offsets_start_at_1": (1, [1, 2], np.zeros((2, 20)), b"offsets[0] = 1"),
    "offsets_decrease": (2, [0, 3, 2], np.zeros((3, 20)), b"offsets decrease at ray 1"),
    "null_rows": (1, [0, 2], None, b"null rows"),
}


@pytest.mark.parametrize("case", sorted(HOST_CASES))
@pytest.mark.parametrize("name", HOST)
def test_host_entry_points_refuse_a_bad_row_set(name, case):
    nrays, offsets, rows, want = HOST_CASES[case]
    rc, msg = _host_call(name, nrays, offsets, rows)
    _refused(name, rc, msg, want)


def _host_outputs(name):
    """Host memory standing in for the outputs: these refusals come before any pointer is looked at."""
    buf = np.zeros(64, dtype=np.int64)
    a = buf.ctypes.data
    if name == "srt_crossings_device":
        return buf, [a, a + 64, a + 128]
    if name == "srt_approaches_device":
        return buf, [a, a + 64, a + 128, a + 192]
    return buf, [a, a + 64, a + 128]


# (binning has no capacity: two cases for it)
DEVICE_CASES = [(name, case) for name in DEVICE for case in ("negative_nrays", "null_d_offsets", "negative_capacity")
                if not (case == "negative_capacity" and name == "srt_bin_rays_device")]


@pytest.mark.parametrize("name,case", DEVICE_CASES)
def test_device_entry_points_refuse_before_any_pointer_is_looked_at(name, case):
    buf, outs = _host_outputs(name)
    off = np.array([0, 2], dtype=np.int64)
    if case == "negative_nrays":
        rc, msg = _device_call(name, -1, off.ctypes.data, None, outs)
        want = b"nrays = -1 is negative"
    elif case == "null_d_offsets":
        rc, msg = _device_call(name, 1, None, None, outs)
        want = b"null d_offsets or d_counters" if name == "srt_bin_rays_device" else b"null d_offsets or d_count"
    else:
        rc, msg = _device_call(name, 1, off.ctypes.data, None, outs, capacity=-1)
        want = b"capacity = -1 is negative"
    _refused(name, rc, msg, want)
    assert not buf.any()


GPU_CASES = {
    "too_many": ([0, 1 << 40], b"too many"),
    # (the allocation is the runtime's: a caching allocator hands out parts of larger ones, so only a count beyond any is told)
    "beyond_the_allocation": ([0, 1 << 28], b"more than the allocation of d_rows holds"),
    "negative_total": ([0, -1], b"is negative"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", DEVICE)
def test_device_entry_points_judge_offsets_and_launch_nothing(name):
    import torch  # before the library's first device call: torch brings its own HIP runtime and must initialise it first

    api.init(0)
    rows = torch.zeros((2, 20), dtype=torch.float64, device="cuda")
    out = torch.zeros(64, dtype=torch.int64, device="cuda")
    a = out.data_ptr()
    if name == "srt_approaches_device":
        outs = [a, a + 160, a + 192, a + 256]  # one event's row, meta, distance; the count
    else:
        outs = [a, a + 160, a + 256]  # one event's row, meta, the count -- or ticks[2], hits[2], counters[4]
    cap = 1
    host_off = np.array([0, 2], dtype=np.int64)
    rc, msg = _device_call(name, 1, host_off.ctypes.data, rows.data_ptr(), outs, cap)
    _refused(name, rc, msg, b"not device memory")
    for case in sorted(GPU_CASES):
        offsets, want = GPU_CASES[case]
        off = torch.tensor(offsets, dtype=torch.int64, device="cuda")
        rc, msg = _device_call(name, 1, off.data_ptr(), rows.data_ptr(), outs, cap)
        _refused(name, rc, msg, want)
    one = torch.tensor([0, 1], dtype=torch.int64, device="cuda")  # one row holds no interval
    rc, msg = _device_call(name, 1, one.data_ptr(), rows.data_ptr(), outs, cap)
    assert rc == api.SRT_OK, msg
    torch.cuda.synchronize()
    assert not out.cpu().numpy().any()  # the count or the counters are zero, and nothing was launched
