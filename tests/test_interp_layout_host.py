"""CPU: the two device layouts of the interp model in numbers -- srt_interp_layout_bytes, srt_interp_layout_choose (what
SRT_INTERP_AUTO does with hipMemGetInfo's free bytes) and the refusal of an unknown layout number, all pure host code of the
library (include/srt.h)."""
import ctypes as C

import numpy as np
import pytest

from stanford_raytracer_amd import api

EXPANDED, NODES, AUTO = 0, 1, 2


def expanded_table(ns, nx, ny, nz):
    return (nx + 1) * (ny + 1) * (nz + 1) * ns * 64 * 8


def nodes_table(ns, nx, ny, nz):
    return nx * ny * nz * ns * 64


@pytest.mark.parametrize("ns,dims", [(4, (256, 256, 256)), (4, (16, 16, 16)), (1, (2, 3, 4))])
def test_layout_bytes(ns, dims):
    te, pe = api.interp_layout_bytes(ns, *dims, "expanded")
    tn, pn = api.interp_layout_bytes(ns, *dims, "nodes")
    assert te == expanded_table(ns, *dims) and tn == nodes_table(ns, *dims)
    assert pe >= te and pn >= tn
    # creation holds the eight grid arrays beside the table
    arrays = 8 * dims[0] * dims[1] * dims[2] * ns * 8
    assert pe == te + arrays and pn == tn + arrays


def test_the_256_cubed_table_is_the_size_the_trace_tests_pin():
    te, _ = api.interp_layout_bytes(4, 256, 256, 256, EXPANDED)
    tn, _ = api.interp_layout_bytes(4, 256, 256, 256, NODES)
    assert te == 257 ** 3 * 4 * 64 * 8  # tests/test_gpu_trace.py's device_bytes: 34.76 GB
    assert tn == 256 ** 3 * 4 * 64 == 2 ** 32


def test_layout_bytes_takes_null_outputs_and_refuses_auto():
    L = api.lib()
    assert L.srt_interp_layout_bytes(4, 16, 16, 16, NODES, None, None) == 0
    assert L.srt_interp_layout_bytes(4, 16, 16, 16, AUTO, None, None) == api.SRT_EINVAL
    assert b"layout" in L.srt_last_error()
    assert L.srt_interp_layout_bytes(4, 1, 16, 16, NODES, None, None) == api.SRT_EINVAL
    assert L.srt_interp_layout_bytes(5, 16, 16, 16, NODES, None, None) == api.SRT_EINVAL


@pytest.mark.parametrize("ns,dims", [(4, (256, 256, 256)), (4, (16, 16, 16)), (1, (2, 3, 4))])
def test_layout_choose_at_the_edges(ns, dims):
    _, pe = api.interp_layout_bytes(ns, *dims, EXPANDED)
    _, pn = api.interp_layout_bytes(ns, *dims, NODES)
    assert pn < pe
    assert api.interp_layout_choose(ns, *dims, pe) == EXPANDED
    assert api.interp_layout_choose(ns, *dims, pe - 1) == NODES
    assert api.interp_layout_choose(ns, *dims, pn) == NODES
    L = api.lib()
    assert L.srt_interp_layout_choose(ns, *dims, pn - 1) == api.SRT_ENOMEM
    with pytest.raises(api.SrtError, match="srt error -4"):
        api.interp_layout_choose(ns, *dims, pn - 1)


def test_a_512_cubed_grid_on_a_288_gb_card_gets_the_node_table():
    assert api.interp_layout_choose(4, 512, 512, 512, 288 * 10 ** 9) == NODES
    assert api.interp_layout_choose(4, 256, 256, 256, 288 * 10 ** 9) == EXPANDED


def test_an_unknown_layout_is_refused_by_name_before_the_device_is_touched(tmp_path):
    L = api.lib()
    dp = api.dp
    F = np.zeros((2, 2, 2, 1))
    b = np.array([0.0, 1.0, 0.0, 1.0, 0.0, 1.0])
    q, m = np.array([1.0]), np.array([1.0])
    h = C.c_void_p()
    rc = L.srt_model_create_interp_layout(1, 2, 2, 2, b.ctypes.data_as(dp), q.ctypes.data_as(dp), m.ctypes.data_as(dp),
                                          F.ctypes.data_as(dp), None, 2010001, 0, 7, C.byref(h))
    assert rc == api.SRT_EINVAL and b"layout" in L.srt_last_error() and not h.value
    rc = L.srt_model_create_interp_file_layout(str(tmp_path / "none.txt").encode(), 2010001, 0, 7, C.byref(h))
    assert rc == api.SRT_EINVAL and b"layout" in L.srt_last_error() and not h.value
    rc = L.srt_model_create_interp_from_model_layout(None, 0, 2, 2, 2, b.ctypes.data_as(dp), 2010001, 0, 7, C.byref(h))
    assert rc == api.SRT_EINVAL and b"layout" in L.srt_last_error() and not h.value
    assert L.srt_model_create_interp_layout(1, 2, 2, 2, b.ctypes.data_as(dp), q.ctypes.data_as(dp), m.ctypes.data_as(dp),
                                            F.ctypes.data_as(dp), None, 2010001, 0, -1, C.byref(h)) == api.SRT_EINVAL
    with pytest.raises(ValueError, match="layout"):
        api.Model.interp(F, b, q, m, layout="bogus")
    assert L.srt_model_interp_layout(None) == -1
