"""CPU: the host side of the trace in segments (include/srt.h): the packed .ray writer gives the padded writer's bytes, the
segment count follows srt_rows_per_ray, and every refusal arrives by name before a device is looked for."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR
from stanford_raytracer_amd import api

GOLDENS = ["config1_outputper25.ray", "driver_interp_adaptive.ray"]


def offsets_of(kept):
    return np.concatenate([[0], np.cumsum(kept)]).astype(np.int64)


def both_writers(tmp_path, ray, sel, raynum0=1, append=False, tag="w"):
    """the rays `sel` of a read .ray file through write_ray_file (padded) and write_ray_file_packed -> the two files' bytes"""
    rows, nrows = api.padded_rows(ray)
    off = offsets_of(ray["kept"])
    species = (ray["nspec"], ray["qs"], ray["ms"])
    kept = ray["kept"][sel]
    packed = np.concatenate([ray["rows"][off[i]:off[i + 1]] for i in sel]) if len(sel) else np.zeros((0, 20))
    # outputper = 1: a ray of `kept` records is a ray of `kept` rows, as padded_rows says
    p = api.make_params(maxsteps=max(int(rows.shape[1]), 1), outputper=1)
    a, b = tmp_path / (tag + "_padded.ray"), tmp_path / (tag + "_packed.ray")
    if append:
        a.write_bytes(b"first line\n")
        b.write_bytes(b"first line\n")
    api.write_ray_file(str(a), species, p, ray["w0"][sel], rows[sel] if len(sel) else np.zeros((0, rows.shape[1], 20)),
                       nrows[sel], ray["stopcond"][sel], raynum0=raynum0, append=append)
    api.write_ray_file_packed(str(b), species, ray["w0"][sel], offsets_of(kept), packed, ray["stopcond"][sel],
                              raynum0=raynum0, append=append)
    return a.read_bytes(), b.read_bytes()


@pytest.mark.parametrize("name", GOLDENS)
def test_packed_writer_gives_the_padded_writers_bytes(tmp_path, name):
    path = os.path.join(GOLDEN_DIR, name)
    ray = api.read_ray_file(path)
    n = len(ray["kept"])
    assert n == 16  # (config[0]'s rays keep 5 records each, the adaptive run's between 1 and many: the offsets matter there)
    a, b = both_writers(tmp_path, ray, np.arange(n))
    assert a == b and len(a) > 0
    # an empty set: an empty file from both
    a, b = both_writers(tmp_path, ray, np.arange(0), tag="empty")
    assert a == b == b""
    # a ray of one record
    one = dict(ray)
    one["kept"] = ray["kept"].copy()
    one["kept"][:] = 1
    off = offsets_of(ray["kept"])
    one["rows"] = ray["rows"][off[:-1]]
    a, b = both_writers(tmp_path, one, np.array([3]), tag="one")
    assert a == b and a.count(b"\n") == 1
    # ray numbers from 7, and appended behind what the file holds
    a, b = both_writers(tmp_path, ray, np.array([2, 5, 6]), raynum0=7, tag="seven")
    assert a == b and a[:10] == b"%10d" % 7 and a.rstrip(b"\n").split(b"\n")[-1][:10] == b"%10d" % 9
    a, b = both_writers(tmp_path, ray, np.array([0, 1]), append=True, tag="append")
    assert a == b and a.startswith(b"first line\n") and a.count(b"\n") == 1 + int(ray["kept"][:2].sum())


def test_packed_writer_refuses_bad_offsets(tmp_path):
    species = (4, np.ones(4), np.ones(4))
    rows = np.zeros((3, 20))
    for off, word in (([1, 2, 3], "start at 0"), ([0, 2, 1], "decrease")):
        with pytest.raises(api.SrtError, match=word):
            api.write_ray_file_packed(str(tmp_path / "x.ray"), species, np.ones(2), off, rows, np.zeros(2, dtype=np.int32))


def test_segment_count_follows_rows_per_ray():
    L = api.lib()
    p = api.make_params(maxsteps=40, outputper=3)
    slots = L.srt_rows_per_ray(C.byref(p))
    assert slots == 14
    assert api.trace_segment_count(p, 4) == 4
    assert api.trace_segment_count(p, slots) == 1
    assert api.trace_segment_count(p, 1) == slots
    assert api.trace_segment_count(p, 0) == 0 and api.trace_segment_count(p, -3) == 0
    p = api.make_params(maxsteps=2000, outputper=1)
    assert api.trace_segment_count(p, 64) == 32 and api.trace_segment_count(p, 1999) == 2


def last_error():
    return (api.lib().srt_last_error() or b"").decode()


def test_refusals_arrive_by_name_before_the_device_is_touched():
    """Null handles and null buffers throughout: each refusal below is given before either is looked at."""
    L = api.lib()
    p = api.make_params(maxsteps=40, outputper=3)  # 14 slots
    run = C.c_void_p()

    def primitive(nrays, segment_rows, segment, queue):
        return L.srt_trace_segment_device(None, C.byref(p), nrays, None, None, None, segment_rows, segment, queue, 0, None, None,
                                          None, None, None, None)

    def opened(nrays, segment_rows):
        return L.srt_trace_run_open(None, C.byref(p), nrays, None, None, None, segment_rows, C.byref(run))

    for call in (lambda n, N: primitive(n, N, 0, None), opened):
        assert call(8, 0) == api.SRT_EINVAL and "segment_rows=0" in last_error()
        assert call(8, -1) == api.SRT_EINVAL and "segment_rows=-1" in last_error()
        assert call(8, 15) == api.SRT_EINVAL and "segment_rows=15 exceeds the 14 rows" in last_error()
        assert call(1 << 31, 4) == api.SRT_EINVAL and "fewer than 2^31 rays" in last_error()
    assert primitive(8, 4, 1, None) == api.SRT_EINVAL and "segment 1 without a queue" in last_error()
    assert primitive(8, 4, 0, C.c_void_p(64)) == api.SRT_EINVAL and "d_queue must be NULL" in last_error()
    assert primitive(8, 4, -1, None) == api.SRT_EINVAL and "segment=-1" in last_error()
    assert primitive(8, 4, 0, None) == api.SRT_EINVAL and "null argument" in last_error()  # all well but the buffers
    bad = api.make_params(maxsteps=0)
    assert L.srt_trace_run_open(None, C.byref(bad), 8, None, None, None, 4, C.byref(run)) == api.SRT_EINVAL and "maxsteps" in last_error()
    L.srt_trace_run_close(None)  # allowed


def test_no_cpu_fallback_for_the_run():
    """All well but the model: without a GPU the run says that there is none; with one, that the model is missing."""
    L = api.lib()
    p = api.make_params(maxsteps=40, outputper=3)
    run = C.c_void_p()
    have_gpu = L.srt_init(0) == api.SRT_OK
    rc = L.srt_trace_run_open(None, C.byref(p), 8, None, None, None, 4, C.byref(run))
    assert not run.value
    if have_gpu:
        assert rc == api.SRT_EINVAL and "null model" in last_error()
    else:
        assert rc == api.SRT_EDEVICE and "no HIP device" in last_error()
