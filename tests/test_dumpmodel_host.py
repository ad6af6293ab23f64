"""CPU: the host half of dumpmodel -- the SM <-> MAG rotations against the reference's xform_double, the dump file's writer
and reader against the files the reference's dumpmodel wrote, and srt_dump_model's refusals (by name, before the device is
touched).  Goldens: tests/golden/make_dumpmodel_golden.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR

FIXTURES = ("dump_ngo_5x1x4", "dump_interp_4x3x2", "dump_scattered_3x3x1", "dump_simple3d_sm_6x1x5", "dump_simple3d_mag_6x1x5")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN_DIR, "dumpmodel_golden.npz"))


@pytest.fixture(scope="module")
def settings():
    return json.load(open(os.path.join(GOLDEN_DIR, "dumpmodel_settings.json")))


def parse_dump(path):
    v = np.array(open(path).read().split(), dtype=np.float64)
    nspec, nx, ny, nz = (int(t) for t in v[:4])
    return nspec, v[4:10], v[10:].reshape(nz, ny, nx, 4 * nspec + 3)


def test_sm_to_mag_matches_xform_double(gold):
    """Both directions at all 6 x 206 = 1236 points: every component within 1e-14 |x| of the Fortran (seven plane rotations of
    two products and one sum each, plus the angles' last-bit differences between maths libraries)."""
    from stanford_raytracer_amd import api

    x = gold["xf_x"]
    norm = np.linalg.norm(x, axis=1, keepdims=True)
    assert x.shape == (206, 3) and len(gold["xf_dates"]) == 6
    worst, equal, total = 0.0, 0, 0
    for (yd, ms), fwd, inv in zip(gold["xf_dates"], gold["xf_sm_to_mag"], gold["xf_mag_to_sm"]):
        a = api.sm_to_mag(x, int(yd), int(ms))
        b = api.sm_to_mag(x, int(yd), int(ms), inverse=True)
        for got, ref in ((a, fwd), (b, inv)):
            e = np.abs(got - ref) / norm
            worst = max(worst, float(e.max()))
            equal += int(np.sum(got == ref))
            total += got.size
    print("sm_to_mag vs xform_double: worst %.3g |x|, %d / %d components bit-equal" % (worst, equal, total))
    assert worst <= 1e-14


def test_sm_to_mag_round_trip(gold):
    from stanford_raytracer_amd import api

    x = gold["xf_x"]
    norm = np.linalg.norm(x, axis=1, keepdims=True)
    for yd, ms in gold["xf_dates"]:
        back = api.sm_to_mag(api.sm_to_mag(x, int(yd), int(ms)), int(yd), int(ms), inverse=True)
        assert np.max(np.abs(back - x) / norm) <= 2e-14
    # a rotation: lengths are kept, and MAG is not SM
    m = api.sm_to_mag(x, 2010001, 0)
    assert np.allclose(np.linalg.norm(m, axis=1), norm[:, 0], rtol=1e-14, atol=0)
    assert np.max(np.abs(m - x) / norm) > 0.1


def test_sm_to_mag_refuses_bad_arguments():
    from stanford_raytracer_amd import api

    x = np.zeros(3)
    out = np.zeros(3)
    rc = api.lib().srt_sm_to_mag(2010001, 0, 2, 1, api._dp(x), api._dp(out))
    assert rc == api.SRT_EINVAL and b"inverse" in api.lib().srt_last_error()
    assert api.sm_to_mag(np.zeros((0, 3)), 2010001, 0).shape == (0, 3)


@pytest.mark.parametrize("name", FIXTURES)
def test_writer_reproduces_the_reference_files(name, tmp_path):
    """The golden's parsed values, written by srt_dump_file_write, are the golden's bytes."""
    from stanford_raytracer_amd import api

    src = os.path.join(GOLDEN_DIR, name + ".txt")
    nspec, bounds, f = parse_dump(src)
    out = str(tmp_path / "out.txt")
    api.write_dump_file(out, f, bounds)
    assert open(out, "rb").read() == open(src, "rb").read()


@pytest.mark.parametrize("name", FIXTURES)
def test_reader_round_trips(name, tmp_path):
    from stanford_raytracer_amd import api

    src = os.path.join(GOLDEN_DIR, name + ".txt")
    nspec, bounds, f = parse_dump(src)
    d = api.read_dump_file(src)
    assert d["nspec"] == nspec and np.array_equal(d["bounds"], bounds) and d["f"].shape == f.shape
    assert np.array_equal(d["f"], f)
    out = str(tmp_path / "again.txt")
    api.write_dump_file(out, d["f"], d["bounds"])
    assert np.array_equal(api.read_dump_file(out)["f"], f)


def test_reader_refuses_a_count_that_disagrees_with_the_header(tmp_path):
    from stanford_raytracer_amd import api

    lines = open(os.path.join(GOLDEN_DIR, "dump_ngo_5x1x4.txt")).read().splitlines(keepends=True)
    cut = tmp_path / "cut.txt"
    cut.write_text("".join(lines[:-1]))  # one line short
    with pytest.raises(api.SrtError, match=r"holds 379 values.*announces 380"):
        api.read_dump_file(str(cut))
    hdr = tmp_path / "hdr.txt"
    hdr.write_text("%10d%10d%10d%10d\n" % (4, 5, 2, 4) + "".join(lines[1:]))  # ny = 2: twice the values announced
    with pytest.raises(api.SrtError, match=r"holds 380 values.*announces 760"):
        api.read_dump_file(str(hdr))
    with pytest.raises(api.SrtError, match="nspec"):
        bad = tmp_path / "nspec.txt"
        bad.write_text("%10d%10d%10d%10d\n" % (9, 5, 1, 4) + "".join(lines[1:]))
        api.read_dump_file(str(bad))


def test_dump_model_refuses_by_name_before_the_device():
    """nx = 0, empty bounds on an axis of two nodes, mag_coords = 2: each SRT_EINVAL with its own text, and none of them needs a
    model or a device to be told so."""
    from stanford_raytracer_amd import api

    L = api.lib()
    assert L.srt_dump_model.argtypes == [C.c_void_p, C.c_int, C.c_int, C.c_int, api.dp, C.c_int, api.dp]
    f = np.zeros(19 * 8)
    b = np.array([1.0, 2.0, 0.0, 0.0, 1.0, 2.0])

    def call(nx, ny, nz, bounds, mag):
        rc = L.srt_dump_model(None, nx, ny, nz, api._dp(bounds), mag, api._dp(f))
        return rc, (L.srt_last_error() or b"").decode()

    rc, msg = call(0, 1, 2, b, 0)
    assert rc == api.SRT_EINVAL and "at least 1 node" in msg
    rc, msg = call(2, 2, 2, b, 0)  # miny = maxy with ny = 2
    assert rc == api.SRT_EINVAL and "empty bounds on the y axis" in msg
    rc, msg = call(2, 1, 2, b, 2)
    assert rc == api.SRT_EINVAL and "mag_coords = 2" in msg
    rc, msg = call(65536, 65536, 1, np.array([0.0, 1.0, 0.0, 1.0, 0.0, 0.0]), 0)
    assert rc == api.SRT_EINVAL and "2^31 - 1 nodes" in msg
    rc, msg = call(2, 1, 2, b, 0)  # all well but the model
    assert rc == api.SRT_EINVAL and "null model" in msg


def test_no_cpu_fallback_for_the_dump():
    """Without a GPU there is nothing to dump with: the model the dump needs cannot be made, and says why."""
    from stanford_raytracer_amd import api

    if api.lib().srt_init(0) == api.SRT_OK:  # (the library's own answer: it is the library's device the dump would need)
        pytest.skip("GPU present")
    with pytest.raises(api.SrtError, match="no HIP device"):
        api.Model.simple3d(4.0).dump(5, 1, 4, [1e7, 2e7, 0, 0, -1e7, 1e7])
