"""GPU (-m gpu): srt_dump_model / Model.dump -- the reference's dumpmodel on the device.

The condition on the values: the dump of a node is BIT-EQUAL to plasma_params at the node's coordinates (numpy's i*del + min,
the Fortran's linspace), with mag_coords to plasma_params at api.sm_to_mag of them -- on handles of every kind and with every
field option.  Against the reference: the five files its own dumpmodel wrote (tests/golden/make_dumpmodel_golden.py), at the
parity ladder's G0 bars.  Model 5 has no golden of the reference's dumpmodel (its adapter needs the card file's plasmapause and
the ladder's own goldens cover its densities, tests/test_gpu_ngo3d.py): it is held against plasma_params only."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR
from stanford_raytracer_amd import workloads as wl

pytestmark = pytest.mark.gpu
R_E = wl.R_E
PARMOD = [3.0, -25.0, 1.5, -4.0, 0.4, 0.5, 0.3, 0.3, 0.4, 0.6]
BOUNDS = np.array([1.5, 4.5, -1.0, 1.2, -1.2, 1.3]) * R_E
SHAPES = [(5, 1, 4), (1, 1, 1), (65, 1, 1), (1, 64, 1), (4, 3, 2)]
KINDS = ["ngo", "interp", "interp_nodes", "scattered", "ngo3d", "simple3d", "at64thch"]
FIXTURES = ("dump_ngo_5x1x4", "dump_interp_4x3x2", "dump_scattered_3x3x1", "dump_simple3d_sm_6x1x5", "dump_simple3d_mag_6x1x5")


def node_points(nx, ny, nz, bounds):
    """[nz*ny*nx, 3] in the file's order (x fastest), formed as dumpmodel.f95:219-237 forms them: (/ (ind) /)*del + min, an axis
    of one node at its minimum."""
    ax = []
    for n, lo, hi in ((nx, bounds[0], bounds[1]), (ny, bounds[2], bounds[3]), (nz, bounds[4], bounds[5])):
        ax.append(np.array([lo]) if n == 1 else np.arange(n, dtype=np.float64) * ((hi - lo) / (n - 1.0)) + lo)
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)


def as_dump(pp, nspec, shape):
    """plasma_params' [n,19] = qs(4) Ns(4) ms(4) nus(4) B0(3) in the file's order [nz,ny,nx,4 nspec+3]."""
    nx, ny, nz = shape
    cols = [4 * g + s for g in range(4) for s in range(nspec)] + [16, 17, 18]
    return pp[:, cols].reshape(nz, ny, nx, 4 * nspec + 3)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.fixture(scope="module")
def models(gpu_models, cfgfiles, grid16):
    from stanford_raytracer_amd import api

    F, b, qs, ms = grid16
    return {"ngo": gpu_models["ngo"], "interp": gpu_models["interp"], "interp_nodes": api.Model.interp(F, b, qs, ms, layout="nodes"),
            "scattered": gpu_models["scattered"], "ngo3d": api.Model.ngo3d(cfgfiles["ngo"], 4.0),
            "simple3d": api.Model.simple3d(4.0), "at64thch": api.Model.at64thch(4, PARMOD)}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("kind", KINDS)
def test_dump_is_bit_equal_to_plasma_params(models, kind, shape):
    m = models[kind]
    nspec = 3 if kind == "at64thch" else 4
    assert m.nspec == nspec
    f = m.dump(*shape, BOUNDS)
    assert f.shape == (shape[2], shape[1], shape[0], 4 * nspec + 3)
    ref = as_dump(m.plasma_params(node_points(*shape, BOUNDS)), nspec, shape)
    assert np.array_equal(bits(f), bits(ref))
    qs, ms = m.species()
    assert np.all(f[..., 0:nspec] == qs[:nspec]) and np.all(f[..., 2 * nspec:3 * nspec] == ms[:nspec])
    assert np.all(f[..., 3 * nspec:4 * nspec] == 0.0)  # nus
    assert np.all(np.isfinite(f)) and np.all(f[..., nspec:2 * nspec] > 0)


def test_a_one_node_axis_sits_at_its_minimum(models):
    m = models["simple3d"]
    b2 = BOUNDS.copy()
    b2[3] = 7.0 * R_E  # maxy: never read with ny = 1
    assert np.array_equal(bits(m.dump(5, 1, 4, BOUNDS)), bits(m.dump(5, 1, 4, b2)))
    b3 = BOUNDS.copy()
    b3[3] = b3[2]  # and an empty y range is no error there
    assert np.array_equal(bits(m.dump(5, 1, 4, BOUNDS)), bits(m.dump(5, 1, 4, b3)))
    b4 = BOUNDS.copy()
    b4[2] = 0.3 * R_E
    assert not np.array_equal(m.dump(5, 1, 4, BOUNDS), m.dump(5, 1, 4, b4))


@pytest.mark.parametrize("field", ["igrf", "t04"])
def test_dump_with_field_options(field):
    from stanford_raytracer_amd import api

    m = api.Model.simple3d(4.0, yearday=2012180, msec=43200000)
    if field == "igrf":
        m.set_field(use_igrf=1)
    else:
        m.set_field(use_igrf=0, use_tsyganenko=1, parmod=PARMOD)
    dip = api.Model.simple3d(4.0, yearday=2012180, msec=43200000).dump(5, 1, 4, BOUNDS)
    for shape in SHAPES:
        f = m.dump(*shape, BOUNDS)
        assert np.array_equal(bits(f), bits(as_dump(m.plasma_params(node_points(*shape, BOUNDS)), 4, shape)))
    f = m.dump(5, 1, 4, BOUNDS)
    assert np.array_equal(f[..., 0:16], dip[..., 0:16]) and not np.array_equal(f[..., 16:19], dip[..., 16:19])


@pytest.mark.parametrize("kind", ["simple3d", "at64thch", "ngo"])
def test_mag_coords_is_plasma_params_at_sm_to_mag(models, kind):
    from stanford_raytracer_amd import api

    m = models[kind]
    nspec = m.nspec
    for shape in ((5, 1, 4), (65, 1, 1)):
        f = m.dump(*shape, BOUNDS, mag_coords=True)
        x = api.sm_to_mag(node_points(*shape, BOUNDS), 2010001, 0)
        assert np.array_equal(bits(f), bits(as_dump(m.plasma_params(x), nspec, shape)))
        # MAG is SM turned about the dipole axis: the field's x and y components move on every model, the densities on
        # those that know a local time or a field line (not on model 1, a function of r and the dipole latitude)
        sm = m.dump(*shape, BOUNDS)
        assert not np.array_equal(f[..., 4 * nspec:], sm[..., 4 * nspec:])
        if kind != "ngo":
            assert not np.array_equal(f[..., nspec:2 * nspec], sm[..., nspec:2 * nspec])


def test_mag_coords_uses_the_models_date():
    from stanford_raytracer_amd import api

    m = api.Model.simple3d(4.0, yearday=2001093, msec=43200000)
    f = m.dump(6, 1, 5, BOUNDS, mag_coords=True)
    x = api.sm_to_mag(node_points(6, 1, 5, BOUNDS), 2001093, 43200000)
    assert np.array_equal(bits(f), bits(as_dump(m.plasma_params(x), 4, (6, 1, 5))))


def model_of(st, cfgfiles, grid16, pointsfile):
    from stanford_raytracer_amd import api

    fl = dict(a[2:].split("=") for a in st["flags"])
    yd, ms = st["yearday"], st["milliseconds_day"]
    if st["modelnum"] == 1:
        m = api.Model.ngo(cfgfiles["ngo"], yd, ms)
    elif st["modelnum"] == 3:
        F, b, qs, msp = grid16
        m = api.Model.interp(F, b, qs, msp, yearday=yd, msec=ms)
    elif st["modelnum"] == 4:
        m = api.Model.scattered_file(pointsfile, yd, ms, window_scale=float(fl["scattered_interp_window_scale"]),
                                     order=int(fl["scattered_interp_order"]), exact=int(fl["scattered_interp_exact"]),
                                     local_window_scale=float(fl["scattered_interp_local_window_scale"]))
    else:
        m = api.Model.simple3d(float(fl["kp"]), yd, ms)
    if int(fl["use_igrf"]) or int(fl["use_tsyganenko"]):
        m.set_field(use_igrf=int(fl["use_igrf"]), use_tsyganenko=int(fl["use_tsyganenko"]))
    return m, int(fl.get("mag_coords", 0))


@pytest.mark.parametrize("name", FIXTURES)
def test_dump_against_the_reference_files(name, cfgfiles, grid16, pointsfile):
    """The ladder's G0 bars: densities within max(1e-11, 10 x the node's recorded sensitivity) relative, B0 within 2e-7 |B|;
    qs and ms equal the file's printed digits; no node is left out."""
    from stanford_raytracer_amd import api

    st = json.load(open(os.path.join(GOLDEN_DIR, "dumpmodel_settings.json")))[name]
    sens = np.load(os.path.join(GOLDEN_DIR, "dumpmodel_golden.npz"))["sens_" + name]
    ref = api.read_dump_file(os.path.join(GOLDEN_DIR, st["file"]))
    m, mag = model_of(st, cfgfiles, grid16, pointsfile)
    nspec = ref["nspec"]
    assert np.array_equal(ref["bounds"], np.array(st["bounds"])) and m.nspec == nspec
    f = m.dump(*st["n"], ref["bounds"], mag_coords=bool(mag))
    assert f.shape == ref["f"].shape and np.all(np.isfinite(f))
    eN = np.max(np.abs(f[..., nspec:2 * nspec] - ref["f"][..., nspec:2 * nspec]) / ref["f"][..., nspec:2 * nspec], axis=-1)
    bar = np.maximum(1e-11, 10.0 * sens)
    B, Br = f[..., 4 * nspec:], ref["f"][..., 4 * nspec:]
    eB = np.linalg.norm(B - Br, axis=-1) / np.linalg.norm(Br, axis=-1)
    print("%s: density worst %.3g (worst ratio to its bar %.3g), B0 worst %.3g |B|" % (name, eN.max(), np.max(eN / bar), eB.max()))
    assert np.all(eN <= bar)
    assert np.all(eB <= 2e-7)
    printed = np.array([float("%.15e" % v) for v in f[0, 0, 0]])
    for lo in (0, 2 * nspec):  # qs, ms
        assert np.array_equal(np.broadcast_to(printed[lo:lo + nspec], ref["f"][..., lo:lo + nspec].shape), ref["f"][..., lo:lo + nspec])
    assert np.all(ref["f"][..., 3 * nspec:4 * nspec] == 0.0) and np.all(f[..., 3 * nspec:4 * nspec] == 0.0)


def test_model_5_through_the_library(cfgfiles):
    """The 3-D Ngo model on model 1's bounds with fixed_mlt, against plasma_params: the executable refuses modelnum 5 and the
    reference's dumpmodel has no golden here, so the library call is what there is to hold."""
    from stanford_raytracer_amd import api

    st = json.load(open(os.path.join(GOLDEN_DIR, "dumpmodel_settings.json")))["dump_ngo_5x1x4"]
    m = api.Model.ngo3d(cfgfiles["ngo"], 4.0, fixed_mlt=2.0)
    f = m.dump(*st["n"], st["bounds"])
    assert np.array_equal(bits(f), bits(as_dump(m.plasma_params(node_points(*st["n"], st["bounds"])), 4, tuple(st["n"]))))
    assert np.all(f[..., 4:8] > 0)


@pytest.mark.parametrize("kind", ["scattered", "at64thch"])
def test_lanes_are_independent(models, kind):
    """130 nodes (26 x 5 x 1) dumped whole and as rows 0-1, 2-3 and 4: the same nodes in other lanes of other waves, the same
    bits.  The y nodes are powers of two apart, so that every piece forms exactly the coordinates of the whole."""
    m = models[kind]
    y = -8388608.0 + 4194304.0 * np.arange(5)
    b = np.array([1.5 * R_E, 4.5 * R_E, y[0], y[4], 0.7 * R_E, 0.7 * R_E])
    whole = m.dump(26, 5, 1, b)
    parts = []
    for lo, hi in ((0, 1), (2, 3), (4, 4)):
        bp = b.copy()
        bp[2], bp[3] = y[lo], y[hi]
        parts.append(m.dump(26, hi - lo + 1, 1, bp))
    assert np.array_equal(bits(whole), bits(np.concatenate(parts, axis=1)))
