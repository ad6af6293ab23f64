"""Point families for the IGRF edge tests (tests/test_igrf_edges.py) and their golden generator
(tests/golden/make_igrf_edges_golden.py): the head of igrf_core (stanford_raytracer_amd/csrc/srt_device.hpp) -- GEOGSW_08,
colatitude, truncation degree, pole predicate -- restated in numpy fp32 with the kernel's own operations in the kernel's
order, so that a family can be checked to sit on the branch it was built for, with a margin in ulp32."""
import numpy as np

R_E = 6371.2e3
F = np.float32
POLE_S = F(1.e-5)

FAM_AXIS, FAM_BIN, FAM_PAIR, FAM_DATE = 0, 1, 2, 3
FAMILY_NAMES = {FAM_AXIS: "axis", FAM_BIN: "degree bins", FAM_PAIR: "boundary pairs", FAM_DATE: "dates"}
AXIS_RADII = (1.5, 3.3, 7.0)
AXIS_OFFSETS = (0.0, 3e-6, 2e-5, 1e-4)          # sine of the GEO colatitude the point is built for
BOUNDARY_DATES = [(1960001, 0), (1965001, 0), (1969365, 0), (1970001, 0), (2019365, 0), (2020001, 0), (2024366, 0),
                  (2025001, 0), (2031001, 0), (2010001, 86399999)]
BASE_DATE = (2010001, 0)


def head(A, xyz):
    """fp32 head of igrf_core for GSW positions xyz[n, 3] (Earth radii): dict of r, rp2 = r + 2, c, s, rho, k, pole."""
    A = np.asarray(A, dtype=F)
    x, y, z = (np.ascontiguousarray(np.asarray(xyz, dtype=F)[..., i]) for i in range(3))
    xgeo = A[0] * x + A[3] * y + A[6] * z
    ygeo = A[1] * x + A[4] * y + A[7] * z
    zgeo = A[2] * x + A[5] * y + A[8] * z
    rho2 = xgeo * xgeo + ygeo * ygeo
    r = np.sqrt(rho2 + zgeo * zgeo)
    rho = np.sqrt(rho2)
    with np.errstate(invalid="ignore", divide="ignore"):
        c, s = zgeo / r, rho / r
    rp2 = r + F(2.0)
    irp3 = np.maximum(rp2.astype(np.int32), 1)
    k = np.minimum(3 + 30 // irp3, 13) + 1
    assert all(v.dtype == F for v in (xgeo, r, rho, c, s, rp2))
    return {"r": r, "rp2": rp2, "c": c, "s": s, "rho": rho, "k": k, "pole": s < POLE_S}


def ulps_from(v, target):
    """|v - target| in units of the fp32 spacing at target."""
    t = F(target)
    return np.abs(np.asarray(v, dtype=np.float64) - np.float64(t)) / np.float64(np.spacing(t))


def ulps_from_integer(rp2):
    """Distance of fp32 r + 2 from the nearest integer, in units of the fp32 spacing at that integer."""
    n = np.rint(np.asarray(rp2, dtype=np.float64))
    return np.abs(np.asarray(rp2, dtype=np.float64) - n) / np.spacing(n.astype(F)).astype(np.float64)


def sm_to_gsw32(x_sm, cs):
    """The adapters' SM -> GSM rotation in fp64 and the cast to REAL Earth radii (bfield_igrf): x_sm[n, 3] in metres."""
    x_sm = np.asarray(x_sm, dtype=np.float64)
    cm, sm = cs
    return np.stack([(x_sm[..., 0] * cm - x_sm[..., 2] * sm) / R_E, x_sm[..., 1] / R_E,
                     (x_sm[..., 2] * cm + x_sm[..., 0] * sm) / R_E], axis=-1).astype(F)


def gsw_to_sm(x_gsw, cs):
    """Inverse rotation, fp64: GSW Earth radii -> SM metres."""
    x_gsw = np.asarray(x_gsw, dtype=np.float64)
    cm, sm = cs
    return R_E * np.stack([x_gsw[..., 0] * cm + x_gsw[..., 2] * sm, x_gsw[..., 1], x_gsw[..., 2] * cm - x_gsw[..., 0] * sm], axis=-1)


def geo_axis_frame(A):
    """The GEO z axis in GSW (column A13, A23, A33 of the GEO -> GSW matrix) and two unit vectors across it, fp64."""
    A = np.asarray(A, dtype=np.float64)
    ax = np.array([A[2], A[5], A[8]])
    ax /= np.linalg.norm(ax)
    e1 = np.cross(ax, [0.0, 1.0, 0.0])
    e1 /= np.linalg.norm(e1)
    return ax, e1, np.cross(ax, e1)


def axis_points_gsw(A, radii=AXIS_RADII, offsets=AXIS_OFFSETS):
    """Family (a) in GSW Earth radii (fp64): both hemispheres, each radius, each sine of colatitude along e1 and (from 2e-5
    on) along e2 too.  Returns (points[n, 3], built_s[n])."""
    ax, e1, e2 = geo_axis_frame(A)
    pts, built = [], []
    for sign in (1.0, -1.0):
        for r in radii:
            for t in offsets:
                for e in ((e1,) if t < 1e-5 else (e1, e2)):
                    pts.append(r * (sign * np.sqrt(1.0 - t * t) * ax + t * e))
                    built.append(t)
    return np.array(pts), np.array(built)


def check_axis(h, built):
    """Family (a) sits where it was built: s < 5e-6 for the polar points, within 10 % of the built sine for the others, and
    never within 8 ulp32 of the kernel's threshold 1e-5f."""
    polar = built < 1e-5
    assert np.all(h["s"][polar] < 5e-6) and np.all(h["pole"][polar])
    assert np.all(np.abs(h["s"][~polar] / built[~polar] - 1.0) < 0.1) and not np.any(h["pole"][~polar])
    assert np.all(ulps_from(h["s"], POLE_S) >= 8)
    assert np.any(h["c"][polar] > 0) and np.any(h["c"][polar] < 0)


def unit_vectors(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def bin_radii():
    """Family (b): one radius in every bin of int(r + 2) from 2 to 31."""
    return np.array([0.9] + [b - 2 + 0.5 for b in range(3, 32)])


def pair_radii(rel=1e-5):
    """Family (b): a pair a relative `rel` either side of every integer r + 2 = 3 .. 31, [inside, outside] interleaved."""
    return np.array([r * (1.0 + sg * rel) for r in range(1, 30) for sg in (-1.0, 1.0)])


def check_bins(h):
    assert np.array_equal(h["rp2"].astype(np.int32), np.arange(2, 32))
    assert h["k"][0] == 14 and h["k"].min() == 4 and np.all(np.diff(h["k"]) <= 0)


def check_pairs(h):
    irp3 = h["rp2"].astype(np.int32)
    assert np.array_equal(irp3[0::2], np.arange(2, 31)) and np.array_equal(irp3[1::2], np.arange(3, 32))
    assert np.all(ulps_from_integer(h["rp2"]) >= 8)
