"""modelnum 5 on the CPU: the Ngo density path of stanford_raytracer_amd/csrc (srt_ngo3d.hpp's per-point head, srt_models.hpp's
dens_core / ducts / taper -- the very source the device compiles) built for the host (tests/native/ngo3d_host.cpp) and held
against goldens captured from the reference's own ngo_3d_dens_model_adapter (tests/golden/ngo3d_golden.npz,
make_ngo3d_golden.py).

Bars, per point and with no point skipped: densities max(1e-11, 10 x the reference's recorded sensitivity) relative -- 1e-11 is
the project's G0 bar, the second term DESIGN section 4's sensitivity rule; lk within 4 ulp of the reference's (a8 is a sum and
product of a dozen terms after one sin and one exp, each of which the two maths libraries may round differently by an ulp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN_DIR, ROOT
from model_ladder import check_g0_density
from stanford_raytracer_amd import workloads as wl

SETTINGS = "abcd"
NEWRAY = (wl.NEWRAY_PLASMAPAUSE, wl.NEWRAY_DUCTS)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN_DIR, "ngo3d_golden.npz"))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """(library, [card file of the plasmapause workload, of the ducts workload])"""
    d = tmp_path_factory.mktemp("ngo3d")
    so = str(d / "libngo3dh.so")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    from stanford_raytracer_amd import build
    assert os.path.exists(build.LIB), "build() first: the host build takes the card-file reader from the library"
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC",
                           "-o", so, os.path.join(ROOT, "tests", "native", "ngo3d_host.cpp"),
                           "-L" + build.LIBDIR, "-lsrt_hip", "-Wl,-rpath," + build.LIBDIR])
    L = C.CDLL(so)
    L.ngo3dh_density.argtypes = [C.c_char_p, C.c_double, C.c_int, C.c_double, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p]
    cards = []
    for k, text in enumerate(NEWRAY):
        cards.append(str(d / ("newray%d.in" % k)))
        with open(cards[-1], "w") as f:
            f.write(text)
    return L, cards


def host_density(host, setting, x):
    """-> Ns[n, 4], lk[n] of a golden setting (kp, yearday, msec, fixed_MLT, MLT, igrf, tsy, card file)"""
    L, cards = host
    kp, fixed, mlt, card = setting[0], setting[3], setting[4], setting[7]
    x = np.ascontiguousarray(x, dtype=np.float64)
    Ns, lk = np.zeros((len(x), 4)), np.zeros(len(x))
    assert L.ngo3dh_density(os.fsencode(cards[int(card)]), kp, int(fixed), mlt, len(x), x.ctypes.data, Ns.ctypes.data, lk.ctypes.data) == 0
    return Ns, lk


def test_the_committed_golden_meets_the_generators_input_conditions(gold):
    sens = np.concatenate([gold["g0_sens_" + t] for t in SETTINGS])
    Ns = np.concatenate([gold["g0_Ns_" + t] for t in SETTINGS])
    lk = np.concatenate([gold["g0_lk_" + t] for t in SETTINGS])
    assert len(sens) >= 2000
    assert np.all(np.isfinite(Ns)) and np.all(Ns > 0) and np.all(np.isfinite(lk))
    assert np.mean(sens > 1e-11) <= 1e-3
    assert sens.max() <= 1e-9
    # at least four settings: two (Kp, date) pairs, fixed_MLT both ways, IGRF and T04_s for one setting each, both card files
    st = np.array([gold["g0_setting_" + t] for t in SETTINGS])
    assert len(st) >= 4 and len({(a, b) for a, b in st[:, 0:2]}) >= 2 and set(st[:, 3]) == {0.0, 1.0}
    assert st[:, 5].sum() >= 1 and st[:, 6].sum() >= 1 and set(st[:, 7]) == {0.0, 1.0}
    for t in SETTINGS:
        x, lk, card = gold["g0_x_" + t], gold["g0_lk_" + t], int(gold["g0_setting_" + t][7])
        ddk = gold["ddk"][card]
        L = np.linalg.norm(x, axis=1) ** 3 / (wl.R_E * (x[:, 0] ** 2 + x[:, 1] ** 2))
        # both sides of the local plasmapause, and points within +-3 ddk of it on either side
        assert (L > lk).sum() >= 100 and (L < lk).sum() >= 100
        near = np.abs(L - lk) <= 3.001 * ddk
        assert (near & (L > lk)).sum() >= 20 and (near & (L < lk)).sum() >= 20, t
        if card == 1:  # the ducts file: either side of the sinusoidal perturbation's critl (l0(2) = -0.5, dd(2) = 0.4)
            critl = (lk + ddk) + np.fmod(0.5 - (lk + ddk) + 0.2, 0.4)
            close = np.abs(L - critl) <= 0.011
            assert (close & (L > critl)).sum() >= 5 and (close & (L < critl)).sum() >= 5, t
    mlt = np.mod(24.0 * np.arctan2(gold["g0_x_a"][:, 1], gold["g0_x_a"][:, 0]) / (2 * np.pi) + 12.0, 24.0)
    assert (mlt < 1e-6).any() and (mlt > 24 - 1e-6).any()


@pytest.mark.parametrize("tag", list(SETTINGS))
def test_host_build_of_the_device_source_against_the_reference(gold, host, tag):
    x, wlk = gold["g0_x_" + tag], gold["g0_lk_" + tag]
    got, lk = host_density(host, gold["g0_setting_" + tag], x)
    ulps = np.abs(lk - wlk) / np.spacing(np.abs(wlk))
    check_g0_density(got, gold, tag, floor=1e-11, per_species=False, report=lambda err: print(
        "setting %s: %d points, max density error %.3g, bit-equal %.1f %%; lk: max %.1f ulp, bit-equal %.1f %%"
        % (tag, len(x), err.max(), 100 * np.mean(err == 0), ulps.max(), 100 * np.mean(ulps == 0))))
    assert ulps.max() <= 4


def test_the_plasmapause_lies_within_bulges_bounds(host):
    """lk = a8 - ddk, and a8 = (b1 Kp + b2) (1 + exp(..)): (b1 Kp + b2) lies between 5.3854 - 8 x 0.5019 = 1.37 and 6.1074 for
    Kp 0 .. 8, the second factor between 1 and 1 + exp(-0.7 + 0.08^2 / 6) = 1.497 -- at every MLT."""
    ddk = 0.07  # of the plasmapause card file
    r = 3.0 * wl.R_E
    for kp in (0.0, 1.0, 2.5, 4.0, 6.0, 8.0):
        mlt = np.linspace(0.0, 24.0, 49)
        phi = (mlt - 12.0) * 2.0 * np.pi / 24.0
        x = np.stack([r * np.cos(phi), r * np.sin(phi), np.full(49, 0.3 * r)], axis=1)
        Ns, lk = host_density(host, (kp, 2010001, 0, 0, 0.0, 0, 0, 0), x)
        assert np.all(np.isfinite(Ns)) and np.all(Ns > 0)
        assert np.all(lk > 1.37 - ddk) and np.all(lk < 9.15), (kp, lk.min(), lk.max())
        # and the same value when that MLT is given as the fixed one
        for j in (0, 7, 30):
            _, lkf = host_density(host, (kp, 2010001, 0, 1, mlt[j], 0, 0, 0), x[:3])
            assert abs(lkf[0] - lk[j]) <= 1e-9, (kp, j)  # (the longitude -> MLT round trip costs a few ulp of 24)


def test_with_a_fixed_mlt_the_plasmapause_does_not_depend_on_the_point(host, gold):
    x = gold["g0_x_a"]
    for card in (0, 1):
        _, lk = host_density(host, (4.0, 2010001, 0, 1, 21.25, 0, 0, card), x)
        assert np.all(lk == lk[0])
        _, free = host_density(host, (4.0, 2010001, 0, 0, 21.25, 0, 0, card), x)
        assert len(np.unique(free)) > 100  # the same points with MLT from the longitude: one plasmapause each
