"""What modelnum 7's host test (tests/test_at64thch_host.py) and device test (tests/test_gpu_at64thch.py) share besides the ladder
(tests/model_ladder.py): the host build of the device's source and the foot check.  Not a test module."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

from conftest import ROOT
from stanford_raytracer_amd import workloads as wl

COEFFS = os.path.join(ROOT, "stanford_raytracer_amd", "data", "igrf_coeffs.txt")


def build_host_library(d):
    """tests/native/at64thch_host.cpp compiled into directory d and loaded"""
    so = str(d / "libat64h.so")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    from stanford_raytracer_amd import build
    assert os.path.exists(build.LIB), "build() first: the host build takes the date's constants from the library"
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC",
                           "-o", so, os.path.join(ROOT, "tests", "native", "at64thch_host.cpp"),
                           "-L" + build.LIBDIR, "-lsrt_hip", "-Wl,-rpath," + build.LIBDIR])
    L = C.CDLL(so)
    L.at64h_create.restype = C.c_void_p
    L.at64h_create.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    L.at64h_destroy.argtypes = [C.c_void_p]
    L.at64h_psi.argtypes = [C.c_void_p]
    L.at64h_psi.restype = C.c_float
    L.at64h_density.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_void_p]
    L.at64h_closed_form.argtypes = [C.c_int, C.c_long, C.c_void_p, C.c_double, C.c_void_p]
    L.at64h_foot.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_float, C.c_int, C.c_void_p]
    return L


class Host:
    """the host build's handle of one golden setting (gcpm_kp, yearday, msec, use_igrf, use_tsyganenko) and its parmod"""

    def __init__(self, L, setting, parmod):
        self.L, self.kp = L, int(setting[0])
        pm = np.ascontiguousarray(parmod, dtype=np.float64)
        self.h = L.at64h_create(os.fsencode(COEFFS), int(setting[1]), int(setting[2]), self.kp, pm.ctypes.data, int(setting[3]))
        assert self.h

    def density(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        Ns = np.zeros((len(x), 3))
        self.L.at64h_density(self.h, len(x), x.ctypes.data, Ns.ctypes.data)
        return Ns

    def closed_form(self, x, zbrat):
        x = np.ascontiguousarray(x, dtype=np.float64)
        Ns = np.zeros((len(x), 3))
        self.L.at64h_closed_form(self.kp, len(x), x.ctypes.data, zbrat, Ns.ctypes.data)
        return Ns

    def foot(self, x, dsmax=1.0, lmax=500):
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = np.zeros((len(x), 6))
        self.L.at64h_foot(self.h, len(x), x.ctypes.data, dsmax, lmax, out.ctypes.data)
        return out

    def __del__(self):
        self.L.at64h_destroy(self.h)


def foot_bar(gold, tag):
    return np.maximum(2e-6, 10.0 * gold["g0_foot_sens_" + tag])


def check_foot(got, gold, tag):
    """the foot test's assertions, for the host's feet and the device's"""
    traced = np.linalg.norm(gold["g0_x_" + tag], axis=1) - wl.R_E > 400e3
    assert np.array_equal(traced, np.isfinite(gold["g0_foot_" + tag][:, 0])), "the golden's feet are not those of the points above 400 km"
    got, want, sens, bar = got[traced], gold["g0_foot_" + tag][traced], gold["g0_sens_" + tag][traced, 0], foot_bar(gold, tag)[traced]
    move = np.linalg.norm(got[:, 0:3] - want[:, 0:3], axis=1)
    quiet = sens < 1e-5
    print("foot %s: %d points, distance from the reference's max %.3g (bit-equal %.1f %%), endings equal %d / %d, L equal %.1f %%"
          % (tag, len(want), move.max(), 100 * np.mean(move == 0), (got[:, 4] == want[:, 4]).sum(), len(want), 100 * np.mean(got[:, 5] == want[:, 5])))
    assert np.all(np.isfinite(got)), "%d feet have a component that is not finite" % (~np.isfinite(got)).any(axis=1).sum()
    assert np.all(move <= bar), "%d feet over their bar, worst ratio %.3g" % ((move > bar).sum(), np.max(move / bar))
    assert np.array_equal(got[quiet, 4], want[quiet, 4]), "%d quiet points end otherwise than the reference's" % (got[quiet, 4] != want[quiet, 4]).sum()
    assert np.all(got[:, 5] <= 500), "a line of %d points" % got[:, 5].max()
    # |IGRF| at the foot: a smooth function of the foot (r^-3: three times the foot's relative bar, and a rounding)
    eb = np.abs(got[:, 3] - want[:, 3]) / want[:, 3]
    bb = 3.0 * bar / np.linalg.norm(want[:, 0:3], axis=1) + 2e-7
    assert np.all(eb <= bb), "|IGRF| at %d feet over its bar, worst ratio %.3g" % ((eb > bb).sum(), np.max(eb / bb))
