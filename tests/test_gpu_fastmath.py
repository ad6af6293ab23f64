"""GPU: the device-only elementary functions of stanford_raytracer_amd/csrc/srt_fastmath.hpp, called directly through the
probe library (tests/native/fastmath_probe.hip -> lib/libsrt_fastmath_probe.so), against long-double references, and the
device's fp64 EXTERN modules of srt_t04.hpp against the reference's ext_out.  Point sets, references and bars are those of
the host emulation's test (fastmath_cases.py, test_fastmath_host.py); here the hardware's v_rcp_f64 / v_rsq_f64 and the
device compiler's contraction are inside what is held."""
import ctypes as C
import os

import numpy as np
import pytest

import fastmath_cases as fc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe():
    from stanford_raytracer_amd import build as pkg_build

    return C.CDLL(pkg_build.build_probe())                                         # rebuilt when a header is newer


@pytest.fixture(scope="module")
def ev(probe):
    return fc.mixed_sizes(fc.ctypes_ev(probe.fmp_eval))


@pytest.fixture(scope="module")
def t04pow(tmp_path_factory):
    return fc.t04_pow_pairs(tmp_path_factory.mktemp("t04p"))


def rng(seed):
    return np.random.default_rng(seed)


# a. bit-exact
def test_gpu_fdiv_is_ieee_division(ev):
    fc.check_fdiv(ev, rng(1))


def test_gpu_sqrt_pos_is_correctly_rounded(ev):
    fc.check_sqrt_pos(ev, rng(2))


def test_gpu_report_outside_the_exponent_box(ev):
    """Printed only: where fdiv and sqrt_pos leave IEEE outside their exponent boxes."""
    assert len(fc.report_outside(ev, rng(9))) > 10


# b. <= 2 ulp
def test_gpu_sqrt_and_inv_pos(ev):
    fc.check_sqrt_and_inv_pos(ev, rng(3))


def test_gpu_log_pos(ev):
    fc.check_log_pos(ev, rng(4))


def test_gpu_exp_any(ev):
    fc.check_exp_any(ev, rng(5))


def test_gpu_sincos_0pi(ev):
    fc.check_sincos_0pi(ev, rng(6))


def test_gpu_sincos_mod(ev):
    fc.check_sincos_mod(ev, rng(7))


def test_gpu_pow_pos(ev, t04pow):
    fc.check_pow_pos(ev, rng(8), t04pow)


# c. the device's fp64 EXTERN modules
def test_gpu_extern_modules_match_the_reference(probe):
    """Each of the 11 modules of EXTERN as the DEVICE computes it in fp64 (srt_fastmath.hpp's functions, the device compiler's
    contraction) against the reference's ext_out: within 10 x the distance FMA contraction alone puts between the host build
    and ext_out (fastmath_cases.T04_FMA_YARDSTICK, floor 1e-15); the IMF term bit for bit."""
    gold = np.load(os.path.join(fc.GOLDEN_DIR, "t04_golden.npz"))
    rows, want = np.ascontiguousarray(gold["ext_in"], dtype=np.float64), gold["ext_out"]
    got = np.zeros((len(rows), 33))
    P = C.POINTER(C.c_double)
    probe.fmp_t04_components.argtypes = [C.c_long, P, P]
    probe.fmp_t04_components.restype = C.c_int
    rc = probe.fmp_t04_components(len(rows), rows.ctypes.data_as(P), got.ctypes.data_as(P))
    assert rc == 0, rc
    err = fc.t04_module_errors(got, want)
    for nm in fc.T04_MODULES:
        print("%-6s device %.3g  bar %.3g" % (nm, err[nm], 10.0 * max(fc.T04_FMA_YARDSTICK[nm], fc.T04_FLOOR)))
    k = fc.T04_MODULES.index("himf")
    assert np.array_equal(got[:, 3 * k:3 * k + 3], want[:, 3 * k:3 * k + 3])
    for nm in fc.T04_MODULES:
        assert err[nm] <= 10.0 * max(fc.T04_FMA_YARDSTICK[nm], fc.T04_FLOOR), (nm, err[nm])


# d. outside the domains
def test_gpu_outside_the_domains(ev):
    fc.check_outside(ev)
