"""CPU: the elementary functions of stanford_raytracer_amd/csrc/srt_fastmath.hpp, the unmodified header compiled for the
host (tests/native/fastmath_host.cpp, exact 1/b and 1/sqrt(x) for the hardware's seeds), on the point sets and under the
bars of the device test (test_gpu_fastmath.py; both live in fastmath_cases.py): the polynomials, the reductions and the
selects, everything but v_rcp_f64 / v_rsq_f64.  Also: the long-double reference against mpmath, the pow arguments of T04,
the FMA-contraction yardstick of the EXTERN modules, and the probe library's build."""
import ctypes as C
import os

import mpmath
import numpy as np
import pytest

import fastmath_cases as fc
from fastmath_cases import LD


@pytest.fixture(scope="module")
def ev(tmp_path_factory):
    return fc.mixed_sizes(fc.host_emulation(tmp_path_factory.mktemp("fmh")))


@pytest.fixture(scope="module")
def t04pow(tmp_path_factory):
    return fc.t04_pow_pairs(tmp_path_factory.mktemp("t04p"))


def rng(seed):
    return np.random.default_rng(seed)


# ------------------------------------------------------------------------------------------------- reference machinery
def to_mpf(v):
    m, e = np.frexp(v)                                                             # (the low half of a tiny v would be a denormal double)
    hi = float(m)
    return mpmath.ldexp(mpmath.mpf(hi) + mpmath.mpf(float(m - LD(hi))), int(e))


def test_long_double_reference_agrees_with_mpmath(t04pow):
    """The yardstick of every ulp figure here: numpy's long double has a 64-bit significand and its sqrt / log / exp / sin / cos
    / pow agree with mpmath (50 digits) to < 2^-60 relative on 2 000 points per function, edge points included.  Where long double
    is the 53-bit double (no such platform builds this project today) this fails rather than falling back to mpmath references."""
    assert np.finfo(LD).nmant >= 63
    r = rng(11)

    def sub(x, n=2000):
        return np.concatenate([x[:n - 200], x[-200:]])

    s0, _ = fc.sincos_0pi_points(r)
    sm, n_uni = fc.sincos_mod_points(r)
    px, py = fc.pow_points(r, t04pow[0], t04pow[1])
    pick = np.concatenate([np.arange(1000), r.integers(0, px.size, 1000)])
    sets = [("sqrt", sub(fc.sqrt_and_inv_points(r)), lambda x: fc.sqrt_and_inv_ref(x)[0], mpmath.sqrt),
            ("rsqrt", sub(fc.sqrt_and_inv_points(r)), lambda x: fc.sqrt_and_inv_ref(x)[1], lambda v: 1 / mpmath.sqrt(v)),
            ("log", sub(fc.log_points(r)), fc.log_ref, mpmath.log),
            ("exp", sub(fc.exp_points(r)), fc.exp_ref, mpmath.exp),
            ("exp, denormal results", sub(fc.exp_denormal_points(r)), fc.exp_ref, mpmath.exp),
            ("sin on [0, pi]", sub(s0), lambda x: fc.sincos_ref(x)[0], mpmath.sin),
            ("cos on [0, pi]", sub(s0), lambda x: fc.sincos_ref(x)[1], mpmath.cos),
            ("sin to 1e5", np.concatenate([sm[:1000], r.choice(sm[n_uni:], 1000)]), lambda x: fc.sincos_ref(x)[0], mpmath.sin),
            ("cos to 1e5", np.concatenate([sm[:1000], r.choice(sm[n_uni:], 1000)]), lambda x: fc.sincos_ref(x)[1], mpmath.cos)]
    with mpmath.workdps(50):
        for name, x, ref, mpf in sets:
            got = ref(x)
            worst = 0.0
            for xi, gi in zip(x, got):
                want = mpf(mpmath.mpf(float(xi)))
                if want != 0:
                    worst = max(worst, float(abs((to_mpf(gi) - want) / want)))
                else:
                    assert gi == 0
            print("%s: long double against mpmath, max relative difference 2^%.1f over %d points" % (name, np.log2(max(worst, 1e-300)), x.size))
            assert worst < 2.0 ** -60, (name, worst)
        got = fc.pow_ref(px[pick], py[pick])
        worst = max(float(abs((to_mpf(g) - mpmath.power(mpmath.mpf(float(a)), mpmath.mpf(float(b)))) / mpmath.power(mpmath.mpf(float(a)), mpmath.mpf(float(b)))))
                    for a, b, g in zip(px[pick], py[pick], got))
        print("pow: long double against mpmath, max relative difference 2^%.1f over %d points" % (np.log2(worst), pick.size))
        assert worst < 2.0 ** -60
    # the floor of the two sincos checks: the header's two literals against pi/2
    unit = fc.pio2_floor_unit()
    assert 2.0 ** -90 < unit < 2.0 ** -85, unit


# ------------------------------------------------------------------------------------------------- a. bit-exact
def test_fdiv_is_ieee_division(ev):
    fc.check_fdiv(ev, rng(1))


def test_sqrt_pos_is_correctly_rounded(ev):
    fc.check_sqrt_pos(ev, rng(2))


# ------------------------------------------------------------------------------------------------- b. 2 ulp
def test_sqrt_and_inv_pos(ev):
    fc.check_sqrt_and_inv_pos(ev, rng(3))


def test_log_pos(ev):
    fc.check_log_pos(ev, rng(4))


def test_exp_any(ev):
    fc.check_exp_any(ev, rng(5))


def test_sincos_0pi(ev):
    fc.check_sincos_0pi(ev, rng(6))


def test_sincos_mod(ev):
    fc.check_sincos_mod(ev, rng(7))


def test_pow_pos(ev, t04pow):
    fc.check_pow_pos(ev, rng(8), t04pow)


# ------------------------------------------------------------------------------------------------- d. outside the domains
def test_outside_the_domains(ev):
    fc.check_outside(ev)


def test_report_outside_the_exponent_box(ev):
    """Printed only: where fdiv and sqrt_pos leave IEEE outside their exponent boxes."""
    assert len(fc.report_outside(ev, rng(9))) > 10


# ------------------------------------------------------------------------------------------------- T04 yardstick, build
def t04_components(lib, rows):
    got = np.zeros((len(rows), 33))
    for i, r in enumerate(rows):
        inp = (C.c_double * 14)(*r)
        out = (C.c_double * 33)()
        lib.t04h_components(inp, out)
        got[i] = list(out)
    return got


def test_t04_fma_yardstick(tmp_path):
    """srt_t04.hpp for the host with libm, without and with FMA contraction: the distance contraction alone puts between our
    source and the reference's ext_out, per module.  fastmath_cases.T04_FMA_YARDSTICK holds these values as constants for the
    device test; each must be at least the value recomputed here and at most twice it (neither stale nor loose)."""
    gold = np.load(os.path.join(fc.GOLDEN_DIR, "t04_golden.npz"))
    rows, want = gold["ext_in"], gold["ext_out"]
    off = fc.t04_module_errors(t04_components(fc.build_host(tmp_path, "off.so", "t04_host.cpp", ["-ffp-contract=off"]), rows), want)
    fast = fc.t04_module_errors(t04_components(fc.build_host(tmp_path, "fast.so", "t04_host.cpp", ["-mfma", "-ffp-contract=fast"]), rows), want)
    for nm in fc.T04_MODULES:
        print("%-6s contract off %.3g  contract fast %.3g  constant %.3g" % (nm, off[nm], fast[nm], fc.T04_FMA_YARDSTICK[nm]))
    for nm in fc.T04_MODULES:
        assert fast[nm] <= fc.T04_FMA_YARDSTICK[nm] <= 2.0 * fast[nm], (nm, fast[nm], fc.T04_FMA_YARDSTICK[nm])
    assert fc.T04_FMA_YARDSTICK["himf"] == 0.0


def test_build_produces_the_probe():
    from stanford_raytracer_amd import build as pkg_build

    assert pkg_build.build_probe() == pkg_build.PROBE and os.path.exists(pkg_build.PROBE)
    assert os.path.dirname(pkg_build.PROBE) == os.path.dirname(pkg_build.LIB) and pkg_build.PROBE != pkg_build.LIB
    lib = C.CDLL(pkg_build.PROBE)                                                  # loading makes no device call
    for s in ("fmp_eval", "fmp_t04_components", "fmp_op_count"):
        assert hasattr(lib, s), s
    lib.fmp_op_count.restype = C.c_int
    assert lib.fmp_op_count() == len(fc.OPS)
    # the product neither links nor names the probe
    import subprocess
    needed = subprocess.run(["readelf", "-d", pkg_build.LIB], capture_output=True, text=True, check=True).stdout
    assert "fastmath_probe" not in needed
