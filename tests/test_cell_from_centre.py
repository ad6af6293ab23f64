"""CPU: the interp lookup's shortcut for the points around a searched centre (csrc/srt_models.hpp, Axis::in_cell) against the
full cell search (Axis::locate), both emulated in numpy exactly as they are written.

A lookup searches the cell of its centre on each axis and then asks of the six offset points and of the free point only
whether they lie in that cell and, if so, where.  Axis::in_cell answers with two comparisons against the cell's own nodes and
one division by a reciprocal the whole axis shares.  For no output bit to move,

  * its decision has to equal `locate(xi) == ci` for EVERY input: coordinates anywhere, NaN and +-inf included, centres in the
    clamped cells 0 and n, on nodes and one ulp either side, offsets far larger than a cell;
  * where the decision is true, its local coordinate has to carry locate's bits.  Here that is an identity of operands, not an
    independent check: both sides are the same expression, and the test shows that the shortcut feeds it what the full search
    would (the same cell, the same node(cell - 1), a reciprocal refined from the same seed).  That the device code computes those
    bits is checked on the GPU against the parent library's outputs (test_gpu_cell_from_centre.py);
  * the select-only form of locate has to return what the if / else form it replaced returned.

The decision and the select form have an independent reference: the count of nodes <= xi (searchsorted).  fdiv is emulated
with exact fp64 operations (a correctly rounded fma from libm).  Its hardware reciprocal seed is an input of the emulation: the
coordinate check runs for several seeds within v_rcp_f64's error; what the seeds add is that each refines to a proper reciprocal.
"""
import ctypes
import ctypes.util
import math

import numpy as np
import pytest

R_E = 6371200.0
GRIDS = ((256, -10 * R_E, 10 * R_E), (40, -5 * R_E, 5 * R_E), (24, -10 * R_E, 10 * R_E), (7, 0.0, 1.0))
# relative errors of the reciprocal seed: v_rcp_f64 is good to about 2^-26 at worst; 0 = the correctly rounded reciprocal
SEED_ERRORS = (0.0, 2.0 ** -26, -(2.0 ** -26), 2.0 ** -31, -(2.0 ** -40), 3 * 2.0 ** -52)


def _scalar_fma():
    if hasattr(math, "fma"):
        return math.fma
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fma.restype = ctypes.c_double
    libm.fma.argtypes = [ctypes.c_double] * 3
    return libm.fma


_fma1 = _scalar_fma()
_fma = np.frompyfunc(lambda a, b, c: _fma1(float(a), float(b), float(c)), 3, 1)


def fma(a, b, c):
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    return _fma(a, b, c).astype(np.float64)


def axis(n, lo, hi):
    d = (hi - lo) / (n - 1)
    return dict(min=lo, del_=d, rdel=1.0 / d, n=n)


def node(A, i):
    # real(i) * del + min, the product rounded on its own
    return (np.asarray(i).astype(np.float64) * A["del_"]) + A["min"]


def fdiv_recip(b, seed_err):
    """fdiv's first three operations: the seed (an input: the exact reciprocal off by seed_err) and two Newton steps."""
    r = (1.0 / b) * (1.0 + seed_err)
    for _ in range(2):
        r = _fma1(_fma1(-b, r, 1.0), r, r)
    return r


def fdiv_r(a, b, r):
    q = a * r
    return fma(fma(-b, q, a), r, q)


def locate_if_else(A, xi):
    """The cell search as it stood: if / else guess, two guarded corrections -> g."""
    n = A["n"]
    with np.errstate(all="ignore"):
        f = (xi - A["min"]) * A["rdel"]
        inside = (f >= 0.0) & ~(f >= float(n))
        g = np.where(inside, np.where(inside, f, 0.0).astype(np.int64) + 1, np.where(~(f >= 0.0), 0, n))
        g = g + ((g < n) & (node(A, g) <= xi))
        g = g - ((g > 0) & (node(A, g - 1) > xi))
    return g


def locate_selects(A, xi):
    """The cell search as it is written now: the guess converted from the clamped quotient, selects only -> g, node(g - 1)."""
    n = A["n"]
    with np.errstate(all="ignore"):
        f = (xi - A["min"]) * A["rdel"]
        fc = np.fmin(np.fmax(f, 0.0), float(n))  # fmax / fmin drop a NaN, like the device's
        g = fc.astype(np.int64) + 1
        g = np.where(f >= float(n), n, g)
        g = np.where(~(f >= 0.0), 0, g)
        g = g + ((g < n) & (node(A, g) <= xi)).astype(np.int64)
        g = g - ((g > 0) & (node(A, g - 1) > xi)).astype(np.int64)
    return g, node(A, g - 1)


def local_coordinate(A, xi, g, lo, r):
    """xl of locate and of in_cell: the same expression."""
    with np.errstate(all="ignore"):
        return np.where((g >= 1) & (g < A["n"]), fdiv_r(xi - lo, A["del_"], r), 0.0)


def in_cell(A, xi, g, lo, hi):
    n = A["n"]
    with np.errstate(all="ignore"):
        below_hi = np.where(g < n, ~(hi <= xi), True)
        above_lo = np.where(g > 0, xi >= lo, True)
    return below_hi & above_lo


def centres(A, rng, nrandom):
    """Random centres inside and up to two cells outside the range, every node and one ulp either side, NaN and +-inf."""
    n, d = A["n"], A["del_"]
    lo, hi = A["min"], A["min"] + (n - 1) * d
    nodes = node(A, np.arange(n))
    on = np.concatenate([nodes, np.nextafter(nodes, np.inf), np.nextafter(nodes, -np.inf)])
    return np.concatenate([rng.uniform(lo - 2 * d, hi + 2 * d, nrandom), np.repeat(on, 8), [np.nan, np.inf, -np.inf] * 4])


def neighbours(A, c, rng):
    """For each centre, the coordinates a lookup may ask about: offsets of 1e-9 .. 1e-3 |c| both ways, of up to five cells,
    exactly the centre, and NaN / +-inf sprinkled in."""
    d = A["del_"]
    with np.errstate(all="ignore"):
        for rel in (1e-9, 1e-6, 1e-3):
            off = np.maximum(np.abs(c) * rel, rel) * rng.uniform(0.5, 2.0, len(c))
            yield c + off
            yield c - off
        yield c + rng.normal(0.0, d, len(c))
        yield c + rng.uniform(-5 * d, 5 * d, len(c))
        yield c
        u = rng.random(len(c))
        yield np.where(u < 0.05, np.nan, np.where(u < 0.10, np.inf, np.where(u < 0.15, -np.inf, c + 1e-6 * np.abs(c))))


@pytest.mark.parametrize("n,lo,hi", GRIDS)
def test_select_form_of_locate_equals_the_if_else_form(n, lo, hi):
    A = axis(n, lo, hi)
    rng = np.random.default_rng(n)
    c = centres(A, rng, 400000)
    nodes = node(A, np.arange(n))
    for x in [c] + list(neighbours(A, c, rng)):
        g_old = locate_if_else(A, x)
        g_new, _ = locate_selects(A, x)
        assert np.array_equal(g_old, g_new)
        # and both are the true count of nodes <= x (what makes in_cell exact for offsets of any size); a NaN counts none
        true = np.where(np.isnan(x), 0, np.searchsorted(nodes, x, side="right"))
        assert np.array_equal(g_new, true)


@pytest.mark.parametrize("n,lo,hi", GRIDS)
def test_in_cell_decision_equals_full_search_everywhere(n, lo, hi):
    A = axis(n, lo, hi)
    rng = np.random.default_rng(100 + n)
    c = centres(A, rng, 400000)
    ci, clo = locate_selects(A, c)
    chi = node(A, ci)
    assert ci.min() == 0 and ci.max() == n  # the clamped cells are among the centres
    npairs = ntrue = 0
    for x in neighbours(A, c, rng):
        full = locate_if_else(A, x) == ci
        fast = in_cell(A, x, ci, clo, chi)
        assert np.array_equal(full, fast), "in_cell differs from locate(xi) == ci at %s" % x[full != fast][:5]
        npairs += len(c)
        ntrue += int(fast.sum())
    assert 0.2 < ntrue / npairs < 0.95  # both answers are well represented


def test_obvious_upper_comparison_would_not_do():
    """xi < node(ci) instead of !(node(ci) <= xi) differs for a NaN coordinate and a centre in cell 0, where locate(NaN) = 0:
    the reason for the form in_cell uses."""
    A = axis(40, -5 * R_E, 5 * R_E)
    c = np.array([A["min"] - 1.0])
    ci, clo = locate_selects(A, c)
    x = np.array([np.nan])
    assert ci[0] == 0 and locate_if_else(A, x)[0] == 0
    assert in_cell(A, x, ci, clo, node(A, ci))[0]
    with np.errstate(all="ignore"):
        assert not (x < node(A, ci))[0]


@pytest.mark.parametrize("seed_err", SEED_ERRORS)
@pytest.mark.parametrize("n,lo,hi", GRIDS)
def test_local_coordinate_bit_equal_where_in_cell(n, lo, hi, seed_err):
    A = axis(n, lo, hi)
    rng = np.random.default_rng(200 + n)
    c = centres(A, rng, 6000)
    r = fdiv_recip(A["del_"], seed_err)
    assert abs(r * A["del_"] - 1.0) < 2.0 ** -50  # the seeds all refine to a proper reciprocal
    ci, clo = locate_selects(A, c)
    chi = node(A, ci)
    nchecked = 0
    for x in neighbours(A, c, rng):
        # the full search of the point, with its own node(g - 1) and its own reciprocal from the same seed ...
        g, glo = locate_selects(A, x)
        xl_full = local_coordinate(A, x, g, glo, fdiv_recip(A["del_"], seed_err))
        # ... against the shortcut on the centre's values and the shared reciprocal
        inside = in_cell(A, x, ci, clo, chi)
        xl_fast = local_coordinate(A, x, ci, clo, r)
        assert np.array_equal(inside, g == ci)
        assert np.array_equal(xl_full[inside].view(np.uint64), xl_fast[inside].view(np.uint64))
        # clamped cells: the coordinate is the zero locate gives there
        clamped = inside & ((ci == 0) | (ci == n))
        assert not np.any(xl_fast[clamped])
        nchecked += int(inside.sum())
    assert nchecked > 10000
