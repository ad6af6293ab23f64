"""GPU (-m gpu): solve_dispersion and is_right_handed of srt_device.hpp against the reference across plasma regimes: the rows of
tests/dispersion_regimes.py with the reference's outputs in tests/golden/dispersion_regimes_golden.npz (the CPU side, and what
the rows guarantee, is tests/test_dispersion_regimes.py).  Five 6^3 models, at most 650 states per call.

Bars, none of them taken from a device's output:
  handedness   equal to the reference wherever gap >= 1e-6 (below it the reference's SVD picks its vector arbitrarily)
  S D P R L    |delta| <= 1e-10 max(|ref|, 1): each is 1 minus a sum and passes through 0 at a cutoff
  F            1e-10 of the size of its cancelling terms (dispersion_checks.f_scale)
  roots        Re and |Im| within 1e-10 kappa of the root's magnitude, kappa = max(1, |B| / sqrt|B^2 - 4 A RLP|): one ulp in S, D, P
               moves n^2 by about kappa ulp through sqrt(disc), and 1e-10 is the G1 bar of test_gpu_parity.py.  k1 against k1 and
               k2 against k2 on the comparable set (gap >= 1e-6, roots more than 1e-6 apart, kappa <= 1e4: at least nine rows in
               ten of every family), as an unordered pair elsewhere.  The rows stand off the resonances, where one ulp in R, L, P
               moves a root by at most a tenth of this bar (dispersion_regimes.detuned).
  cos^2 > 1    k = s B0: finite roots in the order of the reference 1e-6 rad off that direction, to 1e-5 (same order or swapped)
  zero density Ns exactly 0, F = 1 - n^2 to 1e-13 max(1, n^2), roots w / c to 1e-14; a fixed-step trace has the reference's rows and
               stop codes and its positions lie within 2.1e-8 of |x| of the reference's: ten times 2.03e-9, the reference's own
               largest deviation from the straight line x0 + c t d on these 8 rays x 10 steps (its dF/dk differences with del = 1e-8
               around F = 1 - n^2; recorded by the maker as zero_run_line_dev)
  gradients    dF/dk, dF/dw, dx/dt at on-surface states, per density: the ladder's 1e-7, 1e-6, 1e-6 where the oracle itself
               holds them, else ten times the oracle's OWN largest change when k and w move by 1e-15 relative (CPU, seeds 1, 2, 3,
               all five families, del = 1e-6):   N_e     states   dF/dk     dF/dw     dx/dt
                                                 1e6     220      8.0e-10   1.02e-6   1.02e-6
                                                 1e8      87      7.2e-9    8.1e-7    8.1e-7
                                                 1e10     65      1.24e-6   1.22e-5   1.25e-5
                                                 1e12     41      3.53e-5   4.65e-5   3.51e-5
               (central differences with a 1e-8 relative step amplify one ulp of F's cancelling terms by 1e8.)
"""
import os

import numpy as np
import pytest

import dispersion_regimes as dr
from conftest import GOLDEN_DIR, vrel
from dispersion_checks import f_scale

pytestmark = pytest.mark.gpu
KEYS = list(dr.GRIDS)
LADDER = (1e-7, 1e-6, 1e-6)
OWN_CHANGE = {"ne6": (8.0e-10, 1.02e-6, 1.02e-6), "ne8": (7.2e-9, 8.1e-7, 8.1e-7), "ne10": (1.24e-6, 1.22e-5, 1.25e-5),
              "ne12": (3.53e-5, 4.65e-5, 3.51e-5)}
GRAD_BARS = {k: tuple(max(lad, 10.0 * own) for lad, own in zip(LADDER, v)) for k, v in OWN_CHANGE.items()}
ZERO_KW = dict(fixedstep=1, dt0=1e-3, dtmax=0.1, tmax=1.0, maxerr=5e-4, maxsteps=10, root=2, del_=1e-6)


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN_DIR, "dispersion_regimes_golden.npz"))


@pytest.fixture(scope="module")
def omodels():
    from oracle import oracle
    from stanford_raytracer_amd import workloads as wl

    return {key: oracle.Model.interp(*dr.grid(key), wl.QS, wl.MS) for key in KEYS + ["zero"]}


@pytest.fixture(scope="module")
def gmodels():
    from stanford_raytracer_amd import api, workloads as wl

    api.init(0)
    return {key: api.Model.interp(*dr.grid(key), wl.QS, wl.MS) for key in KEYS + ["zero"]}


@pytest.fixture(scope="module")
def cases(g, omodels, gmodels):
    """Per grid, all five families in one call of srt_dispersion (650 states): dict key -> dict of rows, ref (the reference's rows;
    where it stopped, the oracle's, which the CPU suite holds to it bit for bit elsewhere), stopped, judge, metrics, family slices,
    and the device's output."""
    out = {}
    for key in KEYS:
        parts = [dr.judged(g, key, fam) for fam in dr.FAMILIES]
        rows, ref, st, judge = (np.concatenate([p[i] for p in parts]) for i in range(4))
        om = omodels[key]
        with np.errstate(all="ignore"):
            for i in np.where(st)[0]:
                ref[i] = om.disp(rows[i, 0:3], rows[i, 3:6], rows[i, 6])
        m = dr.state_metrics(rows, judge, dr.field_at(om, rows[:, 0:3]))
        sl = {fam: slice(i * dr.N_STATES, (i + 1) * dr.N_STATES) for i, fam in enumerate(dr.FAMILIES)}
        out[key] = dict(rows=rows, ref=ref, stopped=st, judge=judge, m=m, sl=sl,
                        gpu=gmodels[key].dispersion(rows[:, 0:3], rows[:, 3:6], rows[:, 6]))
    return out


@pytest.mark.parametrize("fam", dr.RH_FAMILIES)
def test_handedness_matches_the_reference(g, fam):
    from stanford_raytracer_amd import api

    api.init(0)
    t, ref = g["rh_%s_in" % fam], g["rh_%s_out" % fam].astype(bool)
    got = api.is_right_handed(t)
    ok = dr.rh_gap(t) >= dr.GAP_MIN
    print("%s: %d of %d rows below the gap, %d of them differ; %d differ above it" % (
        fam, (~ok).sum(), len(t), (got != ref)[~ok].sum(), (got != ref)[ok].sum()))
    assert np.array_equal(got[ok], ref[ok]), "%d decisions differ" % (got != ref)[ok].sum()
    assert api.is_right_handed(t[:0]).shape == (0,)
    for n in dr.RAGGED:
        assert np.array_equal(api.is_right_handed(t[:n]), got[:n])
    assert np.array_equal(api.is_right_handed(t[-65:]), got[-65:])


@pytest.mark.parametrize("key", KEYS)
def test_stix_parameters_and_F(cases, key):
    from oracle import oracle

    c = cases[key]
    gpu, ref = c["gpu"], c["ref"]
    e = np.abs(gpu[:, 1:6] - ref[:, 1:6]) / np.maximum(np.abs(ref[:, 1:6]), 1.0)
    ef = np.abs(gpu[:, 0] - ref[:, 0]) / f_scale(c["rows"], ref, oracle.lib().so_speed_of_light())
    for fam, s in c["sl"].items():
        print("%s %-11s S D P R L worst %.3g of 1e-10; F worst %.3g of 1e-10 of its scale" % (key, fam, e[s].max(), ef[s].max()))
    assert e.max() <= 1e-10
    assert ef.max() <= 1e-10


@pytest.mark.parametrize("key", KEYS)
def test_roots_in_the_references_order(cases, gmodels, key):
    c = cases[key]
    gpu, ref, m = c["gpu"], c["ref"], c["m"]
    assert np.all(np.isfinite(gpu))
    bar = 1e-10 * m["kappa"]
    lived = ~c["stopped"]
    eo, eu = dr.ordered_errors(gpu, ref), dr.unordered_errors(gpu, ref)
    comp = m["comparable"] & lived
    rest = ~m["comparable"] & lived
    for fam, s in c["sl"].items():
        print("%s %-11s ordered: worst %.3g of its bar on %d rows; outside the comparable set %.3f (%d rows, unordered worst %.3g "
              "of its bar, %d of them in the other order); stopped %d" % (
                  key, fam, (eo / bar)[s][comp[s]].max(), comp[s].sum(), 1.0 - m["comparable"][s].mean(), rest[s].sum(),
                  (eu / bar)[s][rest[s]].max() if rest[s].any() else 0.0, (eo > bar)[s][rest[s]].sum(), c["stopped"][s].sum()))
    assert np.all(eo[comp] <= bar[comp]), "%d rows" % (eo[comp] > bar[comp]).sum()
    assert np.all(eu[rest] <= bar[rest]), "%d rows" % (eu[rest] > bar[rest]).sum()
    # ragged calls see the same bits per row
    rows = c["rows"][c["sl"]["uniform"]]
    for n in dr.RAGGED:
        alone = gmodels[key].dispersion(rows[:n, 0:3], rows[:n, 3:6], rows[:n, 6])
        assert alone.tobytes() == gpu[c["sl"]["uniform"]][:n].tobytes()
    assert gmodels[key].dispersion(rows[:0, 0:3], rows[:0, 3:6], rows[:0, 6]).shape == (0, 10)


@pytest.mark.parametrize("key", KEYS)
def test_aligned_rows_with_cos2_above_one(g, cases, key):
    """k = s B0 with cos^2 rounded above 1 (SURVEY A-2: the reference stops or sees a NaN angle): the clamp makes phi = 0."""
    c = cases[key]
    s = c["sl"]["aligned"]
    gpu, tl, m = c["gpu"][s], g["%s_aligned_tilted" % key], {k: v[s] for k, v in c["m"].items()}
    over = m["cos2"] > 1.0
    sel = over & (m["sep"] > dr.ROOT_SEP_MIN)
    assert sel.sum() >= 25 and np.all(np.isfinite(gpu[over]))
    e = dr.ordered_errors(gpu, tl)
    print("%s: cos2 > 1 on %d rows (%d of them stopped the reference), worst ordered error against the tilted direction %.3g" % (
        key, over.sum(), (over & c["stopped"][s]).sum(), e[sel].max()))
    assert np.all(e[sel] <= 1e-5), "%d of %d rows ordered otherwise" % ((e[sel] > 1e-5).sum(), sel.sum())


def test_zero_density(g, gmodels):
    """ln N = -800 at every node.  The fixed-step trace: bars in the module docstring (ten times the reference's own 2.03e-9)."""
    from oracle import oracle
    from stanford_raytracer_amd import workloads as wl

    gm, rows, ref = gmodels["zero"], g["zero_in"], g["zero_disp"]
    pp = gm.plasma_params(rows[:, 0:3])
    assert np.array_equal(pp[:, 4:8], np.zeros((len(rows), 4))), pp[:, 4:8].max()
    out = gm.dispersion(rows[:, 0:3], rows[:, 3:6], rows[:, 6])
    c = oracle.lib().so_speed_of_light()
    n2 = (np.linalg.norm(rows[:, 3:6], axis=1) * c / rows[:, 6]) ** 2
    assert np.all(np.abs(out[:, 0] - (1.0 - n2)) <= 1e-13 * np.maximum(1.0, n2))
    assert np.all(np.abs(out[:, 1:6] - ref[:, 1:6]) <= 1e-10)
    for col in (6, 8):
        e = np.abs(out[:, col] - rows[:, 6] / c) / (rows[:, 6] / c)
        print("zero density: root column %d worst %.3g of w / c" % (col, e.max()))
        assert np.all(e <= 1e-14) and np.all(out[:, col + 1] == 0)
    pos, d, w = wl.launch_set(8, 5)
    r, nrows, stop, _ = gm.trace(pos, d, w, outputper=1, minalt=wl.MINALT, **ZERO_KW)
    assert np.array_equal(nrows, g["zero_run_nrows"]) and np.array_equal(stop, g["zero_run_stop"])
    rr, own = g["zero_run_rows"], float(g["zero_run_line_dev"])
    assert 1e-9 <= own <= 3e-9
    T = rr.shape[1]
    assert np.allclose(r[:, :T, 0], rr[:, :, 0], rtol=1e-14, atol=0)
    e = np.linalg.norm(r[:, :T, 1:4] - rr[:, :, 1:4], axis=2) / np.linalg.norm(rr[:, :, 1:4], axis=2)
    line = pos[:, None, :] + c * rr[:, :, 0:1] * d[:, None, :]
    el = np.linalg.norm(r[:, :T, 1:4] - line, axis=2) / np.linalg.norm(line, axis=2)
    print("zero density trace: positions within %.3g of the reference's, %.3g of the straight line (reference: %.3g)" % (
        e.max(), el.max(), own))
    assert e.max() <= 10.0 * own and el.max() <= 10.0 * own


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("root", [1, 2])
def test_launch_rows(cases, omodels, gmodels, key, root):
    """One trace with maxsteps = 1 over the `uniform` and `aligned` families: the launch row is solve_dispersion's chosen root along
    dir0.  Stop code 2 exactly where the oracle's chosen root has Re k = 0, else row-0 n within 1e-10 kappa of the oracle's (on the
    comparable set: elsewhere the two may name the roots the other way round)."""
    from stanford_raytracer_amd import workloads as wl

    c = cases[key]
    idx = np.concatenate([np.arange(dr.N_STATES * len(dr.FAMILIES))[c["sl"][fam]] for fam in ("uniform", "aligned")])
    rows, m = c["rows"][idx], {k: v[idx] for k, v in c["m"].items()}
    kw = dict(fixedstep=1, dt0=1e-3, dtmax=0.1, tmax=1.0, maxerr=5e-4, maxsteps=1, root=root, del_=1e-6, minalt=wl.MINALT)
    r, nrows, stop, _ = gmodels[key].trace(rows[:, 0:3], rows[:, 3:6], rows[:, 6], outputper=1, **kw)
    with np.errstate(all="ignore"):
        orr, onrows, ostop, _ = omodels[key].trace(rows[:, 0:3], rows[:, 3:6], rows[:, 6], capacity=2, **kw)
    comp = m["comparable"]
    dead = np.linalg.norm(orr[:, 0, 10:13], axis=1) == 0
    print("%s root %d: %d launch rows, %d comparable, %d of them evanescent (stop 2), %d stop codes differ outside the comparable "
          "set" % (key, root, len(rows), comp.sum(), (dead & comp).sum(), (stop != ostop)[~comp].sum()))
    assert 0 < (dead & comp).sum() < comp.sum()
    assert np.array_equal(stop[comp] == 2, dead[comp]) and np.array_equal(stop[comp], ostop[comp])
    assert np.array_equal(nrows[comp], onrows[comp])
    live = comp & ~dead
    e = vrel(r[live, 0, 10:13], orr[live, 0, 10:13])
    print("   row-0 n: worst %.3g of its bar" % (e / (1e-10 * m["kappa"][live])).max())
    assert np.all(e <= 1e-10 * m["kappa"][live])
    assert np.array_equal(r[live, 0, 1:4], orr[live, 0, 1:4])


@pytest.mark.parametrize("key", KEYS)
def test_gradients_on_the_surface(cases, omodels, gmodels, key):
    """dF/dk, dF/dw and dx/dt of srt_gradients against oracle.grad at on-surface states of every family (dF/dx is left out: the
    float32 staircase of B decides it).  Bars per density in the module docstring."""
    c = cases[key]
    st = np.concatenate([dr.on_surface(c["rows"][s], c["judge"][s], c["m"]["comparable"][s]) for s in c["sl"].values()])
    assert len(st) >= 40
    got = gmodels[key].gradients(st[:, 0:3], st[:, 3:6], st[:, 6], 1e-6)
    ref = np.array([omodels[key].grad(r[0:3], r[3:6], r[6], 1e-6) for r in st])
    e = (vrel(got[:, 0:3], ref[:, 0:3]), np.abs(got[:, 3] - ref[:, 3]) / np.abs(ref[:, 3]), vrel(got[:, 7:10], ref[:, 7:10]))
    bars = GRAD_BARS[key]
    print("%s: %d on-surface states, f %.3g ... %.3g Hz; dF/dk %.3g (bar %.3g), dF/dw %.3g (bar %.3g), dx/dt %.3g (bar %.3g)" % (
        key, len(st), st[:, 6].min() / (2 * np.pi), st[:, 6].max() / (2 * np.pi), e[0].max(), bars[0], e[1].max(), bars[1],
        e[2].max(), bars[2]))
    for err, bar in zip(e, bars):
        assert err.max() <= bar
