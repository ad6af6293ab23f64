"""The IGRF synthesis at its edges: the geographic-pole branch, every truncation degree and the boundaries between them,
the date set-up at its epoch boundaries, and the two forms of igrf_core's double loop (stanford_raytracer_amd/csrc/srt_device.hpp).
CPU: the oracle against goldens captured from the reference at those edges (tests/golden/igrf_edges_golden.npz,
make_igrf_edges_golden.py), and srt_host::igrf_setup compiled for the host (tests/native/igrf_host.cpp) against the oracle.
GPU: igrf_core<NP> called directly through the probe library (tests/native/igrf_probe.hip) against the oracle's IGRF_GSW_08 on
identical fp32 inputs and against itself form by form; then the public entry points on the same points.
Point families and the numpy fp32 restatement of the kernel's head live in tests/igrf_edge_cases.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import igrf_edge_cases as ec
from conftest import GOLDEN_DIR, ROOT
from stanford_raytracer_amd import workloads as wl

F32 = np.float32
TABLE = os.path.join(ROOT, "stanford_raytracer_amd", "data", "igrf_coeffs.txt")
FAMILIES = (ec.FAM_AXIS, ec.FAM_BIN, ec.FAM_PAIR, ec.FAM_DATE)
# the bars of tests/test_igrf.py::test_gpu_igrf_field_matches_reference_goldens
ERR_BAR, EXACT_SHARE = 2e-6, 0.9


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN_DIR, "igrf_edges_golden.npz"))


@pytest.fixture(scope="module")
def state(cfgfiles):
    """The oracle's G, H, REC, A and (cos, sin) of the tilt for the base date."""
    from oracle import oracle
    return oracle.Model.ngo(cfgfiles["ngo"], *ec.BASE_DATE).set_igrf(*ec.BASE_DATE).igrf_state()


@pytest.fixture(scope="module")
def hostlib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("igrfh") / "libigrfh.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-format-truncation", "-shared", "-fPIC", "-pthread", "-o", so,
                           os.path.join(ROOT, "tests", "native", "igrf_host.cpp")])
    L = C.CDLL(so)
    fp = C.POINTER(C.c_float)
    L.igh_setup.argtypes = [C.c_char_p, C.c_int, C.c_int, fp, fp, fp, fp, fp, C.c_char_p, C.c_int]
    return L


def host_setup(hostlib, path, yd, ms):
    G, H, REC, A, psi = (np.full(n, np.nan, dtype=F32) for n in (105, 105, 105, 9, 1))
    err = C.create_string_buffer(512)
    fp = C.POINTER(C.c_float)
    ok = hostlib.igh_setup(os.fsencode(path), int(yd), int(ms), *(v.ctypes.data_as(fp) for v in (G, H, REC, A, psi)), err, 512)
    return ok, (G, H, REC, A), err.value.decode()


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def field_errors(got, want):
    """(error relative to |H| per point, bit-equal per point) of fp32 fields got[n, 3] against want[n, 3]."""
    got, want = np.asarray(got, dtype=F32).reshape(-1, 3), np.asarray(want, dtype=F32).reshape(-1, 3)
    err = np.abs(got.astype(np.float64) - want).max(axis=1) / np.linalg.norm(want.astype(np.float64), axis=1)
    return err, np.all(bits(got) == bits(want), axis=1)


# ------------------------------------------------------------------------------------------------------------- CPU
def test_golden_families_sit_on_their_branches(gold, state):
    """The golden's points, through the kernel's fp32 head: the axis family is polar / just off the pole with >= 8 ulp32 to
    the threshold, every bin of int(r + 2) from 2 to 31 is there, and every boundary pair straddles its integer by >= 8 ulp32."""
    _, _, _, A, cs = state
    x, fam = gold["x"], gold["fam"]
    assert np.array_equal(gold["dates"], np.array([ec.BASE_DATE] + ec.BOUNDARY_DATES))
    ga, built = ec.axis_points_gsw(A)
    assert np.array_equal(x[fam == ec.FAM_AXIS], ec.gsw_to_sm(ga, cs))          # as the generator built them
    ec.check_axis(ec.head(A, ec.sm_to_gsw32(x[fam == ec.FAM_AXIS], cs)), built)
    ec.check_bins(ec.head(A, ec.sm_to_gsw32(x[fam == ec.FAM_BIN], cs)))
    ec.check_pairs(ec.head(A, ec.sm_to_gsw32(x[fam == ec.FAM_PAIR], cs)))
    assert np.sum(fam == ec.FAM_DATE) == 20 * len(ec.BOUNDARY_DATES)
    for i in range(1, len(gold["dates"])):
        assert np.sum(gold["date_idx"] == i) == 20


def test_oracle_is_bit_identical_to_the_reference_at_the_edges(gold, cfgfiles):
    from oracle import oracle
    x, fam, didx = gold["x"], gold["fam"], gold["date_idx"]
    mine = np.zeros_like(gold["B"])
    for i, (yd, ms) in enumerate(gold["dates"]):
        o = oracle.Model.ngo(cfgfiles["ngo"], int(yd), int(ms)).set_igrf(int(yd), int(ms))
        for j in np.nonzero(didx == i)[0]:
            mine[j] = o.plasma_params(x[j])[4]
    for f in FAMILIES:
        assert np.array_equal(mine[fam == f], gold["B"][fam == f]), ec.FAMILY_NAMES[f]
    for i in range(len(gold["dates"])):
        assert np.array_equal(mine[didx == i], gold["B"][didx == i]), "date %d" % i


def test_oracle_igrf_gsw_wrapper_is_the_models_field(gold, cfgfiles, state):
    """oracle.igrf_gsw on the accessor's arrays and the fp32 GSW positions is what the model's own field tail evaluates."""
    from oracle import oracle
    G, H, REC, A, cs = state
    sel = gold["date_idx"] == 0
    h = oracle.igrf_gsw(G, H, REC, A, ec.sm_to_gsw32(gold["x"][sel], cs)).astype(np.float64) * 1e-9
    B = np.stack([h[:, 0] * cs[0] + h[:, 2] * cs[1], h[:, 1], h[:, 2] * cs[0] - h[:, 0] * cs[1]], axis=1)
    assert np.abs(B - gold["B"][sel]).max() <= 1e-15 * np.abs(gold["B"][sel]).max()
    with pytest.raises(RuntimeError):
        oracle.Model.ngo(cfgfiles["ngo"]).igrf_state()


def test_host_date_setup_is_bit_identical_to_the_oracle(hostlib, cfgfiles):
    """srt_host::igrf_setup, host build: year clamps (1960 -> 1965, 2031 -> 2025), epoch boundaries, the change to
    secular-variation extrapolation at 2020, day 366, the last millisecond of a day."""
    from oracle import oracle
    seen = []
    for yd, ms in [ec.BASE_DATE] + ec.BOUNDARY_DATES:
        want = oracle.Model.ngo(cfgfiles["ngo"], yd, ms).set_igrf(yd, ms).igrf_state()
        ok, got, err = host_setup(hostlib, TABLE, yd, ms)
        assert ok == 1 and err == "", (yd, err)
        for name, g, w in zip("G H REC A".split(), got, want[:4]):
            assert np.array_equal(bits(g), bits(w)), (yd, ms, name)
        seen.append(np.concatenate(got))
    d = dict(zip([ec.BASE_DATE] + ec.BOUNDARY_DATES, seen))
    assert np.array_equal(bits(d[(1960001, 0)]), bits(d[(1965001, 0)]))        # the clamps, not extrapolations
    assert np.array_equal(bits(d[(2025001, 0)]), bits(d[(2031001, 0)]))
    assert not np.array_equal(d[(1969365, 0)][:105], d[(1970001, 0)][:105])
    assert not np.array_equal(d[(2019365, 0)][:105], d[(2020001, 0)][:105])


def test_bad_coefficient_tables_are_refused(hostlib, tmp_path, cfgfiles):
    from oracle import oracle
    lines = open(TABLE).read().splitlines(keepends=True)
    text = "".join(lines)
    cases = {"missing": None, "empty": "", "half": "".join(lines[:110]), "one_row_short": "".join(lines[:-1]),
             "cut_in_the_last_row": text[:len(text) - 30], "binary": "\x00\x01\x02" * 500,
             "wrong_rows": "".join(ln for ln in lines if not ln.startswith("g"))}
    for name, content in cases.items():
        path = str(tmp_path / (name + ".txt"))
        if content is not None:
            open(path, "w").write(content)
        ok, _, err = host_setup(hostlib, path, 2010001, 0)
        assert ok == 0 and "IGRF coefficient table" in err and path in err, (name, ok, err)
    ok, _, err = host_setup(hostlib, str(tmp_path), 2010001, 0)                   # a directory
    assert ok == 0 and "IGRF coefficient table" in err
    with pytest.raises(RuntimeError):
        oracle.Model.ngo(cfgfiles["ngo"]).set_igrf(2010001, 0, coeff_file=str(tmp_path / "half.txt"))
    ok, _, err = host_setup(hostlib, TABLE, 2010001, 0)
    assert ok == 1 and err == ""


# ------------------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def probe():
    from stanford_raytracer_amd import build as pkg_build
    L = C.CDLL(pkg_build.build_probe())
    fp = C.POINTER(C.c_float)
    L.igp_igrf.argtypes = [fp, fp, fp, fp, C.c_int, C.c_long, fp, fp]

    def run(G, H, REC, A, npts, pos):
        """pos[n, npts, 3] fp32 GSW Earth radii -> the device's igrf_core<npts> fields [n, npts, 3]"""
        pos = np.ascontiguousarray(pos, dtype=F32).reshape(-1, npts, 3)
        out = np.zeros_like(pos)
        arrs = [np.ascontiguousarray(v, dtype=F32) for v in (G, H, REC, A)]
        rc = L.igp_igrf(*(v.ctypes.data_as(fp) for v in arrs), npts, pos.shape[0], pos.ctypes.data_as(fp), out.ctypes.data_as(fp))
        assert rc == 0, "igp_igrf: %d" % rc
        return out
    return run


IDENTITY = np.eye(3, dtype=F32).reshape(9)


def on_axis_gsw(A, r, sign, t=0.0, across=0):
    ax, e1, e2 = ec.geo_axis_frame(A)
    return r * (sign * np.sqrt(1.0 - t * t) * ax + t * (e1, e2)[across])


def one_point_families(gold, state):
    """name -> (A, fp32 GSW points [n, 3], check(head) or None)"""
    _, _, _, A, cs = state
    rng = np.random.default_rng(51)
    x, fam = gold["x"], gold["fam"]
    fams = {}
    fams["shell"] = (A, (ec.unit_vectors(rng, 1000) * rng.uniform(1.02, 9.0, (1000, 1))).astype(F32), None)
    _, built = ec.axis_points_gsw(A)
    fams["axis"] = (A, ec.sm_to_gsw32(x[fam == ec.FAM_AXIS], cs), lambda h: ec.check_axis(h, built))
    r = np.linspace(0.9, 29.5, 64)
    zax = np.zeros((64, 3))
    zax[:, 2] = r * np.where(np.arange(64) % 2 == 0, 1.0, -1.0)

    def exact_axis(h):
        assert np.all(h["s"] == 0) and np.all(h["rho"] == 0) and np.all(h["pole"])
        assert np.sum(h["c"] == 1) == 32 and np.sum(h["c"] == -1) == 32 and set(h["k"]) == {4, 5, 6, 7, 8, 9, 10, 11, 14}
    fams["identity A, s = 0"] = (IDENTITY, zax.astype(F32), exact_axis)
    fams["degree bins"] = (A, ec.sm_to_gsw32(x[fam == ec.FAM_BIN], cs), ec.check_bins)
    fams["boundary pairs"] = (A, ec.sm_to_gsw32(x[fam == ec.FAM_PAIR], cs), ec.check_pairs)
    def all_k4(h):
        assert np.all(h["k"] == 4)
    fams["wave at k = 4"] = (A, (ec.unit_vectors(rng, 64) * rng.uniform(29.1, 40.0, (64, 1))).astype(F32), all_k4)
    pw = np.array([on_axis_gsw(A, rr, sg, t, i % 2) for i, (rr, sg, t) in enumerate(
        zip(rng.uniform(1.02, 9.0, 64), np.where(np.arange(64) % 3 == 0, -1.0, 1.0), rng.uniform(0.0, 5e-6, 64)))])

    def all_pole(h):
        assert np.all(h["pole"]) and np.all(ec.ulps_from(h["s"], ec.POLE_S) >= 8) and np.any(h["c"] < 0) and np.any(h["c"] > 0)
    fams["wave at the pole"] = (A, pw.astype(F32), all_pole)
    mix = ec.unit_vectors(rng, 64) * ec.bin_radii()[np.arange(64) % 30][:, None]

    def every_k(h):
        assert set(h["k"]) == {4, 5, 6, 7, 8, 9, 10, 11, 14}             # 12 and 13 cannot occur: 30 // int(r + 2) skips 8 and 9
    fams["wave mixing k = 4 .. 14"] = (A, mix.astype(F32), every_k)
    return fams


@pytest.mark.gpu
def test_gpu_one_point_form_matches_the_oracle_bit_for_bit(gold, state, probe, capsys):
    """igrf_core<1> against the oracle's IGRF_GSW_08 on identical fp32 inputs, family by family.  Both are the same unfused
    IEEE fp32 operations in the same order (division and square root correctly rounded on both sides), so every point of
    every family is bit-equal; the bars of test_igrf.py hold a fortiori, per family."""
    from oracle import oracle
    G, H, REC, _, _ = state
    report = []
    for name, (A, pts, check) in one_point_families(gold, state).items():
        if check is not None:
            check(ec.head(A, pts))
        got = probe(G, H, REC, A, 1, pts).reshape(-1, 3)
        want = oracle.igrf_gsw(G, H, REC, A, pts)
        assert np.all(np.isfinite(want)) and np.all(np.isfinite(got)), name
        err, same = field_errors(got, want)
        report.append("%-26s n = %4d  worst error %.3g of |H|  bit-equal %.4f" % (name, len(pts), err.max(), same.mean()))
        with capsys.disabled():
            print("\nIGRF one-point form:", report[-1])
        assert err.max() <= ERR_BAR and same.mean() >= EXACT_SHARE, report[-1]
        assert same.all(), report[-1]


# --- stencils: a centre, +- delta r along each axis, and a free eighth point
def stencils(centres, delta, rng, free_scale=5.0):
    c = np.asarray(centres, dtype=np.float64)
    r = np.linalg.norm(c, axis=1)[:, None]
    pts = [c]
    for ax in range(3):
        for sg in (1.0, -1.0):
            p = c.copy()
            p[:, ax] += sg * delta * r[:, 0]
            pts.append(p)
    pts.append(c + free_scale * delta * r * ec.unit_vectors(rng, len(c)))
    return np.stack(pts, axis=1).astype(F32)                                     # [n, 8, 3]


def wave_composition(A, st):
    """Per wave of stencils st[64, NP, 3]: does the paired form run (every lane: one degree, no pole), kmax, per-lane k[0]."""
    n, NP, _ = st.shape
    assert n == 64
    h = ec.head(A, st.reshape(-1, 3))
    k, pole = h["k"].reshape(n, NP), h["pole"].reshape(n, NP)
    samek = np.all(k == k[:, :1], axis=1) & ~np.any(pole, axis=1)
    return {"paired": bool(samek.all()), "samek": samek, "kmax": int(k.max()), "k": k, "pole": pole, "h": h}


def in_bin(rng, n, lo, hi):
    return ec.unit_vectors(rng, n) * rng.uniform(lo, hi, (n, 1))


def form_waves(A, delta, rng):
    """name -> (stencils[64, 8, 3], check(composition for NP points))"""
    waves = {}
    # shared degree, no pole: the paired form; wave maxima 14, 11, 10 and 4 (kmax - m takes both parities in each;
    # the odd / even TOTAL trip count of the twice-unrolled n loop differs between 14 / 10 / 4 and 11)
    for kk, (lo, hi) in {14: (1.1, 1.9), 11: (2.1, 2.9), 10: (3.1, 3.9), 4: (29.2, 35.0)}.items():
        waves["paired, k = %d" % kk] = (stencils(in_bin(rng, 64, lo, hi), delta, rng),
                                        lambda w, kk=kk: w["paired"] and w["kmax"] == kk and np.all(w["k"] == kk))
    # one lane much closer to the Earth: kmax > kl for the 63 others, odd (14 - 11) and even (14 - 8) difference
    for kl, (lo, hi) in {11: (2.1, 2.9), 8: (5.1, 5.9)}.items():
        c = in_bin(rng, 64, lo, hi)
        c[5] = in_bin(rng, 1, 1.2, 1.8)[0]
        waves["paired, kmax 14 > kl = %d" % kl] = (stencils(c, delta, rng), lambda w, kl=kl: w["paired"] and w["kmax"] == 14 and
                                                   np.sum(w["k"][:, 0] == kl) == 63 and w["k"][5, 0] == 14)
    # one lane whose stencil straddles an integer of r + 2: the per-point form for the whole wave
    c = in_bin(rng, 64, 2.1, 2.9)
    c[40] = 3.0 * np.array([0.9, 0.3, 0.3]) / np.linalg.norm([0.9, 0.3, 0.3])    # +- delta r along x: +- 0.9 delta in r

    def straddles(w):
        rp2 = w["h"]["rp2"].reshape(64, -1)[40].astype(np.float64)
        ulp = float(np.spacing(F32(5.0)))
        return (not w["paired"] and np.sum(~w["samek"]) == 1 and set(w["k"][40]) == {10, 11} and not w["pole"].any() and
                np.any(rp2 <= 5.0 - 4 * ulp) and np.any(rp2 >= 5.0 + 4 * ulp))
    waves["one lane straddles r + 2 = 5"] = (stencils(c, delta, rng), straddles)
    # one lane centred on the geographic axis
    c = in_bin(rng, 64, 2.1, 2.9)
    c[9] = on_axis_gsw(A, 2.5, -1.0)
    c[33] = on_axis_gsw(A, 2.3, 1.0)
    if delta > 5e-5:
        chk = lambda w: (not w["paired"] and np.sum(~w["samek"]) == 2 and w["pole"][9].any() and not w["pole"][9].all() and  # noqa: E731
                         w["pole"][33].any() and not w["pole"][33].all() and np.all(ec.ulps_from(w["h"]["s"], ec.POLE_S) >= 8))
        waves["axis lanes, pole and non-pole points mixed"] = (stencils(c, delta, rng), chk)
    else:
        chk = lambda w: (not w["paired"] and np.sum(~w["samek"]) == 2 and w["pole"][9].all() and w["pole"][33].all() and  # noqa: E731
                         np.all(ec.ulps_from(w["h"]["s"], ec.POLE_S) >= 8))
        waves["axis lanes, all points polar"] = (stencils(c, delta, rng), chk)
    return waves


@pytest.mark.gpu
@pytest.mark.parametrize("delta", [1e-6, 1e-4])
@pytest.mark.parametrize("NP", [7, 8])
def test_gpu_forms_agree_bit_for_bit(state, probe, NP, delta, capsys):
    """igrf_core<7> and igrf_core<8> -- the packed paired form and the per-point form, wave by wave as composed below --
    against igrf_core<1> on each point alone: the same bits (the code's own claim), and the bars of the one-point test
    against the oracle."""
    from oracle import oracle
    G, H, REC, A, _ = state
    rng = np.random.default_rng(77)
    waves = form_waves(A, delta, rng)
    assert len(waves) == 8
    forms = set()
    for name, (st8, check) in waves.items():
        st = np.ascontiguousarray(st8[:, :NP])
        comp = wave_composition(A, st)
        assert check(comp), "wave '%s' (NP = %d, delta = %g) is not composed as intended" % (name, NP, delta)
        forms.add(comp["paired"])
        got = probe(G, H, REC, A, NP, st).reshape(-1, 3)
        alone = probe(G, H, REC, A, 1, st.reshape(-1, 3)).reshape(-1, 3)
        want = oracle.igrf_gsw(G, H, REC, A, st.reshape(-1, 3))
        err, same = field_errors(got, want)
        same1 = np.all(bits(got) == bits(alone), axis=1)
        with capsys.disabled():
            print("\nIGRF forms NP = %d delta = %g: %-44s %s  vs one-point form %.4f bit-equal; vs oracle worst %.3g, bit-equal %.4f"
                  % (NP, delta, name, "paired   " if comp["paired"] else "per-point", same1.mean(), err.max(), same.mean()))
        assert same1.all(), (name, int((~same1).sum()), np.nonzero(~same1)[0][:8] // NP)
        assert err.max() <= ERR_BAR and same.mean() >= EXACT_SHARE, (name, err.max(), same.mean())
    assert forms == {True, False}


@pytest.mark.gpu
def test_gpu_short_last_wave_repeats_its_last_stencil(state, probe):
    """n = 65 and n = 1 stencils: the lanes past n run the synthesis on a copy of the last stencil (the terms are read across
    the wave), and the stored results are those of the full-wave call."""
    G, H, REC, A, _ = state
    rng = np.random.default_rng(5)
    st = stencils(in_bin(rng, 128, 1.1, 8.0), 1e-4, rng)
    full = probe(G, H, REC, A, 8, st)
    for n in (1, 65):
        assert np.array_equal(bits(probe(G, H, REC, A, 8, st[:n])), bits(full[:n]))


@pytest.fixture(scope="module")
def public_models(cfgfiles, grid16):
    from stanford_raytracer_amd import api
    api.init(0)
    F, b, qs, ms_ = grid16

    def make(kind, yd, ms):
        m = api.Model.ngo(cfgfiles["ngo"], yd, ms) if kind == "ngo" else api.Model.interp(F, b, qs, ms_, yearday=yd, msec=ms)
        return m.set_field(use_igrf=1)
    return make


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ngo", "interp"])
def test_gpu_plasma_params_at_the_edges_matches_the_reference(gold, public_models, kind, capsys):
    """The public path (fp64 SM metres in, the adapters' whole field tail) at the golden's points and dates against the
    reference's B, with test_igrf.py's two bars applied family by family."""
    x, fam, didx = gold["x"], gold["fam"], gold["date_idx"]
    got = np.zeros_like(gold["B"])
    for i, (yd, ms) in enumerate(gold["dates"]):
        sel = didx == i
        got[sel] = public_models(kind, int(yd), int(ms)).plasma_params(x[sel])[:, 16:19]
    err = np.abs(got - gold["B"]).max(axis=1) / np.linalg.norm(gold["B"], axis=1)
    for f in FAMILIES:
        e = err[fam == f]
        with capsys.disabled():
            print("\nIGRF public path %-6s %-14s n = %3d  worst error %.3g of |B|  bit-equal %.4f"
                  % (kind, ec.FAMILY_NAMES[f], len(e), e.max(), np.mean(e <= 1e-14)))
        assert e.max() <= ERR_BAR, (ec.FAMILY_NAMES[f], e.max())
        assert np.mean(e <= 1e-14) >= EXACT_SHARE, (ec.FAMILY_NAMES[f], np.mean(e <= 1e-14))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ngo", "interp"])
def test_gpu_ragged_batches_with_igrf(gold, public_models, kind):
    """n = 1, 63, 65 with IGRF on: the same bits as the same points inside a 130-point batch (axis points, every degree bin
    and boundary pairs among them: the short waves' spare lanes repeat the last point)."""
    m = public_models(kind, *ec.BASE_DATE)
    x = np.concatenate([gold["x"][20:140], gold["x"][:10]])          # 130 points, axis points at both ends
    assert len(x) == 130
    full = m.plasma_params(x)
    for n in (1, 63, 65):
        for start in (0, 130 - n):
            part = m.plasma_params(x[start:start + n])
            assert np.array_equal(part, full[start:start + n]), (n, start)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ngo", "interp"])
def test_gpu_trace_rows_do_not_depend_on_the_form(state, public_models, kind):
    """64 fixed-step rays in one wave, then the same with ray 17 launched on the geographic axis at 2.5 R_E, which puts the
    whole wave on the per-point form: the other 63 rays' rows and stop codes are bit-equal."""
    _, _, _, A, cs = state
    m = public_models(kind, *ec.BASE_DATE)
    pos, d, w = wl.launch_set(64, 23)
    if kind == "interp":
        pos = pos * 0.9
    kw = dict(fixedstep=1, dt0=1e-3, dtmax=0.1, tmax=0.05, maxerr=5e-4, maxsteps=8, del_=1e-4, outputper=1)
    rows, nrows, stop, _ = m.trace(pos, d, w, **kw)
    pos2 = pos.copy()
    pos2[17] = ec.gsw_to_sm(on_axis_gsw(A, 2.5, 1.0), cs)
    h = ec.head(A, ec.sm_to_gsw32(pos2[17:18], cs))
    assert h["pole"][0] and h["s"][0] < 5e-6
    rows2, nrows2, stop2, _ = m.trace(pos2, d, w, **kw)
    others = np.arange(64) != 17
    assert np.mean(nrows[others] == 8) >= 0.9            # the rays do run (a few find no propagating mode at launch)
    assert np.array_equal(nrows[others], nrows2[others]) and np.array_equal(stop[others], stop2[others])
    a, b = rows[others], rows2[others]
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.nan_to_num(a), np.nan_to_num(b))
    assert not np.array_equal(np.nan_to_num(rows[17]), np.nan_to_num(rows2[17]))
