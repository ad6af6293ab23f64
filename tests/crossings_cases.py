"""Surface crossings along kept rows (include/srt.h): the numpy restatement the tests hold the library against, and the case
builders C1 .. C5 shared by the CPU tests (tests/test_crossings_host.py, the host build of csrc/srt_crossings.hpp) and the GPU
tests (tests/test_gpu_crossings.py).

The restatement has the header's definition and nothing of its code: the same g, the same Delta form of the cubic, a plain
bisection.  Where a truth exists that owes nothing to either (C1: the components are cubic in t, so the interpolant is the
curve itself and a plane's crossing time is a root of a cubic) it is used as well.

Bars (C1 .. C4), under the precondition the builders assert on the reference -- |dg/dsigma| at the root >= 0.1 (|g_i| + |g_i+1|),
i.e. the crossing is transversal, so that the rounding of g (1e-15 relative) moves sigma* by about 1e-14:
    |sigma* - sigma_ref| <= SIGMA_BAR = 1e-12,   |pos - pos_ref| <= POS_BAR (|x| + |Delta|) = 1e-12 (..),
    the definition itself: g has the interval's two end signs at sigma* -+ 2^-40,   the meta is equal."""
import numpy as np

ROW = 20
R_E = 6371.2e3
C_LIGHT = np.sqrt(1.0 / 8.854187817e-12 / (np.pi * 4e-7))  # constants.f95:4-7, as the library's models compute it
SIGMA_BAR = 1e-12
POS_BAR = 1e-12
DEF_STEP = 2.0 ** -40

SPHERE, LSHELL, MAGLAT, PLANE = 0, 1, 2, 3


# ---------------------------------------------------------------------------------------------- the restatement
def g_of(surface, x):
    """g(x) of surface = (kind, p[4]); x[..., 3] in SM metres."""
    kind, p = surface
    x = np.asarray(x, dtype=np.float64)
    if kind == PLANE:
        return p[0] * x[..., 0] + p[1] * x[..., 1] + p[2] * x[..., 2] - p[3]
    rho2 = x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1]
    r2 = rho2 + x[..., 2] * x[..., 2]
    r = np.sqrt(r2)
    if kind == SPHERE:
        return r - p[0]
    if kind == LSHELL:
        return r2 * r - (p[0] * R_E) * rho2
    return x[..., 2] - r * np.sin(p[0])


def usable(r0, r1):
    cols = [0, 1, 2, 3, 7, 8, 9]
    return bool(np.all(np.isfinite(r0[cols])) and np.all(np.isfinite(r1[cols])) and r1[0] != r0[0])


def curve(r0, r1, linear=False):
    """sigma -> position between two rows: the cubic Hermite curve in its Delta form, or the straight line."""
    h = r1[0] - r0[0]
    d = r1[1:4] - r0[1:4]
    if linear:
        return lambda s: r0[1:4] + s * d
    m0, m1 = C_LIGHT * r0[7:10] * h, C_LIGHT * r1[7:10] * h
    c2, c3 = 3.0 * d - 2.0 * m0 - m1, m0 + m1 - 2.0 * d
    return lambda s: r0[1:4] + s * (m0 + s * (c2 + s * c3))


def bisect(surface, p, neg0):
    lo, hi = 0.0, 1.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            break
        if (g_of(surface, p(mid)) < 0.0) == neg0:
            lo = mid
        else:
            hi = mid
    return hi if neg0 else lo


def reference(offsets, rows, surfaces, linear=False):
    """-> list of events (ray, surface index, interval, direction, sigma, row[20]) in the defined order."""
    out = []
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, ROW)
    for ray in range(len(offsets) - 1):
        for j in range(int(offsets[ray]), int(offsets[ray + 1]) - 1):
            r0, r1 = rows[j], rows[j + 1]
            if not usable(r0, r1):
                continue
            for si, s in enumerate(surfaces):
                n0, n1 = g_of(s, r0[1:4]) < 0.0, g_of(s, r1[1:4]) < 0.0
                if n0 == n1:
                    continue
                p = curve(r0, r1, linear)
                sig = bisect(s, p, n0)
                ev = r0 + sig * (r1 - r0)
                ev[0] = r0[0] + sig * (r1[0] - r0[0])
                ev[1:4] = p(sig)
                out.append((ray, si, j - int(offsets[ray]), 1 if n0 else -1, sig, ev))
    return out


def ref_arrays(events):
    meta = np.array([e[:4] for e in events], dtype=np.int32).reshape(-1, 4)
    sig = np.array([e[4] for e in events])
    ev = np.array([e[5] for e in events]).reshape(-1, ROW)
    return ev, meta, sig


def assert_transversal(offsets, rows, surfaces, events):
    """The precondition of the bars: |dg/dsigma| at the root >= 0.1 (|g_i| + |g_i+1|), by a central difference of the reference."""
    for ray, si, iv, _, sig, _ in events:
        j = int(offsets[ray]) + iv
        r0, r1 = rows[j], rows[j + 1]
        p, s = curve(r0, r1), surfaces[si]
        e = 1e-6
        a, b = max(sig - e, 0.0), min(sig + e, 1.0)
        slope = abs(g_of(s, p(b)) - g_of(s, p(a))) / (b - a)
        ends = abs(g_of(s, r0[1:4])) + abs(g_of(s, r1[1:4]))
        assert slope >= 0.1 * ends, ("not transversal", ray, si, iv, slope, ends)


def sigma_of(offsets, rows, ev, meta):
    """sigma* of each event, from its time: (t - t0) / h."""
    j = np.asarray(offsets)[meta[:, 0]] + meta[:, 2]
    return (ev[:, 0] - rows[j, 0]) / (rows[j + 1, 0] - rows[j, 0])


def check_against_reference(offsets, rows, surfaces, ev, meta, label=""):
    """The bars of the module's docstring; returns the figures (max sigma error, max relative position error, events)."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, ROW)
    events = reference(offsets, rows, surfaces)
    assert_transversal(offsets, rows, surfaces, events)
    rev, rmeta, rsig = ref_arrays(events)
    assert meta.shape == rmeta.shape and np.array_equal(meta, rmeta), (label, meta.tolist(), rmeta.tolist())
    if not len(events):
        return 0.0, 0.0, 0
    j = np.asarray(offsets)[meta[:, 0]] + meta[:, 2]
    r0, r1 = rows[j], rows[j + 1]
    h = r1[:, 0] - r0[:, 0]
    # sigma* from the event's time; t = t0 + sigma h rounds at |t|, so sigma is known from it to about 2^-52 |t| / |h|
    sig = (ev[:, 0] - r0[:, 0]) / h
    slack = 4.0 * 2.0 ** -52 * np.maximum(np.abs(r0[:, 0]), np.abs(r1[:, 0])) / np.abs(h)
    es = np.abs(sig - rsig)
    scale = np.linalg.norm(r0[:, 1:4], axis=1) + np.linalg.norm(r1[:, 1:4] - r0[:, 1:4], axis=1)
    ep = np.linalg.norm(ev[:, 1:4] - rev[:, 1:4], axis=1) / scale
    print("%s: %d events, sigma error max %.3g, position error max %.3g (|x| + |D|), bit-equal event rows %d / %d"
          % (label, len(events), es.max(), ep.max(), int(np.sum(np.all(ev == rev, axis=1))), len(ev)))
    assert np.all(es <= SIGMA_BAR + slack), (label, float(es.max()))
    assert np.all(ep <= POS_BAR), (label, float(ep.max()))
    # columns 4 .. 19 are linear in sigma
    lin = r0[:, 4:] + rsig[:, None] * (r1[:, 4:] - r0[:, 4:])
    tol = 1e-12 * (np.abs(r0[:, 4:]) + np.abs(r1[:, 4:])) + 1e-300
    assert np.all(np.abs(ev[:, 4:] - lin) <= tol), label
    # the definition, whatever the method: g has the two end signs at sigma* -+ 2^-40 (the rows' own signs beyond [0, 1])
    for k in range(len(ev)):
        s = surfaces[meta[k, 1]]
        p = curve(r0[k], r1[k])
        n0, n1 = g_of(s, r0[k, 1:4]) < 0.0, g_of(s, r1[k, 1:4]) < 0.0
        assert n0 != n1 and meta[k, 3] == (1 if n0 else -1)
        a, b = sig[k] - DEF_STEP, sig[k] + DEF_STEP
        na = n0 if a <= 0.0 else (g_of(s, p(a)) < 0.0)
        nb = n1 if b >= 1.0 else (g_of(s, p(b)) < 0.0)
        assert na == n0 and nb == n1, (label, k, sig[k])
    return float(es.max()), float(ep.max()), len(events)


# ---------------------------------------------------------------------------------------------- rows from curves
def rows_on_cubic(coef, times):
    """Rows at `times` on the curve p(t) = coef[0] + coef[1] t + coef[2] t^2 + coef[3] t^3 (coef[4, 3]), vgrel = p'(t) / C; the
    other columns are smooth functions of t, so that an event's linear columns can be checked."""
    t = np.asarray(times, dtype=np.float64)
    rows = np.zeros((len(t), ROW))
    rows[:, 0] = t
    rows[:, 1:4] = coef[0] + t[:, None] * (coef[1] + t[:, None] * (coef[2] + t[:, None] * coef[3]))
    rows[:, 7:10] = (coef[1] + t[:, None] * (2.0 * coef[2] + t[:, None] * 3.0 * coef[3])) / C_LIGHT
    rows[:, 4:7] = 0.5 + 0.1 * t[:, None] * np.array([1.0, -2.0, 3.0])
    rows[:, 10:13] = 20.0 - 3.0 * t[:, None] * np.array([1.0, 0.5, -1.5])
    rows[:, 13:16] = 1e-5 * (1.0 + t[:, None] * np.array([0.3, 0.2, -0.1]))
    rows[:, 16:20] = 1e9 * (1.0 + t[:, None] * np.array([0.5, 0.4, 0.05, 0.02]))
    return rows


def pack(ray_rows):
    """list of [k_i, 20] arrays -> offsets[n + 1], rows[total, 20]"""
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in ray_rows])]).astype(np.int64)
    rows = np.concatenate([np.asarray(r, dtype=np.float64).reshape(-1, ROW) for r in ray_rows]) if ray_rows else np.zeros((0, ROW))
    return offsets, np.ascontiguousarray(rows)


def reversed_cubic(coef):
    """q(t) = p(1 - t)"""
    a0, a1, a2, a3 = coef
    return np.array([a0 + a1 + a2 + a3, -(a1 + 2 * a2 + 3 * a3), a2 + 3 * a3, -a3])


# C1: an outbound arc from 1.15 R_E at -35 degrees of latitude to 3.4 R_E at +30 degrees, bent, and the same arc run backwards
C1_COEF = np.array([[1.15 * 0.82, 0.02, -1.15 * 0.57], [1.2, 0.15, 1.1], [0.9, -0.2, 1.6], [-0.3, 0.1, -0.43]]) * R_E
C1_SURFACES = [(SPHERE, [2.0 * R_E, 0, 0, 0]), (LSHELL, [2.6, 0, 0, 0]), (MAGLAT, [np.deg2rad(10.0), 0, 0, 0]),
               (PLANE, [0.3, -0.2, 1.0, 0.25 * R_E]), (MAGLAT, [0.0, 0, 0, 0]), (PLANE, [1.0, 0.0, 0.0, 2.2 * R_E])]
C1_TIMES = [np.array([0.0, 1.0]), np.array([0.0, 0.55, 1.0]), np.linspace(0.0, 1.0, 5), np.linspace(0.0, 1.0, 9),
            np.array([0.0, 0.07, 0.3, 0.41, 0.77, 0.9, 1.0])]


def c1_case():
    """-> offsets, rows, surfaces: one ray per time set and direction (10 rays, 2 .. 9 rows each)."""
    rays = []
    for coef in (C1_COEF, reversed_cubic(C1_COEF)):
        for t in C1_TIMES:
            rays.append(rows_on_cubic(coef, t))
    offsets, rows = pack(rays)
    return offsets, rows, C1_SURFACES


def c1_plane_truth(offsets, rows, surfaces, meta):
    """For the events of planes: the crossing time as a root of the cubic n . p(t) - d (numpy.roots, polished by two Newton steps
    in extended precision), expressed as sigma of the event's interval.  -> (indices of the plane events, their sigma)."""
    idx, sig = [], []
    nper = len(C1_TIMES)
    for k, (ray, si, iv, _) in enumerate(meta):
        kind, p = surfaces[si]
        if kind != PLANE:
            continue
        coef = C1_COEF if ray < nper else reversed_cubic(C1_COEF)
        nrm = np.array(p[:3], dtype=np.longdouble)
        c = (coef.astype(np.longdouble) @ nrm)
        c[0] -= np.longdouble(p[3])
        j = int(offsets[ray]) + iv
        t0, t1 = rows[j, 0], rows[j + 1, 0]
        roots = [z.real for z in np.roots(np.array(c[::-1], dtype=np.float64)) if abs(z.imag) < 1e-9 and t0 - 1e-9 <= z.real <= t1 + 1e-9]
        assert len(roots) == 1, (ray, si, iv, roots)
        t = np.longdouble(roots[0])
        for _ in range(2):
            t = t - (c[0] + t * (c[1] + t * (c[2] + t * c[3]))) / (c[1] + t * (2 * c[2] + t * 3 * c[3]))
        idx.append(k)
        sig.append(float((t - np.longdouble(t0)) / (np.longdouble(t1) - np.longdouble(t0))))
    return np.array(idx, dtype=np.int64), np.array(sig)


def c2_case():
    """A row exactly on the plane z = 0, coordinates representable: ray 0 passes -, 0, +; ray 1 passes +, 0, -."""
    def ray(sign):
        r = np.zeros((3, ROW))
        r[:, 0] = [0.0, 1.0, 2.0]
        r[:, 1] = [8388608.0, 8388608.0 + 4096.0, 8388608.0 + 8192.0]
        r[:, 3] = np.array([-1024.0, 0.0, 2048.0]) * sign
        r[:, 7] = 4096.0 / C_LIGHT
        r[:, 9] = np.array([1024.0, 1536.0, 2048.0]) * sign / C_LIGHT
        r[:, 16:20] = 1e9
        return r
    offsets, rows = pack([ray(1.0), ray(-1.0)])
    return offsets, rows, [(PLANE, [0.0, 0.0, 1.0, 0.0])]


def c3_cases():
    """name -> (offsets, rows, surfaces), none of which holds an event."""
    surf = [(PLANE, [0.0, 0.0, 1.0, 0.0]), (SPHERE, [2.0 * R_E, 0, 0, 0])]
    base = rows_on_cubic(C1_COEF, np.array([0.0, 1.0]))  # crosses both surfaces in its one interval
    out = {}
    for name, col, which in (("nan_pos", 2, 0), ("nan_t", 0, 1), ("nan_vgrel", 8, 1), ("inf_pos", 3, 1)):
        r = base.copy()
        r[which, col] = np.inf if name.startswith("inf") else np.nan
        out[name] = pack([r]) + (surf,)
    r = base.copy()
    r[1, 0] = r[0, 0]
    out["t1_equals_t0"] = pack([r]) + (surf,)
    out["one_row_ray"] = pack([base[:1]]) + (surf,)
    # the rows either side of a ray boundary differ in sign: no event may come from the pair
    out["rays_of_one_row"] = pack([base[:1], base[1:]]) + (surf,)
    out["nrays_0"] = (np.zeros(1, dtype=np.int64), np.zeros((0, ROW)), surf)
    return out


def c3_empty_between():
    """An empty ray between two others: the events are those of the two, and the second is ray 2."""
    a = rows_on_cubic(C1_COEF, np.linspace(0.0, 1.0, 5))
    b = rows_on_cubic(reversed_cubic(C1_COEF), np.linspace(0.0, 1.0, 4))
    offsets, rows = pack([a, np.zeros((0, ROW)), b])
    return offsets, rows, C1_SURFACES[:4]


def c4_case(nsurf):
    """Order and counts: 3 rays on the C1 arcs, nsurf surfaces (1 or 16); with 16, surfaces 3 and 11 are identical."""
    rays = [rows_on_cubic(C1_COEF, np.linspace(0.0, 1.0, 9)), rows_on_cubic(reversed_cubic(C1_COEF), np.linspace(0.0, 1.0, 6)),
            rows_on_cubic(C1_COEF, np.array([0.0, 0.2, 0.5, 1.0]))]
    offsets, rows = pack(rays)
    if nsurf == 1:
        return offsets, rows, [C1_SURFACES[0]]
    surf = [(SPHERE, [(1.4 + 0.12 * k) * R_E, 0, 0, 0]) for k in range(6)] + \
           [(MAGLAT, [np.deg2rad(-25.0 + 9.0 * k), 0, 0, 0]) for k in range(5)] + \
           [(SPHERE, [(1.4 + 0.12 * 3) * R_E, 0, 0, 0])] + \
           [(LSHELL, [2.0 + 0.4 * k, 0, 0, 0]) for k in range(2)] + \
           [(PLANE, [0.1 * k, 0.05, 1.0, (0.2 * k - 0.1) * R_E]) for k in range(2)]
    assert len(surf) == 16 and surf[3] == surf[11]
    return offsets, rows, surf


# ---------------------------------------------------------------------------------------------- C5: real trajectories
def c5_surfaces():
    return [(SPHERE, [1.3 * R_E, 0, 0, 0]), (MAGLAT, [0.0, 0, 0, 0]), (MAGLAT, [np.deg2rad(20.0), 0, 0, 0]), (LSHELL, [2.0, 0, 0, 0])]


C5_NAMES = ["sphere 1.3 R_E", "magnetic equator", "latitude 20 deg", "L = 2"]
C5_TRACE = dict(fixedstep=0, tmax=2.0, maxsteps=2000, del_=1e-4)  # the other parameters at their defaults


def thin(offsets, rows, every):
    """Every `every`-th kept row of each ray (rows 0, every, 2 every, ..), packed."""
    return pack([rows[int(offsets[r]):int(offsets[r + 1]):every] for r in range(len(offsets) - 1)])


def c5_figures(full, hermite, linear, nsurf=4):
    """full / hermite / linear = (event_rows, meta) located from all rows, and from the thinned rows on the Hermite curve and on
    the straight line.  Events are matched pair by pair (ray, surface) in order; pairs with unequal counts are left out.
    -> dict of the figures the conditions are stated on."""
    def by_pair(ev, meta):
        d = {}
        for e, m in zip(ev, meta):
            d.setdefault((int(m[0]), int(m[1])), []).append(e[1:4])
        return d
    F, H, Ln = by_pair(*full), by_pair(*hermite), by_pair(*linear)
    pairs = sorted(set(F) | set(H) | set(Ln))
    left_out = [k for k in pairs if not (len(F.get(k, [])) == len(H.get(k, [])) == len(Ln.get(k, [])))]
    dh, dl = {s: [] for s in range(nsurf)}, {s: [] for s in range(nsurf)}
    for k in pairs:
        if k in left_out:
            continue
        for a, b, c in zip(F[k], H[k], Ln[k]):
            dh[k[1]].append(np.linalg.norm(b - a))
            dl[k[1]].append(np.linalg.norm(c - a))
    allh, alll = np.concatenate([dh[s] for s in dh]), np.concatenate([dl[s] for s in dl])
    return {"pairs": len(pairs), "left_out": len(left_out), "matched": len(allh), "closer": float(np.mean(allh < alll)),
            "hermite_median": [float(np.median(dh[s])) if dh[s] else None for s in range(nsurf)],
            "linear_median": [float(np.median(dl[s])) if dl[s] else None for s in range(nsurf)],
            "events_full": len(full[1])}


def c5_report(fig, label):
    lines = ["%s: %d events from all rows; %d (ray, surface) pairs, %d left out for unequal counts; %d matched events, "
             "%.1f %% closer by Hermite" % (label, fig["events_full"], fig["pairs"], fig["left_out"], fig["matched"], 100 * fig["closer"])]
    for name, h, l in zip(C5_NAMES, fig["hermite_median"], fig["linear_median"]):
        lines.append("  %-18s Hermite median %10.4g m   linear median %10.4g m   ratio %.4g" % (name, h, l, h / l))
    return "\n".join(lines)


def c5_assert(fig):
    """The conditions of C5: at most 10 % of the pairs left out, at least 90 % of the matched events closer by Hermite, and per
    surface the Hermite median <= 0.25 x the linear median."""
    assert fig["matched"] > 0
    assert fig["left_out"] <= 0.10 * fig["pairs"], fig
    assert fig["closer"] >= 0.90, fig
    for h, l in zip(fig["hermite_median"], fig["linear_median"]):
        assert h is not None and l is not None and h <= 0.25 * l, fig
