"""Seeded inputs for the dispersion-solver tests across plasma regimes: shared by tests/golden/make_dispersion_regimes_golden.py,
tests/test_dispersion_regimes.py (CPU) and tests/test_gpu_dispersion_regimes.py, so that all three see the same rows.  Not a
test module.

* five tiny modelnum-3 grids (6^3 over +-6 R_E, ln N constant): N_e = 1e6, 1e8, 1e10, 1e12 m^-3 with ions 0.8 / 0.15 / 0.05, and
  one with ln N = -800 (every density exactly 0): they let solve_dispersion_relation be driven at any density;
* five families of states [x, k, w] per grid, 130 rows each (two full waves of 64 and two lanes of a third);
* four families of handedness tuples [n2, phi (degrees), S, D, P], 2 000 rows each;
* what decides whether a row can be compared root by root: `gap` (relative gap between the two least |eigenvalues| of the
  float32-rounded wave matrix: below 1e-6 the reference's SVD picks its vector arbitrarily), the separation of the two roots,
  and kappa = max(1, |B| / sqrt|B^2 - 4 A RLP|), the amplification of one ulp in S, D, P into n^2 through the discriminant.
"""
import numpy as np

from stanford_raytracer_amd import workloads as wl

GRIDS = {"ne6": 1.0e6, "ne8": 1.0e8, "ne10": 1.0e10, "ne12": 1.0e12}
ION_FRACTIONS = (0.8, 0.15, 0.05)
HALF_WIDTH = 6.0 * wl.R_E
FAMILIES = ("uniform", "across", "near_axis", "near_across", "aligned")
RH_FAMILIES = ("vlf", "hf", "mixed", "hf_off")
N_STATES = 130
N_TUPLES = 2000
RAGGED = (1, 65)
TILT = 1.0e-6            # radians: the yardstick direction for rows the reference cannot do
GAP_MIN = 1.0e-6
ROOT_SEP_MIN = 1.0e-6
KAPPA_MAX = 1.0e4
OUTSIDE_CAP = 0.10       # at most this share of a family outside the comparable set
EPS0 = 8.854187817e-12
C_LIGHT = 2.99792458e8
F_MIN = 10.0             # Hz
F_MAX = 30.0e6
# a wave far above the plasma frequency sees a vacuum: both roots within 1e-6 of each other, nothing to order.  Frequencies are
# therefore drawn log-uniformly up to this multiple of the electron plasma frequency (and never above F_MAX).
F_CAP_FPE = 3.0
# across B the two modes are n^2 = P and RL / S.  Above the gyrofrequency they differ by X Y^2 only where X = fpe^2 / f^2 is small
# (Y = fce / f), and by 1 / X where it is large (RL / S = -X + O(1) = P + O(1)): in both bands kappa passes 1e4 (27 % of the rows
# at N_e = 1e12 with a cap of 20 fce).  The two families across B are therefore also capped at the local electron gyrofrequency.
F_CAP_FCE = 1.0
# ... and start at 100 Hz: below it, across B, the roots stand 1e6 and more apart (n^2 ~ 1e5 against -3e11 at 16 Hz, N_e = 1e12) and
# the smaller one is B + sqrt(disc) with B ~ -sqrt(disc): one ulp in R, L, P moves it by 1e-10 of itself, which is the whole bar of
# the root comparison although kappa = 1 there.
F_MIN_ACROSS = 100.0


def uniform_grid(ne):
    """F[6, 6, 6, 4] = ln N_s, the same at every node, and its bounds."""
    F = np.empty((6, 6, 6, 4))
    F[..., 0] = np.log(ne)
    for i, fr in enumerate(ION_FRACTIONS):
        F[..., 1 + i] = np.log(ne * fr)
    return F, np.array([-HALF_WIDTH, HALF_WIDTH] * 3)


def zero_grid():
    """ln N = -800 everywhere: exp underflows to exactly 0 in fp64, so every density is 0."""
    return np.full((6, 6, 6, 4), -800.0), np.array([-HALF_WIDTH, HALF_WIDTH] * 3)


def grid(key):
    return zero_grid() if key == "zero" else uniform_grid(GRIDS[key])


def fpe(ne):
    return np.sqrt(ne * wl.Q_E ** 2 / (wl.MS[0] * EPS0)) / (2.0 * np.pi)


def _seed(*parts):
    return [20261019] + [sum(ord(ch) * (i + 1) for i, ch in enumerate(p)) if isinstance(p, str) else int(p) for p in parts]


def positions(rng, n):
    """r = 1.1 ... 5.5 R_E, any direction."""
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return u * (rng.uniform(1.1, 5.5, n) * wl.R_E)[:, None]


def field_at(om, x):
    """B0 of the model itself (oracle handle `om`) at x[n, 3]."""
    return np.array([om.plasma_params(p)[4] for p in x])


def _frame(b):
    bh = b / np.linalg.norm(b, axis=1, keepdims=True)
    ref = np.where(np.abs(bh[:, 2:3]) < 0.9, np.array([[0.0, 0.0, 1.0]]), np.array([[1.0, 0.0, 0.0]]))
    e1 = np.cross(bh, ref)
    e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
    return bh, e1, np.cross(bh, e1)


def frequencies(rng, n, ne, x=None):
    """Log-uniform from F_MIN to the caps above; x[n, 3]: cap at the gyrofrequency of the dipole there as well."""
    hi = np.full(n, min(F_MAX, F_CAP_FPE * fpe(ne)) if ne > 0 else F_MAX)
    if x is not None:
        fce = wl.Q_E * np.linalg.norm(wl.dipole_b(x), axis=1) / wl.MS[0] / (2.0 * np.pi)
        hi = np.minimum(hi, F_CAP_FCE * fce)
    return 2.0 * np.pi * np.exp(rng.uniform(np.log(F_MIN if x is None else F_MIN_ACROSS), np.log(hi)))


def states(family, key, om, n=N_STATES):
    """[n, 7] = x, k, w of one family on grid `key`; `om` is the oracle's handle of that grid (for its own B0)."""
    rng = np.random.default_rng(_seed(family, key))
    x = positions(rng, n)
    w = frequencies(rng, n, GRIDS.get(key, 0.0), x if family in ("across", "near_across") else None)
    b = field_at(om, x)
    bh, e1, e2 = _frame(b)
    az = rng.uniform(0.0, 2.0 * np.pi, n)[:, None]
    e = np.cos(az) * e1 + np.sin(az) * e2
    sgn = rng.choice([-1.0, 1.0], n)[:, None]
    kmag = (w / C_LIGHT) * 10.0 ** rng.uniform(-1.0, 2.0, n)       # |n| = 0.1 ... 100: F is exercised off the surface too
    if family == "uniform":
        th = rng.uniform(0.0, np.pi, n)[:, None]
        kh = np.cos(th) * bh + np.sin(th) * e
    elif family == "across":
        kh = np.cross(b, e1 * np.cos(az) + e2 * np.sin(az) + bh)   # one cross product with the model's own B0
        kh /= np.linalg.norm(kh, axis=1, keepdims=True)
    elif family == "near_axis":
        th = 10.0 ** rng.uniform(-8.0, -2.0, n)[:, None]
        kh = sgn * (np.cos(th) * bh + np.sin(th) * e)
    elif family == "near_across":
        th = 10.0 ** rng.uniform(-8.0, -2.0, n)[:, None] * sgn
        kh = np.cos(th) * e + np.sin(th) * bh
    elif family == "aligned":
        kh, kmag = b, (10.0 ** rng.uniform(-3.0, 3.0, n)[:, None] * sgn)[:, 0]
    else:
        raise ValueError(family)
    k = kh * kmag[:, None]
    if key in GRIDS:
        w = detuned(w, GRIDS[key], np.linalg.norm(b, axis=1), np.minimum(cos2phi(k, b), 1.0))
    return np.concatenate([x, k, w[:, None]], axis=1)


def tilted(rows, om):
    """The same states with k turned by TILT radians away from its direction (unit length: the roots depend on the direction
    only).  The yardstick for rows whose cos^2 rounds above 1."""
    x, k = rows[:, 0:3], rows[:, 3:6]
    kh = k / np.linalg.norm(k, axis=1, keepdims=True)
    _, e1, _ = _frame(field_at(om, x))
    return np.concatenate([x, np.cos(TILT) * kh + np.sin(TILT) * e1, rows[:, 6:7]], axis=1)


def dot3(a, b):
    """dot_product as the reference's compiler associates it."""
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cos2phi(k, b):
    """solve_dispersion_relation's cos^2 of the angle between k and B0, fp64, the reference's association."""
    return (dot3(k, b) * dot3(k, b)) / (dot3(k, k) * dot3(b, b))


def rh_matrix(t):
    """The real symmetric twin of the reference's wave matrix for tuples t[n, 5], entries rounded through float32, phi in
    DEGREES fed to cos / sin as the reference does."""
    n2, phi, S, D, P = (t[:, i] for i in range(5))
    cp, sp = np.cos(phi), np.sin(phi)
    f32 = lambda v: np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)   # noqa: E731
    with np.errstate(over="ignore", invalid="ignore"):
        a, d, b, c, e = f32(S - n2 * (cp * cp)), f32(D), f32(n2 * cp * sp), f32(S - n2), f32(P - n2 * (sp * sp))
    z = np.zeros_like(a)
    return np.stack([np.stack([a, d, b], -1), np.stack([d, c, z], -1), np.stack([b, z, e], -1)], -2)


def rh_gap(t):
    """Relative gap between the two least |eigenvalues| of rh_matrix(t): (|l2| - |l1|) / |l2|; 0 where the matrix is not finite."""
    T = rh_matrix(np.atleast_2d(t))
    ok = np.isfinite(T).all(axis=(1, 2))
    gap = np.zeros(len(T))
    if ok.any():
        a = np.sort(np.abs(np.linalg.eigvalsh(T[ok])), axis=1)
        gap[ok] = np.where(a[:, 1] > 0, (a[:, 1] - a[:, 0]) / np.where(a[:, 1] > 0, a[:, 1], 1.0), 0.0)
    return gap


def stix(w, ne, bmag):
    """S, D, P, R, L in numpy for N_e = ne with the grids' ion mix (only to DRAW tuples: no test compares against it)."""
    Ns = np.stack([ne] + [ne * fr for fr in ION_FRACTIONS], -1)
    wps2 = Ns * wl.QS ** 2 / wl.MS / EPS0
    wcs = wl.QS * bmag[:, None] / wl.MS
    ww = w[:, None]
    R = 1.0 - np.sum(wps2 / (ww * (ww + wcs)), -1)
    L = 1.0 - np.sum(wps2 / (ww * (ww - wcs)), -1)
    P = 1.0 - np.sum(wps2 / (ww * ww), -1)
    return 0.5 * (R + L), 0.5 * (R - L), P, R, L


def nsq_roots(S, D, P, R, L, c2):
    """Both n^2 of solve_dispersion_relation (complex), and A, B, discriminant."""
    s2 = 1.0 - c2
    A = S * s2 + P * c2
    B = R * L * s2 + P * S * (1.0 + c2)
    disc = B * B - 4.0 * A * R * L * P
    with np.errstate(divide="ignore", invalid="ignore"):
        sq = np.sqrt(disc.astype(complex))
        return (B + sq) / (2.0 * A), (B - sq) / (2.0 * A), A, B, disc


ULP_PATTERNS = ((1, -1, 1), (-1, 1, 1), (1, 1, -1), (1, -1, -1))
SENS_MAX = 1.0e-11       # of kappa: a tenth of the bar of the root comparison


def ulp_sensitivity(w, ne, bmag, c2):
    """How far one ulp in R, L and P moves the two roots, relative to each root and divided by kappa: the largest over four sign
    patterns.  kappa accounts for the discriminant only; this also sees a resonance (S = (R + L) / 2 or A = S sin^2 + P cos^2
    cancelling to 1e-5 of its terms) and a root 1e6 times smaller than the other (B + sqrt(disc) cancelling)."""
    S, D, P, R, L = stix(w, ne, bmag)
    q1, q2, _, B, disc = nsq_roots(S, D, P, R, L, c2)
    with np.errstate(divide="ignore", invalid="ignore"):
        kappa = np.maximum(1.0, np.abs(B) / np.sqrt(np.abs(disc)))
        worst = np.zeros(len(w))
        for sr, sl, sp in ULP_PATTERNS:
            R2, L2, P2 = R * (1.0 + sr * 2.3e-16), L * (1.0 + sl * 2.3e-16), P * (1.0 + sp * 2.3e-16)
            p1, p2, _, _, _ = nsq_roots(0.5 * (R2 + L2), 0.5 * (R2 - L2), P2, R2, L2, c2)
            e = np.maximum(np.abs(np.sqrt(p1) - np.sqrt(q1)) / np.abs(np.sqrt(q1)), np.abs(np.sqrt(p2) - np.sqrt(q2)) / np.abs(np.sqrt(q2)))
            worst = np.maximum(worst, np.where(np.isfinite(e), e, np.inf))
        return worst / kappa


def detuned(w, ne, bmag, c2):
    """w with every row whose ulp_sensitivity exceeds SENS_MAX moved up by 7 % at a time until it does not: the states sit off the
    resonances by construction (a condition on the inputs, computed with numpy's own Stix parameters, nothing of a device)."""
    w = w.copy()
    for _ in range(40):
        bad = ~(ulp_sensitivity(w, ne, bmag, c2) <= SENS_MAX)
        if not bad.any():
            break
        w[bad] *= 1.07
    return w


def tuples(family, n=N_TUPLES):
    """[n, 5] = n2, phi (degrees), S, D, P of physical plasmas: N_e 1e6 ... 1e12, |B| of the dipole at 1.1 ... 5.5 R_E,
    phi exactly 0 and 90 degrees, 1e-9 ... 1e-3 rad from either, and uniform between."""
    rng = np.random.default_rng(_seed("rh", family))
    ne = 10.0 ** rng.uniform(6.0, 12.0, n)
    bmag = 0.312e-4 / rng.uniform(1.1, 5.5, n) ** 3 * np.sqrt(1.0 + 3.0 * rng.uniform(0.0, 1.0, n) ** 2)
    lo, hi = {"vlf": (300.0, 30.0e3), "hf": (1.0e6, F_MAX), "mixed": (F_MIN, F_MAX), "hf_off": (1.0e6, F_MAX)}[family]
    top = np.minimum(hi, F_CAP_FPE * fpe(ne))
    f = np.exp(rng.uniform(np.log(np.minimum(lo, top / 3.0)), np.log(top)))
    kind = rng.choice(5, n, p=[0.1, 0.1, 0.15, 0.15, 0.5])
    small = 10.0 ** rng.uniform(-9.0, -3.0, n)
    ang = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [0.0, 0.5 * np.pi, small, 0.5 * np.pi - small],
                    rng.uniform(0.0, 0.5 * np.pi, n))
    c2 = np.where(kind == 1, 0.0, np.cos(ang) ** 2)
    phi = np.arccos(np.sqrt(c2)) * (180.0 / np.pi)          # as solve_dispersion_relation hands it over
    S, D, P, R, L = stix(2.0 * np.pi * f, ne, bmag)
    q1, q2, _, _, _ = nsq_roots(S, D, P, R, L, c2)
    n2 = np.where(rng.uniform(size=n) < 0.75, q1.real, q2.real)
    if family == "hf_off":
        n2 = n2 * 10.0 ** rng.uniform(-1.0, 1.0, n) * rng.choice([1.0, 1.0, 1.0, -1.0], n)
    return np.stack([n2, phi, S, D, P], axis=1)


def state_metrics(rows, disp, b):
    """For states rows[n, 7] with the reference's --mode=disp output disp[n, 10] and the model's B0 b[n, 3]: dict of
    cos2 (fp64, the reference's association), kappa, gap (of the tuple solve_dispersion_relation hands to is_right_handed; 1
    where it does not ask), sep (relative separation of the two roots) and `comparable`."""
    c2 = cos2phi(rows[:, 3:6], b)
    S, D, P, R, L = (disp[:, i] for i in range(1, 6))
    q1, _, A, B, disc = nsq_roots(S, D, P, R, L, np.minimum(c2, 1.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        kappa = np.maximum(1.0, np.abs(B) / np.sqrt(np.abs(disc)))
        n1 = np.sqrt(q1)
    asks = n1.real > 0
    phi = np.arccos(np.sqrt(np.minimum(c2, 1.0))) * (180.0 / np.pi)
    gap = np.where(asks, rh_gap(np.stack([q1.real, phi, S, D, P], axis=1)), 1.0)
    k1, k2 = disp[:, 6] + 1j * np.abs(disp[:, 7]), disp[:, 8] + 1j * np.abs(disp[:, 9])
    with np.errstate(invalid="ignore"):
        sep = np.abs(k1 - k2) / np.maximum(np.abs(k1), np.abs(k2))
        comparable = (gap >= GAP_MIN) & (sep > ROOT_SEP_MIN) & (kappa <= KAPPA_MAX)
    return {"cos2": c2, "kappa": kappa, "gap": gap, "sep": sep, "comparable": comparable, "asks": asks}


def root_errors(g, ref):
    """|Re| and ||Im|| differences of root columns g[n, 2] against ref[n, 2], relative to the reference root's magnitude."""
    mag = np.maximum(np.hypot(ref[:, 0], ref[:, 1]), 1e-300)
    return np.maximum(np.abs(g[:, 0] - ref[:, 0]), np.abs(np.abs(g[:, 1]) - np.abs(ref[:, 1]))) / mag


def ordered_errors(g, ref):
    """Per row: max over k1-vs-k1 and k2-vs-k2 (columns 6..9 of a disp output)."""
    return np.maximum(root_errors(g[:, 6:8], ref[:, 6:8]), root_errors(g[:, 8:10], ref[:, 8:10]))


def unordered_errors(g, ref):
    """Per row: the better of the two pairings."""
    sw = np.concatenate([g[:, :6], g[:, 8:10], g[:, 6:8]], axis=1)
    return np.minimum(ordered_errors(g, ref), ordered_errors(sw, ref))


def judged(g, key, family):
    """The reference's --mode=disp rows of one family from the golden file `g`, with the rows it stopped on replaced by its rows
    for the tilted direction: what the comparable set and kappa are computed from.  Returns (rows_in, disp, stopped, judge)."""
    rows, out, st = (g["%s_%s_%s" % (key, family, k)] for k in ("in", "disp", "stopped"))
    judge = out.copy()
    if st.any():
        judge[st] = g["%s_%s_tilted" % (key, family)][st]
    return rows, out, st, judge


def on_surface(rows, judge, comparable):
    """States on the dispersion surface for the gradient tests: the comparable rows of a family on which a root propagates, k put
    on that root (k2 where it propagates, else k1) along the row's own direction.  Returns [m, 7]."""
    kh = rows[:, 3:6] / np.linalg.norm(rows[:, 3:6], axis=1, keepdims=True)
    kr = np.where(judge[:, 8] > 0, judge[:, 8], judge[:, 6])
    ok = comparable & (kr > 0) & (judge[:, 7] == 0) & (judge[:, 9] == 0)
    return np.concatenate([rows[ok, 0:3], kh[ok] * kr[ok, None], rows[ok, 6:7]], axis=1)
