"""What the G1 rung (Stix parameters, F, roots of srt_dispersion) is measured with: shared by tests/test_gpu_parity.py (models the
golden vectors cover) and the test files of modelnum 5 and 6 (models the oracle does not have).  Not a test module."""
import numpy as np


def rel(a, b):
    return np.abs(a - b) / np.maximum(np.abs(b), 1e-300)


def f_scale(rows, out, c):
    n2 = (np.linalg.norm(rows[:, 3:6], axis=1) * c / rows[:, 6]) ** 2
    S, D, P, R, L = (out[:, i] for i in range(1, 6))
    return (np.abs(S) + np.abs(P)) * n2 ** 2 + (np.abs(R * L) + np.abs(P * S)) * 2 * n2 + np.abs(R * L * P)


def check_dispersion_against_own_params(model, states):
    """srt_dispersion on a handle of a model the oracle does not have (modelnum 5, 6; called from their test files): at most the
    first 65 states [x, k, w] (one full wave and one lane of a second; the golden files of both models hold 24, part of one
    wave), F and the Stix parameters against the oracle's POINTWISE
    so_dispersion_relation / so_stix_parameters fed with the same handle's plasma_params, at the bars of
    test_g1_dispersion_vs_golden; the four root columns finite, and those of the first state the same bits in the batch and
    alone (solve_dispersion is per lane and sees the same inputs in both calls)."""
    import ctypes as C

    from oracle import oracle

    st = np.ascontiguousarray(states[:65])
    assert len(st) >= 1
    x, k, w = st[:, 0:3], st[:, 3:6], st[:, 6]
    g, pp = model.dispersion(x, k, w), model.plasma_params(x)
    so, ref = oracle.lib(), np.zeros((len(st), 6))
    c = so.so_speed_of_light()
    for i in range(len(st)):
        qs, Ns, ms, B0 = (np.ascontiguousarray(pp[i, a:b]) for a, b in ((0, 4), (4, 8), (8, 12), (16, 19)))
        n = np.ascontiguousarray(k[i] * c / w[i])
        ref[i, 0] = so.so_dispersion_relation(oracle._dp(n), float(w[i]), model.nspec, oracle._dp(qs), oracle._dp(Ns), oracle._dp(ms),
                                              oracle._dp(B0))
        o = [C.c_double() for _ in range(5)]
        b0mag = float(np.sqrt((B0[0] * B0[0] + B0[1] * B0[1]) + B0[2] * B0[2]))  # sqrt(dot_product(B0,B0)), the Fortran's association
        so.so_stix_parameters(float(w[i]), model.nspec, oracle._dp(qs), oracle._dp(Ns), oracle._dp(ms), b0mag, *[C.byref(v) for v in o])
        ref[i, 1:6] = [v.value for v in o]
    e_stix, e_f = rel(g[:, 1:6], ref[:, 1:6]).max(), np.max(np.abs(g[:, 0] - ref[:, 0]) / f_scale(st, ref, c))
    print("G1 from the handle's own parameters: %d states, S D P R L error max %.3g, F error max %.3g of its scale" % (len(st), e_stix, e_f))
    assert e_stix <= 1e-10
    assert e_f <= 1e-10
    assert np.all(np.isfinite(g[:, 6:10]))
    alone = model.dispersion(x[:1], k[:1], w[:1])
    assert alone[0, 6:10].tobytes() == g[0, 6:10].tobytes()
