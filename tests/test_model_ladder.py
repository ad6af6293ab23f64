"""The shared parity ladder (tests/model_ladder.py) held against the committed goldens alone, without a GPU: a stub model that
answers with the reference's own arrays passes every rung G0 .. G4 with the arguments the GPU test files of modelnum 6, 5 and 7
pass; the same stub with one sample moved to 1.01 x its bar fails that rung with an AssertionError, and with the sample at
0.99 x its bar passes it.  A sample's bar is max(the rung's fixed bar, 10 x that sample's recorded sensitivity), worked out here
from the golden, not taken from the ladder: the figures below are the ladder's bars written a second time on purpose.
(The builders' checks compare a handle with itself and have nothing to be held against here.)"""
import os

import numpy as np
import pytest

import model_ladder as ladder
from conftest import GOLDEN_DIR, vrel

# per golden: what its GPU test file passes to the ladder
GOLDENS = {
    "simple3d": dict(tags="abcd", g23="ab", state="g23_state_%s", floor=1e-11, per_species=False, min_steady=56,
                     adaptive=dict(min_curves=48, same_t=ladder.same_t_first_rows)),
    "ngo3d": dict(tags="abcd", g23="abe", state="g23_state_%s", floor=1e-11, per_species=False, min_steady=56,
                  adaptive=dict(min_curves=48, same_t=ladder.same_t_first_rows)),
    "at64thch": dict(tags="abcd", g23="abd", state="g23_state", floor=1e-6, per_species=True, min_steady=14,
                     adaptive=dict(min_curves=15, yard_curves=15, same_t=ladder.same_t_all_rows)),
}
# G2: columns of srt_gradients' output and their fixed bar (dk/dt: that of its maximum); G3: offsets within one of the three
# outputs and (median bar, maximum bar)
G2_COLUMNS = {"dFdk": (slice(0, 3), 1e-7), "dFdw": (slice(3, 4), 1e-6), "dFdx": (slice(4, 7), 1e-7), "dx/dt": (slice(7, 10), 1e-6),
              "dk/dt max": (slice(10, 13), 2e-5)}
DKDT_MEDIAN = 1e-6
G3_PARTS = {"position": (0, 1e-8, 1e-7), "k": (3, 1e-7, 1e-2)}


@pytest.fixture(scope="module", params=list(GOLDENS))
def case(request):
    return np.load(os.path.join(GOLDEN_DIR, request.param + "_golden.npz")), GOLDENS[request.param]


class Stub:
    """A model that answers with the golden's reference arrays of setting `tag` (copies: a test moves a sample in them).  Its
    fixed-step trace is the reference's run; its adaptive one the reference's run from the launch points shifted by 1e-9 -- the
    ladder's own yardstick, so it is held at ratio 1 -- with row 0 at the launch points it was asked for."""

    def __init__(self, gold, cfg, tag):
        if tag in cfg["tags"]:
            self.Ns, self.B0 = gold["g0_Ns_" + tag].copy(), gold["g0_B0_" + tag]
        if tag in cfg["g23"]:
            self.g2, self.g3 = gold["g2_" + tag].copy(), gold["g3_" + tag].copy()
        self.runs = {}
        for mode, key in (("fixed", "run_fixed"), ("adaptive", "run_adaptive_shift")):
            self.runs[mode] = [ladder.widen(gold[key + "_rows"]), gold[key + "_nrows"], gold[key + "_stop"]]
        self.runs["adaptive"][0][:, 0, 1:4] = gold["run_adaptive_rows"][:, 0, 1:4]

    def plasma_params(self, x):
        g = np.zeros((len(x), 19))
        g[:, 4:4 + self.Ns.shape[1]], g[:, 16:19] = self.Ns, self.B0
        return g

    def gradients(self, x, k, w, del_):
        return self.g2

    def rk_step(self, args, dt, del_):
        return self.g3

    def trace(self, pos0, dir0, w0, params):
        rows, nrows, stop = self.runs["fixed" if params.fixedstep else "adaptive"]
        return rows, nrows, stop, int(nrows.sum())


def g0(m, gold, cfg, tag):
    n = m.Ns.shape[1]
    ladder.check_g0_density(m.plasma_params(gold["g0_x_" + tag])[:, 4:4 + n], gold, tag, floor=cfg["floor"], per_species=cfg["per_species"],
                            report=None if cfg["per_species"] else lambda err: None)


def g2(m, gold, cfg, tag):
    ladder.check_g2(m, gold[cfg["state"].replace("%s", tag)], gold["g2_" + tag], gold["g2_sens_" + tag], 1e-6, tag)


def g3(m, gold, cfg, tag):
    ladder.check_g3(m, gold[cfg["state"].replace("%s", tag)], gold["g3_" + tag], gold["g3_sens_" + tag], gold["g3_dt"], 1e-6, tag)


def g4_fixed(m, gold, cfg):
    ladder.check_g4_fixed(ladder.trace_golden_rays(gold, [(m, slice(None))], "fixed"), gold, min_steady=cfg["min_steady"])


def g4_adaptive(m, gold, cfg):
    ladder.check_g4_adaptive(ladder.trace_golden_rays(gold, [(m, slice(None))], "adaptive"), gold, **cfg["adaptive"])


def test_the_references_own_arrays_pass_every_rung(case):
    gold, cfg = case
    for tag in cfg["tags"]:
        g0(Stub(gold, cfg, tag), gold, cfg, tag)
    for tag in cfg["g23"]:
        g2(Stub(gold, cfg, tag), gold, cfg, tag)
        g3(Stub(gold, cfg, tag), gold, cfg, tag)
    g4_fixed(Stub(gold, cfg, "a"), gold, cfg)
    g4_adaptive(Stub(gold, cfg, "a"), gold, cfg)


def either_side(rung, perturbed, names):
    """rung(stub) with perturbed(factor) -> stub: fails at 1.01 x the bar with a message that names `names`, passes at 0.99 x"""
    with pytest.raises(AssertionError, match=names):
        rung(perturbed(1.01))
    rung(perturbed(0.99))


def quiet_and_loud(sens):
    """the sample the reference moves least (its bar is the fixed one) and the one it moves most"""
    return sorted({int(np.argmin(sens)), int(np.argmax(sens))})


def test_g0_density_one_point_either_side_of_its_bar(case):
    gold, cfg = case
    for tag in cfg["tags"]:
        sens = gold["g0_sens_" + tag]
        for flat in quiet_and_loud(sens.ravel()):
            # per species the sensitivity is [n, nspec]; otherwise [n], and any species of the point may carry the error
            i, s = np.unravel_index(flat, sens.shape) if cfg["per_species"] else (flat, 1)
            bar = max(cfg["floor"], 10.0 * sens.ravel()[flat])

            def perturbed(f):
                m = Stub(gold, cfg, tag)
                m.Ns[i, s] *= 1.0 + f * bar
                return m
            either_side(lambda m: g0(m, gold, cfg, tag), perturbed, "1 points over their bar")


def sens_of(sens, ref, cols):
    """a golden's absolute sensitivity of the columns `cols`, relative to the reference's value there"""
    return np.linalg.norm(sens[:, cols], axis=1) / np.linalg.norm(ref[:, cols], axis=1)


@pytest.mark.parametrize("column", list(G2_COLUMNS), ids=["dFdk", "dFdw", "dFdx", "dxdt", "dkdt"])
def test_g2_one_sample_either_side_of_its_bar(case, column):
    gold, cfg = case
    cols, fixed = G2_COLUMNS[column]
    for tag in cfg["g23"]:
        rel = sens_of(gold["g2_sens_" + tag], gold["g2_" + tag], cols)
        for i in quiet_and_loud(rel):
            bar = max(fixed, 10.0 * rel[i])

            def perturbed(f):
                m = Stub(gold, cfg, tag)
                m.g2[i, cols] *= 1.0 + f * bar
                return m
            either_side(lambda m: g2(m, gold, cfg, tag), perturbed, "%s: sample %d has error" % (column, i))


def test_g2_dkdt_median_either_side_of_its_bar(case):
    """every sample at 1.01 x its own median bar (and so far below its maximum bar): the median is over; at 0.99 x it is not"""
    gold, cfg = case
    cols = G2_COLUMNS["dk/dt max"][0]
    for tag in cfg["g23"]:
        bar = np.maximum(DKDT_MEDIAN, 10.0 * sens_of(gold["g2_sens_" + tag], gold["g2_" + tag], cols))

        def perturbed(f):
            m = Stub(gold, cfg, tag)
            m.g2[:, cols] *= 1.0 + f * bar[:, None]
            return m
        either_side(lambda m: g2(m, gold, cfg, tag), perturbed, "dk/dt median: .* median error / bar 1.01")


@pytest.mark.parametrize("part", list(G3_PARTS))
@pytest.mark.parametrize("out", [0, 1, 2])
def test_g3_one_sample_and_the_median_either_side_of_their_bars(case, out, part):
    gold, cfg = case
    off, median_bar, max_bar = G3_PARTS[part]
    cols = slice(7 * out + off, 7 * out + off + 3)
    for tag in cfg["g23"]:
        rel = sens_of(gold["g3_sens_" + tag], gold["g3_" + tag], cols)
        for i in quiet_and_loud(rel):
            bar = max(max_bar, 10.0 * rel[i])

            def one(f):
                m = Stub(gold, cfg, tag)
                m.g3[i, cols] *= 1.0 + f * bar
                return m
            either_side(lambda m: g3(m, gold, cfg, tag), one, "out %d: .*%s max: sample %d has error" % (out, part, i))
        bars = np.maximum(median_bar, 10.0 * rel)

        def every(f):
            m = Stub(gold, cfg, tag)
            m.g3[:, cols] *= 1.0 + f * bars[:, None]
            return m
        either_side(lambda m: g3(m, gold, cfg, tag), every, "out %d: %s median: .* median error / bar 1.01" % (out, part))


def test_g4_fixed_the_worst_ray_either_side_of_its_bar(case):
    """the steady ray the reference's own 1e-9 shift moves most, and the one it moves least: the last row's position at 1.01 x
    and 0.99 x 10 max(that movement, 1e-8)"""
    gold, cfg = case
    ref, rn, rs = gold["run_fixed_rows"], gold["run_fixed_nrows"], gold["run_fixed_stop"]
    steady = np.nonzero((rn == gold["run_fixed_shift_nrows"]) & (rs == gold["run_fixed_shift_stop"]) & (rn > 1))[0]
    own = np.array([vrel(gold["run_fixed_shift_rows"][i, :rn[i], 1:4], ref[i, :rn[i], 1:4]).max() for i in steady])
    for j in quiet_and_loud(own):
        i, bar = steady[j], 10.0 * max(own[j], 1e-8)

        def perturbed(f):
            m = Stub(gold, cfg, "a")
            m.runs["fixed"][0][i, rn[i] - 1, 1:4] *= 1.0 + f * bar
            return m
        either_side(lambda m: g4_fixed(m, gold, cfg), perturbed, "ray %d: error .* over its bar" % i)
