"""GPU (-m gpu): the interp lookup's reordering (exp per species inside the species loop, offset cell searches behind the
re-stage, exp of straddling points in the out-of-line direct evaluation) changes no output bit.  nspec 2, 3 and 4 on a coarse
grid with del_ = 1e-3, so that stencil points leave the centre's cell in a few per cent of the lookups; loose adaptive traces
whose free point changes cell; fixed-step traces; srt_rk_step / srt_gradients on those states: the digests recorded by
tests/golden/make_lookup_overlap_golden.py with the library from before the change."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

pytestmark = pytest.mark.gpu


def test_outputs_bit_identical_to_pre_change_golden():
    from make_lookup_overlap_golden import compute

    ref = np.load(os.path.join(HERE, "golden", "lookup_overlap_golden.npz"))
    report = {}
    got = compute(report)
    print("straddle shares:", report)
    assert sorted(got) == sorted(ref.files)
    assert min(report.values()) >= 0.01, "the cases no longer exercise the straddle path: %s" % report
    bad = []
    for k, v in got.items():
        r = ref[k]
        if isinstance(v, str):
            if v != str(r):
                bad.append(k)
        elif not np.array_equal(np.asarray(v), r):
            bad.append("%s: %s != %s" % (k, v, r))
    assert not bad, "differs from the pre-change library: %s" % bad
    for k in got:
        if k.endswith("_absent_species_absmax"):
            assert float(got[k][0]) == 0.0, k
