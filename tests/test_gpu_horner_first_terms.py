"""GPU (-m gpu): the interp lookup assigns the first term of each Horner sum instead of adding it to a 0.0 (plane_stencil: the
j = 3 row of every plane, the k = 3 plane of every species).  fma(+0.0, y, v) differs from v only for v = -0.0, and a zero of
either sign is absorbed by the next non-zero term or ends in exp(+-0) = 1, so no output bit moves -- checked where zeros travel
furthest: a flat ln N = 0.0 grid, grids holding -0.0, a grid with planes of zeros, centres exactly on nodes (local coordinates 0),
centres in the clamped cells, straddling stencils, nspec 4 and 2; srt_plasma_params, srt_gradients, srt_rk_step and short RKF45 /
RK4 traces.  Against the digests recorded by tests/golden/make_horner_first_terms_golden.py with the library from before the
change."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

pytestmark = pytest.mark.gpu


def test_outputs_bit_identical_to_pre_change_golden():
    from make_horner_first_terms_golden import compute, low_coverage

    ref = np.load(os.path.join(HERE, "golden", "horner_first_terms_golden.npz"))
    report = {}
    got = compute(report)
    print("coverage of the states:", report)
    assert sorted(got) == sorted(ref.files)
    assert not low_coverage(report), "the states no longer reach nodes, clamped cells or straddling stencils: %s" % low_coverage(report)
    bad = []
    for k, v in got.items():
        r = ref[k]
        if isinstance(v, str):
            if v != str(r):
                bad.append(k)
        elif not np.array_equal(np.asarray(v), r, equal_nan=True):
            bad.append("%s: %s != %s" % (k, v, r))
    assert not bad, "differs from the pre-change library: %s" % bad
