"""GPU (-m gpu): the interp lookup decides from the centre's cell whether its offset points and its free point share that cell
(Axis::in_cell) instead of searching for each, and divides by one reciprocal per axis.  No output bit moves where the existing
goldens do not look: centres exactly on grid nodes and one ulp either side on each axis, centres outside the grid on every face
(clamped cells, zeroed local coordinate), offsets that skip whole cells (del_ = 0.2), a free point cells away (maxerr = 0.3),
nspec 1 and 4; traces (RKF45, RK4) and srt_rk_step / srt_gradients.  Against the digests recorded by
tests/golden/make_cell_from_centre_golden.py with the library from before the change."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

pytestmark = pytest.mark.gpu


def test_outputs_bit_identical_to_pre_change_golden():
    from make_cell_from_centre_golden import compute, low_shares

    ref = np.load(os.path.join(HERE, "golden", "cell_from_centre_golden.npz"))
    report = {}
    got = compute(report)
    print("(straddle share, clamped share):", report)
    assert sorted(got) == sorted(ref.files)
    assert not low_shares(report), "the cases no longer exercise the straddle path or the clamped cells: %s" % low_shares(report)
    bad = []
    for k, v in got.items():
        r = ref[k]
        if isinstance(v, str):
            if v != str(r):
                bad.append(k)
        elif not np.array_equal(np.asarray(v), r, equal_nan=True):
            bad.append("%s: %s != %s" % (k, v, r))
    assert not bad, "differs from the pre-change library: %s" % bad
