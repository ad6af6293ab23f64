"""GPU (-m gpu): the interp model's ring residency changes no output bit.  Coarse grid, refills, nspec 4 and 1, adaptive and
fixed-step traces, and srt_rk_step / srt_gradients states whose stages change cell: the digests recorded by
tests/golden/make_ring_residency_golden.py with the library from before the change."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

pytestmark = pytest.mark.gpu


def test_outputs_bit_identical_to_pre_residency_golden():
    from make_ring_residency_golden import compute

    ref = np.load(os.path.join(HERE, "golden", "ring_residency_golden.npz"))
    got = compute()
    assert sorted(got) == sorted(ref.files)
    bad = []
    for k, v in got.items():
        r = ref[k]
        if isinstance(v, str):
            if v != str(r):
                bad.append(k)
        elif not np.array_equal(np.asarray(v), r):
            bad.append("%s: %s != %s" % (k, v, r))
    assert not bad, "differs from the pre-change library: %s" % bad
