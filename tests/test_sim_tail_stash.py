"""CPU: tools/sim_tail_stash.py on a small fixture of real row counts (tests/golden/tail_stash_nrows4096.npy: every 244th ray of
the headline launch set in the library's launch-cell order, maxsteps 256).  Whatever the candidate, every ray finishes exactly
once and every banked ray is resumed; and the tool's restatement of the marks is the header's (srt_tail_stash.hpp)."""
import os
import re
import sys

import numpy as np
import pytest

from conftest import GOLDEN_DIR, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import sim_tail_stash as sim  # noqa: E402


@pytest.fixture(scope="module")
def nrows():
    a = np.load(os.path.join(GOLDEN_DIR, "tail_stash_nrows4096.npy")).astype(np.int64)
    assert a.shape == (4096,) and a.min() >= 1 and a.max() == 256
    return a


@pytest.mark.parametrize("waves", [1, 4, 16])
@pytest.mark.parametrize("name,kw", sim.CANDIDATES)
def test_every_ray_finishes_exactly_once(nrows, waves, name, kw):
    r = sim.simulate(nrows, waves, 256, **kw)
    assert np.array_equal(r["finished"], np.ones(len(nrows), dtype=np.int64)), name
    assert r["resumed"] == sum(r["banked"])
    assert (sum(r["banked"]) > 0) == (kw.get("quotas", 0) != 0)
    # the work is the rays' steps, whatever the schedule
    assert round(r["occupancy"] * r["trips"] * waves * 64) == int(np.sum(nrows - 1))
    assert r["trips"] >= int(np.ceil(np.sum(nrows) / (waves * 64.0)))


def test_no_banking_where_it_cannot_help(nrows):
    few = nrows[:256]
    assert sum(sim.simulate(few, 4, 256, quotas=32)["banked"]) == 0  # no more rays than lanes
    short = np.minimum(nrows, 31)
    assert sum(sim.simulate(short, 4, 31, quotas=32)["banked"]) == 0  # maxsteps below the minimum
    assert sum(sim.simulate(np.minimum(nrows, 32), 4, 32, quotas=32)["banked"]) > 0


def test_the_tool_restates_the_header():
    text = open(os.path.join(ROOT, "stanford_raytracer_amd", "csrc", "srt_tail_stash.hpp")).read()
    const = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))
    assert const("STASH_LEVELS") == sim.LEVELS and const("STASH_MIN_MAXSTEPS") == sim.MIN_MAXSTEPS
    assert "sp.mark[k] = maxsteps - (maxsteps >> (k + 1));" in text
    for maxsteps in (32, 64, 100, 256):
        marks, quota = sim.policy(maxsteps, 1000, 128, const("STASH_QUOTA"))
        assert marks.tolist() == [maxsteps - (maxsteps >> (k + 1)) for k in range(4)]
        assert quota.tolist() == [const("STASH_QUOTA")] * 4
