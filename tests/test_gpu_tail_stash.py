"""GPU (-m gpu): the tail stash of the unsegmented interp kernels (srt_tail_stash.hpp, include/srt.h srt_launch_stash_stats).

Every launch is held against digests recorded by tests/golden/make_tail_stash_golden.py with the library of the commit before
the stash (rows as bytes, nrows, stop codes, accepted steps, attempts), and against the launch's own statistics: every mark
has banked at least one ray and every banked ray was resumed.  So no case passes without having used the stash.  600 rays on
two waves (SRT_MAX_BLOCKS=2): 4.7 rays per lane."""
import json
import os

import numpy as np
import pytest
import torch  # before the library's first call

import tail_stash_cases as tc
from conftest import GOLDEN_DIR
from stanford_raytracer_amd import api

pytestmark = pytest.mark.gpu
if torch.cuda.is_available():
    torch.cuda.init()

GRID_CAP = {"SRT_MAX_BLOCKS": "2"}


@pytest.fixture(scope="module")
def gold():
    return json.load(open(os.path.join(GOLDEN_DIR, "tail_stash_golden.json")))["cases"]


@pytest.fixture(scope="module")
def rays():
    api.init(0)
    return tc.rays()


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(kind):
        if kind not in cache:
            cache[kind] = tc.make_model(kind)
        return cache[kind]

    return get


def run(model, rays, extra, env):
    with tc.Env(**env):
        r = tc.launch(model, api.make_params(**dict(tc.TRACE, **extra)), *rays)
        return r, model.stash_stats()


def assert_digests(r, want, what):
    got = tc.digests(*r)
    for k in ("nrows", "stop", "accepted", "attempts", "rows"):
        assert got[k] == want[k], "%s: %s differs from the library without the stash" % (what, k)


@pytest.mark.parametrize("name", list(tc.CASES))
def test_banked_rays_come_back_bit_equal(models, rays, gold, name):
    kind, extra, env = tc.CASES[name]
    r, st = run(models(kind), rays, extra, dict(GRID_CAP, **env))
    print(name, st, "trips", int(r[3][3]))
    assert_digests(r, gold[name], name)
    assert all(b >= 1 for b in st["banked"]), st
    assert st["resumed"] == sum(st["banked"]), st
    assert 1 <= st["max_fill"] <= 4 * 32 and st["tail_trips"] >= 1, st
    # the launch set's own mix, as recorded: several stop codes, and rays that stop on a mark
    assert len(gold[name]["stop_codes"]) >= 3, gold[name]["stop_codes"]


def test_switched_off(models, rays, gold):
    r, st = run(models("interp4"), rays, {}, dict(GRID_CAP, **tc.SAME_AS_ADAPTIVE["off"]))
    assert_digests(r, gold["adaptive"], "SRT_TAIL_STASH=0")
    assert st == {"banked": [0, 0, 0, 0], "resumed": 0, "max_fill": 0, "tail_trips": 0}
    r_on, st_on = run(models("interp4"), rays, {}, GRID_CAP)
    # counters[3], the loop trips of all waves, is the one thing that moves
    print("trips without", int(r[3][3]), "with", int(r_on[3][3]), st_on)
    assert sum(st_on["banked"]) > 0


def test_queue_empty_at_the_first_claim_banks_nothing(models, rays, gold):
    """64 rays on one wave: no more rays than lanes"""
    first = tuple(a[:64] for a in rays)
    with tc.Env(SRT_MAX_BLOCKS="1"):
        r = tc.launch(models("interp4"), api.make_params(**tc.TRACE), *first)
        st = models("interp4").stash_stats()
    assert st == {"banked": [0, 0, 0, 0], "resumed": 0, "max_fill": 0, "tail_trips": 0}
    with tc.Env(SRT_TAIL_STASH="0"):
        r0 = tc.launch(models("interp4"), api.make_params(**tc.TRACE), *first)
    assert tc.digests(*r) == tc.digests(*r0)


def test_maxsteps_below_the_minimum_banks_nothing(models, rays):
    """maxsteps 31 < 32: the marks would be too close to each other"""
    r, st = run(models("interp4"), rays, dict(maxsteps=31), GRID_CAP)
    assert st == {"banked": [0, 0, 0, 0], "resumed": 0, "max_fill": 0, "tail_trips": 0}
    assert np.sum(r[2] == 6) > 100 and r[1].max() == 31  # (rays did run to maxsteps)
    r32, st32 = run(models("interp4"), rays, dict(maxsteps=32), GRID_CAP)
    assert sum(st32["banked"]) > 0 and st32["resumed"] == sum(st32["banked"]), st32


def test_quota_of_one_leaves_further_rays_running(models, rays, gold):
    """SRT_TAIL_STASH=1: each of the two waves banks one ray per mark; the other rays on that mark run on in their lanes"""
    r, st = run(models("interp4"), rays, {}, dict(GRID_CAP, **tc.SAME_AS_ADAPTIVE["quota1"]))
    assert_digests(r, gold["adaptive"], "SRT_TAIL_STASH=1")
    assert all(1 <= b <= 2 for b in st["banked"]), st
    assert st["resumed"] == sum(st["banked"]) and st["max_fill"] <= 4, st
    assert min(gold["adaptive"]["rays_reaching_mark"]) > 100  # (many more rays passed every mark than were banked)


def test_a_ray_that_stops_on_a_mark_is_not_banked(models, rays):
    """Fixed steps of dt0 and tmax = 30.5 dt0: a ray that survives that long has t = 31 dt0 >= tmax when its step count is 32,
    the first mark, and stops there with code 0 -- the stop tests come first, so the stash, which is on (the waves count their
    trips after the queue ran empty), banks nothing."""
    dt0 = tc.TRACE["dt0"]
    r, st = run(models("interp4"), rays, dict(fixedstep=1, tmax=30.5 * dt0), GRID_CAP)
    nrows, stop = r[1], r[2]
    assert nrows.max() == tc.MARKS[0] and np.sum((nrows == tc.MARKS[0]) & (stop == 0)) > 100
    assert st["banked"] == [0, 0, 0, 0] and st["resumed"] == 0 and st["max_fill"] == 0, st
    assert st["tail_trips"] >= 1, st
    with tc.Env(SRT_TAIL_STASH="0", **GRID_CAP):
        r0 = tc.launch(models("interp4"), api.make_params(**dict(tc.TRACE, fixedstep=1, tmax=30.5 * dt0)), *rays)
    assert tc.digests(*r) == tc.digests(*r0)
