#!/usr/bin/env python3
"""What the trace kernels' tail stash (csrc/srt_tail_stash.hpp, HISTORY.md section 29) does to the length of a launch, simulated
from the row counts of a real launch set.

    python bench.py --gpus 1 --steps 1 --warmup 0 --dump-outputs DIR          # on an MI355X: DIR/nrows.npy, DIR/rays.npy
    python tools/sim_tail_stash.py DIR/nrows.npy [--rays-npy DIR/rays.npy] [--seed 3] > profiles/tail_stash/sim_table.txt

The model.  W waves of 64 lanes run in lock step, one loop trip per tick (on the device the waves drift apart; a trip costs
about the same however many lanes are busy).  A ray with n rows takes one trip to be launched and n - 1 trips for its steps:
rejected attempts are not in the row counts: --reject draws them per lane and trip (the headline rejects 4.0 % of its attempts;
without them every wave of the model stays in step with every other for the whole launch, because 55 % of the rays have the
same length).  A tick is
the kernel's loop top in its order: stop tests, bank, refill from the queue (waves claim in wave order, a wave sees the queue
empty when its own claim reaches the end), resume, one trip.  The bank and pick rules are those of srt_tail_stash.hpp, restated
here; tests/test_sim_tail_stash.py holds the two against each other on the marks and checks that every ray finishes once.

Order of the rays: with --seed the launch set is regenerated (workloads.launch_set) and sorted the way the library's
ray_order = 1 does it -- the Morton code of the launch cell on the 256^3 grid over +-10 R_E, cell index = nodes <= the
coordinate, stable -- else the order of the file is used, and the table says which.

Ratios of rays per lane other than the set's own: every k-th ray of the ordered set (sub-sampling), or the set repeated.
"""
import argparse
import sys

import numpy as np

WAVE = 64
LEVELS = 4
MIN_MAXSTEPS = 32


def policy(maxsteps, nrays, lanes, quotas, nmarks=LEVELS):
    """marks and quotas of a launch (stash_policy): quotas = one number or one per level"""
    q = [quotas] * LEVELS if np.isscalar(quotas) else list(quotas)
    on = maxsteps >= MIN_MAXSTEPS and nrays > lanes
    marks = [maxsteps - (maxsteps >> (k + 1)) for k in range(LEVELS)]
    return np.array(marks), np.array([q[k] if (on and k < nmarks) else 0 for k in range(LEVELS)])


def simulate(nrows, waves, maxsteps, quotas=0, nmarks=LEVELS, fit=True, wave_cap=WAVE, reject=0.0, seed=1):
    """nrows[n] in queue order -> dict(trips: ticks of the launch, wave_trips: trips summed over the waves, occupancy: busy
    lane-trips over ticks x lanes, lane_occupancy: over 64 x wave_trips (what bench.py reports: attempts over the lanes of the
    trips the waves ran), banked[4], resumed, tail_trips, finished[n]: how often each ray stopped).  reject: the share of
    attempts that are rejected, drawn per lane and trip (seeded)."""
    rng = np.random.default_rng(seed)
    nrows = np.asarray(nrows, dtype=np.int64)
    n = len(nrows)
    marks, quota = policy(maxsteps, n, waves * wave_cap, quotas, nmarks)
    Q = max(int(quota.max()), 1)
    rem = maxsteps - marks
    lane_ray = np.full((waves, WAVE), -1, dtype=np.int64)
    nstep = np.zeros((waves, WAVE), dtype=np.int64)
    active = np.zeros((waves, WAVE), dtype=bool)
    needinit = np.zeros((waves, WAVE), dtype=bool)
    seen_empty = np.zeros(waves, dtype=bool)
    fill = np.zeros((waves, LEVELS), dtype=np.int64)
    st_ray = np.full((waves, LEVELS, Q), -1, dtype=np.int64)
    st_step = np.zeros((waves, LEVELS, Q), dtype=np.int64)
    tail = np.zeros(waves, dtype=np.int64)
    finished = np.zeros(n, dtype=np.int64)
    banked = np.zeros(LEVELS, dtype=np.int64)
    resumed = head = ticks = wave_trips = work = 0
    wi = np.arange(waves)[:, None]
    while True:
        # A. stop tests
        stop = active & (nstep >= nrows[np.maximum(lane_ray, 0)])
        np.add.at(finished, lane_ray[stop], 1)
        active &= ~stop
        # bank
        if quota.any():
            for k in range(LEVELS):
                want = active & (nstep == marks[k]) & ~seen_empty[:, None]
                if not want.any():
                    continue
                rank = np.cumsum(want, axis=1) - 1
                take = want & (rank < (quota[k] - fill[:, k])[:, None])
                w, l = np.nonzero(take)
                slot = fill[w, k] + rank[w, l]
                st_ray[w, k, slot] = lane_ray[w, l]
                st_step[w, k, slot] = nstep[w, l]
                active[w, l] = False
                cnt = take.sum(axis=1)
                fill[:, k] += cnt
                banked[k] += cnt.sum()
        # B. refill from the queue
        free = ~active
        nfree = free.sum(axis=1)
        room = wave_cap - (WAVE - nfree)
        take = np.where(seen_empty, 0, np.clip(np.minimum(nfree, room), 0, None))
        base = head + np.cumsum(take) - take
        head += int(take.sum())
        rank = np.cumsum(free, axis=1) - 1
        ids = base[:, None] + rank
        claim = free & (rank < take[:, None]) & (ids < n)
        lane_ray[claim] = ids[claim]
        needinit |= claim
        seen_empty |= (take > 0) & (base + take >= n)
        # resume
        if quota.any():
            idle = ~active & ~needinit
            nidle = idle.sum(axis=1)
            room = wave_cap - (WAVE - nidle)
            take2 = np.where(seen_empty & (fill.sum(axis=1) > 0), np.clip(np.minimum(nidle, room), 0, None), 0)
            if take2.any():
                rank = np.cumsum(idle, axis=1) - 1
                given = np.zeros(waves, dtype=np.int64)
                for _ in range(LEVELS):
                    # stash_pick for every wave
                    budget = maxsteps - tail
                    has = fill > 0
                    fits = has & (rem[None, :] <= budget[:, None]) if fit else has
                    k = np.where(fits.any(axis=1), np.argmax(fits, axis=1), LEVELS - 1 - np.argmax(has[:, ::-1], axis=1))
                    have = np.where(has.any(axis=1), fill[np.arange(waves), k], 0)
                    m = np.minimum(have, take2 - given)
                    if not m.any():
                        break
                    sel = idle & (rank >= given[:, None]) & (rank < (given + m)[:, None])
                    w, l = np.nonzero(sel)
                    slot = have[w] - 1 - (rank[w, l] - given[w])
                    lane_ray[w, l] = st_ray[w, k[w], slot]
                    nstep[w, l] = st_step[w, k[w], slot]
                    active[w, l] = True
                    fill[np.arange(waves), k] -= m
                    given += m
                    resumed += int(m.sum())
        # D. exit
        busy = active | needinit
        if not busy.any():
            # (a wave with every lane free has claimed above, found the queue empty and taken what its stash held)
            if head < n or fill.any() or not seen_empty.all():
                raise RuntimeError("the simulation stalls: queue at %d of %d, %d records in the stash" % (head, n, fill.sum()))
            break
        # E. one trip
        run = busy.any(axis=1)
        ticks += 1
        wave_trips += int(run.sum())
        work += int(active.sum())
        tail += seen_empty & run
        if reject > 0.0:
            nstep[active & (rng.random(active.shape) >= reject)] += 1
        else:
            nstep[active] += 1
        nstep[needinit] = 1
        active |= needinit
        needinit[:] = False
    return dict(trips=ticks, wave_trips=wave_trips, occupancy=work / max(ticks * waves * WAVE, 1),
                lane_occupancy=work / max(wave_trips * WAVE, 1), banked=banked.tolist(),
                resumed=resumed, tail_trips=int(tail.sum()), finished=finished)


def library_order(seed, n, grid=256, half_width_re=10.0):
    """queue position -> ray id as srt_params.ray_order = 1 sorts the seeded launch set"""
    import os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    from stanford_raytracer_amd import workloads as wl

    pos = wl.launch_set(n, seed)[0]
    hw = half_width_re * wl.R_E
    c = np.clip(np.floor((pos + hw) / (2.0 * hw) * (grid - 1)).astype(np.int64) + 1, 0, grid)

    def spread(v):
        v = v & 0x3FF
        v = (v | (v << 16)) & 0x030000FF
        v = (v | (v << 8)) & 0x0300F00F
        v = (v | (v << 4)) & 0x030C30C3
        v = (v | (v << 2)) & 0x09249249
        return v

    return np.argsort(spread(c[:, 0]) | (spread(c[:, 1]) << 1) | (spread(c[:, 2]) << 2), kind="stable")


CANDIDATES = [("no stash", dict(quotas=0)),
              ("1/2 x 32", dict(quotas=32, nmarks=1)),
              ("1/2 3/4 7/8 x 32", dict(quotas=32, nmarks=3)),
              ("4 marks x 16", dict(quotas=16)),
              ("4 marks x 32", dict(quotas=32)),
              ("4 marks x 48", dict(quotas=48)),
              ("4 marks x 32, no fit rule", dict(quotas=32, fit=False))]
RATIOS = [1.5, 2.5, 4.0, 7.6, 15.3, 61.0]


def resample(nrows, ratio, lanes):
    """the ordered set at `ratio` rays per lane: every k-th ray, or the set repeated"""
    want = int(round(ratio * lanes))
    if want <= len(nrows):
        return nrows[np.linspace(0, len(nrows) - 1, want).astype(np.int64)]
    return np.tile(nrows, (want + len(nrows) - 1) // len(nrows))[:want]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("nrows")
    ap.add_argument("--rays-npy", default=None, help="ray ids the row counts belong to (bench.py --dump-outputs: rays.npy)")
    ap.add_argument("--seed", type=int, default=None, help="regenerate the launch set with this seed and use the library's Morton order")
    ap.add_argument("--waves", type=int, default=1024, help="waves of the launch (MI355X: 256 CUs x 4)")
    ap.add_argument("--maxsteps", type=int, default=256)
    ap.add_argument("--ratios", type=float, nargs="*", default=RATIOS)
    ap.add_argument("--reject", type=float, default=0.0402, help="share of attempts rejected (0 = the row counts alone)")
    a = ap.parse_args()
    nrows = np.load(a.nrows).astype(np.int64).ravel()
    if a.rays_npy:
        ids = np.load(a.rays_npy).astype(np.int64).ravel()
        full = np.zeros(ids.max() + 1, dtype=np.int64)
        full[ids] = nrows
        nrows = full
    order = "the file's order"
    if a.seed is not None:
        nrows = nrows[library_order(a.seed, len(nrows))]
        order = "launch-cell Morton order of launch_set(%d, %d), as ray_order = 1 sorts it" % (len(nrows), a.seed)
    lanes = a.waves * WAVE
    print("# %d rays, mean %.1f rows, %.1f %% at maxsteps %d; %d waves; order: %s" % (
        len(nrows), nrows.mean(), 100.0 * np.mean(nrows >= a.maxsteps), a.maxsteps, a.waves, order))
    print("# %.4f of the attempts rejected; trips = ticks of the launch; trips/wave = mean over the waves; lane occ. = busy lanes of the trips run" % a.reject)
    print("# rays/lane  candidate                     trips  vs none  trips/wave  vs none  lane occ.  banked per mark")
    for ratio in a.ratios:
        rows = resample(nrows, ratio, lanes)
        base = None
        for name, kw in CANDIDATES:
            r = simulate(rows, a.waves, a.maxsteps, reject=a.reject, **kw)
            assert np.all(r["finished"] == 1) and r["resumed"] == sum(r["banked"])
            base = (r["trips"], r["wave_trips"]) if base is None else base
            print("%9.2f    %-28s %6d  %+6.2f %%  %9.1f  %+6.2f %%  %.4f     %s" % (
                len(rows) / lanes, name, r["trips"], 100.0 * (r["trips"] - base[0]) / base[0], r["wave_trips"] / a.waves,
                100.0 * (r["wave_trips"] - base[1]) / base[1], r["lane_occupancy"], r["banked"]))
            sys.stdout.flush()


if __name__ == "__main__":
    main()
