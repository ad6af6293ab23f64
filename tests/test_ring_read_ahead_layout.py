"""The species loop of the interp lookup with its LDS reads issued a unit ahead (stanford_raytracer_amd/csrc/srt_models.hpp:
InterpModel::density_stencil, read_unit_issue / wait_lgkm / wait_vm), replayed on the host in the style of
test_ring_residency_layout.py, but with TIME in it: what is in flight, and what each wait retires.

The loop reads unit k + 1 into a second register set before it waits for unit k's reads, refills buffer k only after that
wait, and so has one unit fewer in flight when unit k + 1 is read than the plain schedule had: its vmcnt counts are
24 / 16 / 16 / 16, for the last species 24 / 16 / 8 / 0.  On the GPU a count that is one unit too loose passes nearly always (the
units' DMA has almost always landed when it is waited for), so the counts and the issue order are checked here, pessimistically:

  * an LDS-DMA instruction makes its 1 KiB of the ring UNDEFINED from the moment it is issued until a vmcnt wait retires it (the
    loads of a wave retire in issue order; vmcnt(N) leaves at most the N youngest instructions in flight; a unit is 8 of them);
  * an LDS read may fetch its data at any moment between its issue and the lgkmcnt wait that releases it (LDS reads return in
    order; lgkmcnt(N) leaves at most the N youngest in flight; a unit is 8 reads): the unit must be defined and right at both ends
    of that window, and no DMA into its buffer may be issued inside it;
  * a register set takes a new unit only when the plane evaluated from it has consumed the last one.

Every lane must then read its own (cell, species, plane) for nspec 1..4, in both species directions, with resident and with
re-staged rows.  The same replay with a count loosened by one unit, or a refill issued before the wait that releases the buffer's
reads, must fail: the emulation would have caught them.  (The kernel itself is tested on the GPU: test_gpu_ring_residency.py,
test_gpu_lookup_overlap.py, test_gpu_cell_from_centre.py.)"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ring_residency_model import (HOLDS_FIRST, HOLDS_LAST, INVALID, MAX_IMM, PAD, RES_END, RING, UNIT,  # noqa: E402
                                  WAVE, prepare, read_unit)

UNDEFINED = ("in flight",)

# the waits in front of the reads of units 0..3: (while another species follows, for the last species) -- as in the source
VMCNT = {0: (24, 24), 1: (16, 16), 2: (16, 8), 3: (16, 0)}


class Wave:
    """The ring, the wave's load queue (LDS-DMA instructions, oldest first), its LDS-read queue and the two register sets."""

    def __init__(self):
        self.lds = {}
        self.vm = []  # one entry per DMA instruction: [(address, value)]
        self.lgkm = []  # one entry per unit read: [set name, buffer, reads outstanding]
        self.regs = {"cf": None, "cg": None}  # None: free; else {"J", "at_issue", "released", "value"}

    def dma(self, nspec, a, t, imm, J, lanes=range(WAVE)):
        """Instruction t of a unit (test_ring_residency_layout.dma), in flight until retired."""
        assert all(r[1] != J for r in self.lgkm), "DMA into buffer %d while reads of it have not been released" % J
        stride = nspec * 512
        m0 = PAD + J * UNIT + t * 1024 - imm
        assert 0 <= imm <= MAX_IMM and m0 >= RES_END
        writes = []
        for L in lanes:
            dst, src = m0 + imm + 16 * L, a[t][L] + imm
            assert PAD <= dst and dst + 16 <= PAD + RING * UNIT
            self.lds[dst] = UNDEFINED
            writes.append((dst, (src // stride, src % stride)))
        self.vm.append(writes)

    def wait_vm(self, n):
        while len(self.vm) > n:
            for dst, val in self.vm.pop(0):
                self.lds[dst] = val

    def read_unit_issue(self, J, name):
        assert self.regs[name] is None, "register set %s is overwritten before its plane was evaluated" % name
        self.regs[name] = {"J": J, "at_issue": [read_unit(self.lds, J, lane) for lane in range(WAVE)], "released": False}
        self.lgkm.append([name, J, 8])

    def wait_lgkm(self, n):
        while sum(r[2] for r in self.lgkm) > n:
            name, J, _ = self.lgkm.pop(0)
            r = self.regs[name]
            r["value"] = [read_unit(self.lds, J, lane) for lane in range(WAVE)]
            r["released"] = True

    def plane(self, name, want, what):
        """plane_stencil on a register set: its reads must have been released, and have seen the right unit throughout."""
        r = self.regs[name]
        assert r is not None and r["released"], "%s: evaluated before the wait that releases its reads" % (what,)
        for lane in range(WAVE):
            for got in (r["at_issue"][lane], r["value"][lane]):
                assert got == want(lane), "%s: lane %d read %s" % (what, lane, got[:2])
        self.regs[name] = None


def lookup(w, hdr, nspec, cells, log, vmcnt=VMCNT, refill_before_release=False):
    """One density_stencil call in the order of the source."""
    state = hdr["state"]
    desc = state == HOLDS_LAST
    miss = [state == INVALID or hdr["cell"][L] != cells[L] for L in range(WAVE)]
    hdr["cell"] = list(cells)
    hdr["state"] = HOLDS_FIRST if desc else HOLDS_LAST
    step = -512 if desc else 512
    a = prepare(cells, nspec, nspec - 1 if desc else 0)
    assert not w.vm and not w.lgkm, "something is in flight when the lookup starts"
    if any(miss):  # restage_issue: exec-masked, four planes per instruction slot
        for t in range(8):
            lanes = [L for L in range(WAVE) if miss[(L & 56) + t]]
            if lanes:  # an instruction whose exec is empty is skipped: these loads cannot be counted
                for k in range(4):
                    w.dma(nspec, a, t, k * 128, 3 - k, lanes)
    w.wait_vm(0)
    a = [[x + step for x in row] for row in a]
    for s in range(nspec):
        sp = nspec - 1 - s if desc else s
        more = s + 1 < nspec
        last = 0 if more else 1

        def refill(k):
            if more:
                for t in range(8):
                    w.dma(nspec, a, t, k * 128, 3 - k)

        def plane(name, k):
            w.plane(name, lambda lane: [(cells[lane], sp * 512 + k * 128 + q * 16) for q in range(8)], (sp, k))
            log.append((sp, k))

        w.wait_vm(vmcnt[0][last])
        w.read_unit_issue(0, "cf")
        w.wait_vm(vmcnt[1][last])
        w.read_unit_issue(1, "cg")
        if refill_before_release:
            refill(3)
        w.wait_lgkm(8)
        if not refill_before_release:
            refill(3)
        plane("cf", 3)
        w.wait_vm(vmcnt[2][last])
        w.read_unit_issue(2, "cf")
        w.wait_lgkm(8)
        refill(2)
        plane("cg", 2)
        w.wait_vm(vmcnt[3][last])
        w.read_unit_issue(3, "cg")
        w.wait_lgkm(8)
        refill(1)
        plane("cf", 1)
        w.wait_lgkm(0)
        refill(0)
        plane("cg", 0)
        a = [[x + step for x in row] for row in a]
    assert not w.vm, "loads in flight at the lookup's last wait: it is meant to be already true"
    w.wait_vm(0)
    assert not w.lgkm and w.regs == {"cf": None, "cg": None}


def run(nspec, nlookups=10, seed=0, **kw):
    rng = np.random.default_rng(seed)
    w, hdr, log = Wave(), {"state": INVALID, "cell": [-1] * WAVE}, []
    cells = [int(c) for c in rng.integers(0, 257 ** 3, WAVE)]
    directions = set()
    for it in range(nlookups):
        if it == 6:
            hdr["state"] = INVALID  # another writer of the tile (density<NP>)
        move = rng.random(WAVE) < (0.0 if it % 4 == 1 else 0.15)  # it % 4 == 1: every row resident
        cells = [int(rng.integers(0, 257 ** 3)) if m else c for c, m in zip(cells, move)]
        directions.add(hdr["state"] == HOLDS_LAST)
        lookup(w, hdr, nspec, cells, log, **kw)
    assert directions == {False, True}
    assert len(log) == nlookups * 4 * nspec
    return log


@pytest.mark.parametrize("nspec", [1, 2, 3, 4])
def test_every_lane_reads_its_own_unit_in_both_directions(nspec):
    log = run(nspec)
    assert {sp for sp, _ in log} == set(range(nspec)) and {k for _, k in log} == {0, 1, 2, 3}


def test_counts_are_the_tightest_that_may_be_needed():
    """Each count equals the number of DMA instructions issued after the unit about to be read, at the point of the wait, when
    the ring is full (a species in the middle of three or more): a smaller count would wait for loads the read does not need."""
    for unit, (n_more, n_last) in VMCNT.items():
        # issued behind unit `unit` of this species: its later units, and the refills of the buffers already released --
        # buffer k is refilled after unit k + 1's reads are issued, so at the wait for unit `unit` buffers 0 .. unit - 2
        younger_same = 3 - unit
        refilled = max(unit - 1, 0)
        assert n_more == 8 * (younger_same + refilled)
        assert n_last == 8 * younger_same


@pytest.mark.parametrize("unit", [0, 1, 2, 3])
@pytest.mark.parametrize("last", [0, 1])
def test_a_count_one_unit_too_loose_is_caught(unit, last):
    loose = {u: list(v) for u, v in VMCNT.items()}
    loose[unit][last] += 8
    with pytest.raises(AssertionError):
        for nspec in (2, 3, 4):
            run(nspec, vmcnt=loose)


def test_a_refill_before_the_release_of_the_buffers_reads_is_caught():
    with pytest.raises(AssertionError, match="have not been released"):
        run(3, refill_before_release=True)
