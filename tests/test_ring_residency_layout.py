"""Ring residency of the interp model (stanford_raytracer_amd/csrc/srt_models.hpp: InterpModel::density_stencil,
restage_species, the RES_* header), emulated lane by lane on the host in the style of test_ring_layout.py: the species
order alternates between lookups, a[] is moved by +-512 B per species (immediates stay k*128), the lanes whose cell
changed get their rows re-staged by exec-masked LDS-DMA, and every unit a lane reads must hold its own cell's
coefficients of the right (species, k-plane) -- whether the rows were resident or re-staged.  (The kernel itself is
tested on the GPU: test_gpu_ring_residency.py.)"""
import numpy as np

from ring_residency_model import (HOLDS_FIRST, HOLDS_LAST, INVALID, MAX_IMM, PAD, RES_END, RING, UNIT, WAVE, dma, prepare,
                                  read_unit)


def lookup(lds, hdr, nspec, cells, log):
    """One density_stencil call; returns the lanes that were re-staged.  `log` collects (lane, species, k) reads checked."""
    state = hdr["state"]
    desc = state == HOLDS_LAST
    miss = [state == INVALID or hdr["cell"][L] != cells[L] for L in range(WAVE)]
    hdr["cell"] = list(cells)
    hdr["state"] = HOLDS_FIRST if desc else HOLDS_LAST
    first = nspec - 1 if desc else 0
    step = -512 if desc else 512
    a = prepare(cells, nspec, first)
    restaged = set()
    if any(miss):
        for t in range(8):
            # exec of instruction t: the 8-lane groups whose owner lane (g + t) missed
            lanes = [L for L in range(WAVE) if miss[(L & 56) + t]]
            for L in lanes:
                restaged.add((L & 56) + t)  # the row slot written belongs to lane (L & 56) + t
            for k in range(4):
                dma(lds, nspec, a, t, k * 128, 3 - k, lanes)
    a = [[x + step for x in row] for row in a]
    for s in range(nspec):
        sp = nspec - 1 - s if desc else s
        more = s + 1 < nspec
        for k in (3, 2, 1, 0):
            J = 3 - k
            for lane in range(WAVE):
                got = read_unit(lds, J, lane)
                want = [(cells[lane], sp * 512 + k * 128 + q * 16) for q in range(8)]
                assert got == want, "lane %d species %d plane %d read %s" % (lane, sp, k, got[:2])
                log.append((lane, sp, k))
            if more:  # the buffer just read takes the same plane of the next species
                for t in range(8):
                    dma(lds, nspec, a, t, k * 128, J)
        a = [[x + step for x in row] for row in a]
    return restaged, miss


def test_header_and_every_dma_base_stay_apart():
    assert RES_END <= PAD - MAX_IMM
    for J in range(RING):
        for t in range(8):
            for imm in (0, 128, 256, 384):
                assert PAD + J * UNIT + t * 1024 - imm >= RES_END


def test_masked_restage_writes_exactly_the_mismatched_lanes_rows():
    rng = np.random.default_rng(1)
    for trial in range(20):
        nspec = int(rng.integers(1, 5))
        miss = rng.random(WAVE) < rng.choice([0.02, 0.2, 0.7])
        lds, written = {}, set()
        cells = [int(c) for c in rng.integers(0, 1000, WAVE)]
        a = prepare(cells, nspec, 0)
        for t in range(8):
            lanes = [L for L in range(WAVE) if miss[(L & 56) + t]]
            before = set(lds)
            dma(lds, nspec, a, t, 384, 0, lanes)
            written |= set(lds) - before
        # the row slots written are exactly those the mismatched lanes read
        rows = {(addr - PAD) // 128 for addr in written}
        want = {8 * (j & 7) + (j >> 3) for j in range(WAVE) if miss[j]}
        assert rows == want
        for j in range(WAVE):
            if miss[j]:
                assert read_unit(lds, 0, j) == [(cells[j], 384 + 16 * q) for q in range(8)]


def test_resident_and_restaged_rows_read_back_the_right_cell():
    rng = np.random.default_rng(0)
    for nspec in (1, 2, 3, 4):
        lds, hdr, log = {}, {"state": INVALID, "cell": [-1] * WAVE}, []
        cells = [int(c) for c in rng.integers(0, 257 ** 3, WAVE)]
        n_restaged = []
        for it in range(12):
            if it in (5, 9):
                hdr["state"] = INVALID  # another writer of the tile (density<NP>)
            move = rng.random(WAVE) < (0.0 if it % 4 == 1 else 0.15)
            cells = [int(rng.integers(0, 257 ** 3)) if m else c for c, m in zip(cells, move)]
            if it == 7:
                hdr["cell"][3] = -1  # a lane given a new ray (new_ray_hook)
            restaged, miss = lookup(lds, hdr, nspec, cells, log)
            assert restaged == {j for j in range(WAVE) if miss[j]}
            n_restaged.append(len(restaged))
        assert n_restaged[0] == WAVE and 0 in n_restaged and any(0 < n < WAVE for n in n_restaged)
        assert len(log) == 12 * WAVE * 4 * nspec


def test_descending_order_addresses_and_immediates():
    """a[] moved per species: every global address stays inside the lane's cell block and every immediate fits 12 bits."""
    nspec = 4
    cells = list(range(100, 164))
    a = prepare(cells, nspec, nspec - 1)
    for s in range(nspec):
        sp = nspec - 1 - s
        for t in range(8):
            for L in range(WAVE):
                for k in range(4):
                    src = a[t][L] + k * 128
                    blk = cells[(L & 56) + t] * nspec * 512
                    assert blk + sp * 512 <= src and src + 16 <= blk + (sp + 1) * 512
                    assert 0 <= k * 128 < 4096
        a = [[x - 512 for x in row] for row in a]
