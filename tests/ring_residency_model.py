"""The ring of the interp model's residency scheme as the host emulations see it: its constants, the LDS-DMA instruction, the
address preparation and a lane's read of a unit, shared by tests/test_ring_residency_layout.py and
tests/test_ring_read_ahead_layout.py.  Not a test module."""
WAVE, UNIT, RING, PAD = 64, 64 * 128, 4, 2048
RES_END = 2 * WAVE * 4  # RES_CELL int[64] + RES_STATE int[64]
MAX_IMM = 384
INVALID, HOLDS_FIRST, HOLDS_LAST = 0, 1, 2


def dma(lds, nspec, a, t, imm, J, lanes=range(WAVE)):
    """Instruction t of a unit: lane L writes 16 B at M0 + imm + 16 L from a[L] + imm (tools/probes/dma_probe.hip)."""
    stride = nspec * 512
    m0 = PAD + J * UNIT + t * 1024 - imm  # issue_unit / restage_species: destination biased by -imm
    assert 0 <= imm <= MAX_IMM and m0 >= RES_END, "a DMA base reaches into the residency header"
    for L in lanes:
        dst, src = m0 + imm + 16 * L, a[t][L] + imm
        assert PAD <= dst and dst + 16 <= PAD + RING * UNIT, "DMA leaves the ring"
        lds[dst] = (src // stride, src % stride)


def prepare(cells, nspec, species):
    """stage_prepare: a[t][L] = block of the cell of lane (L & 56) + t, at `species`, chunk ((L & 7) - t) & 7."""
    return [[cells[(L & 56) + t] * nspec * 512 + species * 512 + ((((L & 7) - t) & 7) << 4) for L in range(WAVE)]
            for t in range(8)]


def read_unit(lds, J, lane):
    row = PAD + J * UNIT + (8 * (lane & 7) + (lane >> 3)) * 128  # read_addrs
    return [lds.get(row + (((q + lane) & 7) << 4)) for q in range(8)]
