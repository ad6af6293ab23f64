"""DMA pieces of the interp model's LDS ring with one M0 per half unit (stanford_raytracer_amd/csrc/srt_models.hpp:
stage_prepare, issue_unit, restage_issue), emulated lane by lane on the host in the style of test_ring_residency_layout.py.

The immediate of an LDS-DMA load shifts the LDS address as well as the global one.  The scheme before this one gave piece t
of a unit its own destination base, ring + J*UNIT + t*1024 - K, and the immediate K = k*128 of the plane.  Now the four
pieces of a half unit share one base, ring + J*UNIT + (t & 4)*1024 - K, step through it with the immediate K + (t & 3)*1024,
and stage_prepare moves a[t] down by (t & 3)*1024 to make up for it.  Both schemes are replayed here over whole lookups
(species order alternating, masked re-stage, resident and re-staged rows, nspec 1-4): every piece must write exactly the LDS
bytes and read exactly the global bytes it did before.  Also: every immediate lies within 0 ... 4095, no M0 base lies below
the end of the residency header, no effective global address leaves the table (first and last cell), a unit's eight pieces
need at most two M0 values -- and a wrong bias or an immediate off by 1024 is caught by the comparison."""
import numpy as np

WAVE, UNIT, RING, PAD = 64, 64 * 128, 4, 2048
RES_END = 2 * WAVE * 4  # RES_CELL int[64] + RES_STATE int[64]
MAX_UNIT_IMM = 384
INVALID, HOLDS_FIRST, HOLDS_LAST = 0, 1, 2
TABLE = 0x7F3A40000000  # where the coefficient table starts (any 512-aligned address)
NCELL = 257 ** 3


class PerPiece:
    """The scheme before: a[t] unbiased, an M0 of its own per piece, the plane's immediate."""
    @staticmethod
    def bias(t):
        return 0

    @staticmethod
    def m0(J, t, K):
        return PAD + J * UNIT + t * 1024 - K

    @staticmethod
    def imm(t, K):
        return K


class HalfUnit:
    """The scheme now: a[t] moved down by (t & 3) KiB, one M0 per half unit, immediates stepping through it."""
    @staticmethod
    def bias(t):
        return (t & 3) * 1024

    @staticmethod
    def m0(J, t, K):
        return PAD + J * UNIT + (t & 4) * 1024 - K

    @staticmethod
    def imm(t, K):
        return K + (t & 3) * 1024


def prepare(scheme, cells, nspec, species):
    """stage_prepare: a[t][L] = block of the cell of lane (L & 56) + t, at `species`, chunk ((L & 7) - t) & 7, less the bias."""
    return [[TABLE + cells[(L & 56) + t] * nspec * 512 + species * 512 + ((((L & 7) - t) & 7) << 4) - scheme.bias(t)
             for L in range(WAVE)] for t in range(8)]


def piece(scheme, a, t, K, J, lanes, nspec, out):
    """One global_load_lds_dwordx4: lane L writes 16 B at M0 + imm + 16 L from a[t][L] + imm."""
    m0, imm = scheme.m0(J, t, K), scheme.imm(t, K)
    assert 0 <= imm <= 4095, "immediate %d outside 0 ... 4095" % imm
    assert m0 >= RES_END, "an M0 base reaches into the residency header"
    moved = []
    for L in lanes:
        dst, src = m0 + imm + 16 * L, a[t][L] + imm
        assert PAD <= dst and dst + 16 <= PAD + RING * UNIT, "DMA leaves the ring"
        assert TABLE <= src and src + 16 <= TABLE + NCELL * nspec * 512, "DMA reads outside the table"
        moved.append((dst, src))
    out.append({"m0": m0, "imm": imm, "moved": moved})


def lookup(scheme, hdr, nspec, cells, out):
    """The DMA pieces of one density_stencil call, in issue order (cf. test_ring_residency_layout.lookup)."""
    state = hdr["state"]
    desc = state == HOLDS_LAST
    miss = [state == INVALID or hdr["cell"][L] != cells[L] for L in range(WAVE)]
    hdr["cell"] = list(cells)
    hdr["state"] = HOLDS_FIRST if desc else HOLDS_LAST
    step = -512 if desc else 512
    a = prepare(scheme, cells, nspec, nspec - 1 if desc else 0)
    if any(miss):  # restage_issue: exec-masked, the four planes of instruction slot t back to back
        for t in range(8):
            lanes = [L for L in range(WAVE) if miss[(L & 56) + t]]
            if lanes:
                for k in (3, 2, 1, 0):
                    piece(scheme, a, t, k * 128, 3 - k, lanes, nspec, out)
    a = [[x + step for x in row] for row in a]
    units = []
    for s in range(nspec):
        if s + 1 < nspec:  # issue_unit: each buffer, once read, takes the same plane of the next species
            for k in (3, 2, 1, 0):
                first = len(out)
                for t in range(8):
                    piece(scheme, a, t, k * 128, 3 - k, range(WAVE), nspec, out)
                units.append(out[first:])
        a = [[x + step for x in row] for row in a]
    return units


def replay(scheme, nspec, seed, lookups=10, cells0=None):
    rng = np.random.default_rng(seed)
    hdr, out, units = {"state": INVALID, "cell": [-1] * WAVE}, [], []
    cells = cells0 if cells0 is not None else [int(c) for c in rng.integers(0, NCELL, WAVE)]
    for it in range(lookups):
        if it == 5:
            hdr["state"] = INVALID  # another writer of the tile (density<NP>)
        move = rng.random(WAVE) < (0.0 if it % 4 == 1 else 0.15)
        cells = [int(rng.integers(0, NCELL)) if m else c for c, m in zip(cells, move)]
        if it == 7:
            hdr["cell"][3] = -1  # a lane given a new ray (new_ray_hook)
        units += lookup(scheme, hdr, nspec, cells, out)
    return out, units


def same_bytes(x, y):
    return len(x) == len(y) and all(p["moved"] == q["moved"] for p, q in zip(x, y))


def test_every_piece_moves_the_bytes_it_moved_before():
    for nspec in (1, 2, 3, 4):
        old, _ = replay(PerPiece, nspec, seed=nspec)
        new, units = replay(HalfUnit, nspec, seed=nspec)
        assert len(old) == len(new) and len(new) > 0
        for p, q in zip(old, new):
            assert p["moved"] == q["moved"]
        # both species directions, full and partly masked re-stages, and lookups with resident rows only, were replayed
        n_lanes = sorted({len(p["moved"]) for p in new})
        assert n_lanes[-1] == WAVE and (nspec == 1 or len(units) == 10 * 4 * (nspec - 1))
        assert any(0 < n < WAVE for n in n_lanes)


def test_immediates_and_bases():
    imms, bases = set(), set()
    for J in range(RING):
        for t in range(8):
            for K in (0, 128, 256, 384):
                imm, m0 = HalfUnit.imm(t, K), HalfUnit.m0(J, t, K)
                assert 0 <= imm <= 4095 and m0 >= RES_END
                assert m0 + imm == PerPiece.m0(J, t, K) + PerPiece.imm(t, K)
                imms.add(imm), bases.add(m0)
    assert max(imms) == MAX_UNIT_IMM + 3 * 1024 == 3456 and min(imms) == 0
    assert min(bases) == PAD - MAX_UNIT_IMM  # the lowest base is the one of the scheme before
    assert bases <= {PerPiece.m0(J, t, K) for J in range(RING) for t in range(8) for K in (0, 128, 256, 384)}


def test_a_unit_needs_two_m0_values():
    _, units = replay(HalfUnit, 4, seed=7)
    assert units
    for u in units:
        assert len(u) == 8
        changes = 1 + sum(1 for p, q in zip(u, u[1:]) if p["m0"] != q["m0"])
        assert changes == 2
    _, units = replay(PerPiece, 4, seed=7)
    assert all(1 + sum(1 for p, q in zip(u, u[1:]) if p["m0"] != q["m0"]) == 8 for u in units)


def test_first_and_last_cell_stay_inside_the_table():
    """a[t] itself may point up to 3 KiB below the table (cell 0, t = 3 or 7); the address a piece reads from may not."""
    for nspec in (1, 2, 3, 4):
        for c in (0, NCELL - 1):
            for scheme in (PerPiece, HalfUnit):
                out, _ = replay(scheme, nspec, seed=3, lookups=4, cells0=[c] * WAVE)  # (piece asserts the bounds)
                assert out
            lo = min(min(row) for row in prepare(HalfUnit, [c] * WAVE, nspec, 0))
            assert (lo < TABLE) == (c == 0)
    # and the bound does catch a piece that reads in front of the table
    class NoImmediateStep(HalfUnit):
        @staticmethod
        def imm(t, K):
            return K
    try:
        replay(NoImmediateStep, 4, seed=3, lookups=1, cells0=[0] * WAVE)
    except AssertionError as e:
        assert "outside the table" in str(e) or "leaves the ring" in str(e)
    else:
        raise AssertionError("a read in front of the table went unnoticed")


def test_wrong_bias_and_shifted_immediate_are_caught():
    old, _ = replay(PerPiece, 4, seed=11)

    class HalfBias(HalfUnit):  # a[t] moved down by half of what the immediates add
        @staticmethod
        def bias(t):
            return (t & 3) * 512

    class NoBias(HalfUnit):
        @staticmethod
        def bias(t):
            return 0

    class ImmOneStepLate(HalfUnit):  # immediates off by 1024, base unchanged: lands one piece further on
        @staticmethod
        def imm(t, K):
            return K + (((t & 3) + 1) & 3) * 1024

    class ImmAndBaseShifted(HalfUnit):  # immediate off by 1024 with the base moved to match: LDS right, global wrong
        @staticmethod
        def imm(t, K):
            return K + (t & 3) * 1024 + 512

        @staticmethod
        def m0(J, t, K):
            return HalfUnit.m0(J, t, K) - 512

    for wrong in (HalfBias, NoBias, ImmOneStepLate, ImmAndBaseShifted):
        try:
            new, _ = replay(wrong, 4, seed=11)
        except AssertionError:
            continue  # already outside the ring, the table or the immediate's range
        assert not same_bytes(old, new), wrong.__name__
    new, _ = replay(HalfUnit, 4, seed=11)
    assert same_bytes(old, new)
