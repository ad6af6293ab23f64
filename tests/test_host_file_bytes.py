"""CPU: every host file format pinned byte for byte.  Each writer of the library runs on the smallest inputs that reach every
branch of its record, and the sha256 of each file is compared with tests/golden/host_file_bytes.json; each reader runs on
crafted bad files, and its return code and srt_last_error() text are compared with the same JSON; the readers' good paths are
round trips against the arrays written.  The JSON was recorded with `python tests/test_host_file_bytes.py` from the library
as it stood before the file formats were gathered in csrc/srt_host.cpp: a change of a byte or of a refusal text shows here."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN_DIR
from stanford_raytracer_amd import api

JSON = os.path.join(GOLDEN_DIR, "host_file_bytes.json")
SPECIAL = [np.nan, np.inf, -np.inf, -0.0, 5e-324, 1.7976931348623157e308, 9.9999999999999995e22]
B6 = np.array([-3.0e7, 3.0e7, -2.0e7, 2.0e7, -1.0e7, 1.5e7])
QS = np.array([-1.602e-19, 1.602e-19, 1.602e-19, 1.602e-19])
MS = np.array([9.10938188e-31, 1.6726e-27, 6.6904e-27, 2.67616e-26])


def values(n, salt=0, special=True):
    """n doubles from exact IEEE operations alone (a product with the literal 0.1, a power of two), the SPECIAL ones first."""
    i = np.arange(n, dtype=np.float64) + salt
    v = np.ldexp((i + 1.0) * 0.1 * np.where(i % 2 == 0, 1.0, -1.0), ((3 * i) % 120 - 60).astype(np.int64))
    if special:
        k = min(n, len(SPECIAL))
        v[:k] = SPECIAL[:k]
    return v


def r16(a):
    """What 16 significant digits keep of a: the array a text file gives back."""
    a = np.asarray(a, dtype=np.float64)
    return np.array([float("%.15E" % x) for x in a.flat]).reshape(a.shape)


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


def sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def refusal(path_dir, fn, *args):
    """The text of the SrtError fn(*args) raises, the directory's name taken out of it; "accepted" if it raises nothing."""
    try:
        fn(*args)
    except api.SrtError as e:
        return str(e).replace(str(path_dir), "<dir>")
    return "accepted"


# ---- the writers -------------------------------------------------------------------------------------------------------
def write_grids(d, out):
    for nspec in (1, 4):
        for with_derivs in (False, True):
            F = values(8 * nspec, 1).reshape(2, 2, 2, nspec)
            derivs = [values(8 * nspec, 10 * a, special=a == 3).reshape(F.shape) for a in range(7)] if with_derivs else None
            for binary in (False, True):
                name = "grid_n%d_d%d.%s" % (nspec, with_derivs, "bin" if binary else "txt")
                p = str(d / name)
                api.write_grid_file(p, F, B6, QS[:nspec], MS[:nspec], derivs=derivs, binary=binary)
                out[name] = sha(p)
                assert api.grid_file_is_binary(p) == binary
                g = api.read_grid_file(p)
                back = (lambda x: x) if binary else r16
                assert same(g["F"], back(F)) and same(g["bounds"], back(B6)), name
                assert same(g["qs"], back(QS[:nspec])) and same(g["ms"], back(MS[:nspec])), name
                assert (g["derivs"] is None) == (not with_derivs), name
                if with_derivs:
                    assert all(same(x, back(y)) for x, y in zip(g["derivs"], derivs)), name
            conv = str(d / "conv.bin")
            api.convert_grid_file(str(d / ("grid_n%d_d%d.txt" % (nspec, with_derivs))), conv)
            out["grid_n%d_d%d.converted" % (nspec, with_derivs)] = sha(conv)


def write_points(d, out):
    for nspec in (1, 4):
        rec = values(3 * (3 + nspec), 2).reshape(3, 3 + nspec)
        for binary in (False, True):
            name = "points_n%d.%s" % (nspec, "bin" if binary else "txt")
            p = str(d / name)
            api.write_points_file(p, rec, B6, QS[:nspec], MS[:nspec], binary=binary)
            out[name] = sha(p)
            assert api.points_file_is_binary(p) == binary
        conv = str(d / "pconv.bin")
        api.convert_points_file(str(d / ("points_n%d.txt" % nspec)), conv)
        out["points_n%d.converted" % nspec] = sha(conv)
        assert same(np.fromfile(conv, dtype=np.float64, offset=136).reshape(3, 3 + nspec), r16(rec))
        assert same(np.fromfile(str(d / ("points_n%d.bin" % nspec)), dtype=np.float64, offset=136).reshape(3, 3 + nspec), rec)


def write_dumps(d, out):
    for nspec, (nz, ny, nx) in ((1, (1, 1, 1)), (4, (3, 1, 2))):
        f = values(nz * ny * nx * (4 * nspec + 3), 3).reshape(nz, ny, nx, 4 * nspec + 3)
        name = "dump_%dx%dx%d.txt" % (nx, ny, nz)
        p = str(d / name)
        api.write_dump_file(p, f, B6)
        out[name] = sha(p)
        g = api.read_dump_file(p)
        assert g["nspec"] == nspec and same(g["f"], r16(f)) and same(g["bounds"], r16(B6)), name


def write_events(d, out):
    for ne in (0, 1, 3):
        raynum = np.array([1, 9999999999, 42][:ne], dtype=np.int64)
        meta = np.array([[0, 0, 0, 1], [1, 15, 2147483646, -1], [2, 3, 7, 0]][:ne], dtype=np.int32).reshape(ne, 4)
        rows = values(ne * 20, 4).reshape(ne, 20)
        dist = values(ne, 5)
        p = str(d / ("crossings_%d.txt" % ne))
        api.write_crossings_file(p, raynum, meta, rows)
        out["crossings_%d.txt" % ne] = sha(p)
        p = str(d / ("approaches_%d.txt" % ne))
        api.write_approaches_file(p, raynum, meta, dist, rows)
        out["approaches_%d.txt" % ne] = sha(p)


def write_tubes(d, out):
    offsets = np.array([0, 2, 5], dtype=np.int64)
    rows = values(5 * 20, 6).reshape(5, 20)
    section = values(5 * 4, 7).reshape(5, 4)
    flag = np.array([0, 1, 2, 0, 5], dtype=np.int32)
    p = str(d / "tubes.txt")
    api.write_tubes_file(p, np.array([7, 9999999999], dtype=np.int64), offsets, rows, section, flag)
    out["tubes.txt"] = sha(p)
    p = str(d / "tubes_0.txt")
    api.write_tubes_file(p, np.zeros(0, dtype=np.int64), np.zeros(1, dtype=np.int64), np.zeros((0, 20)), np.zeros((0, 4)),
                         np.zeros(0, dtype=np.int32))
    out["tubes_0.txt"] = sha(p)


BIN1 = [("x", [0.0, 1.0])]
BIN3 = [("x", [-1.0e7, 0.5, 2.0e7]), ("sinlat", [-1.0, 1.0]), ("r", [6.4e6, 7.0e6, 1.0e7, 5.0e7])]


def write_bins(d, out):
    for name, axes, ticks, hits, quantum in (
            ("bin_1.txt", BIN1, [5], [2], 2.0 ** -30),
            ("bin_3.txt", BIN3, [0, 1, 2 ** 62, 3, 4, 5], [0, 9, 2 ** 40, 1, 2, 3], 0.1),
            ("bin_3_noticks.txt", BIN3, None, [1, 2, 3, 4, 5, 6], 2.0 ** -30),
            ("bin_3_nohits.txt", BIN3, [1, 2, 3, 4, 5, 6], None, 2.0 ** -30),
            ("bin_3_none.txt", BIN3, None, None, 2.0 ** -30)):
        axl = [api.axis(k, e) for k, e in axes]
        p = str(d / name)
        api.write_bin_file(p, axl, ticks, hits, nsub=3, quantum=quantum)
        out[name] = sha(p)
        g = api.read_bin_file(p)
        n = len(axl) and int(np.prod([len(e) - 1 for _, e in axl]))
        assert g["nsub"] == 3 and g["quantum"] == float("%.15E" % quantum), name
        assert [k for k, _ in g["axes"]] == [k for k, _ in axl] and all(same(a[1], r16(b[1])) for a, b in zip(g["axes"], axl)), name
        want_sum = r16(np.array(ticks if ticks is not None else [0] * n, dtype=np.int64).astype(np.float64) * quantum)
        assert same(g["sum"].reshape(-1), want_sum), name
        want_hits = np.array(hits if hits is not None else [0] * n, dtype=np.int64)
        # (hits pass through a double in the reader: 2^40 is exact)
        assert np.array_equal(g["hits"].reshape(-1), want_hits), name


def write_rays(d, out, monkeypatch):
    p = api.make_params(maxsteps=3, outputper=1)
    slots = api.lib().srt_rows_per_ray(C.byref(p))
    for nspec in (1, 4):
        sp = (nspec, QS[:nspec], MS[:nspec])
        rows = values(2 * slots * 20, 8).reshape(2, slots, 20)
        rows[:, 1:, 0] = np.arange(1, slots)[None, :] * 1e-3       # later rows have t > 0: rays stay apart in the reader
        rows[:, 0, 0] = 0.0
        w0 = np.array([1.0e4, 5e-324])
        nrows, stop = np.array([slots, 2], dtype=np.int32), np.array([0, 6], dtype=np.int32)
        for nth in ("1", "3"):
            monkeypatch.setenv("SRT_IO_THREADS", nth)
            for nrays, tag in ((0, "0rays"), (1, "norow"), (2, "2rays")):
                nr = np.zeros(1, dtype=np.int32) if tag == "norow" else nrows[:nrays]
                name = "ray_n%d_%s_t%s" % (nspec, tag, nth)
                a, b = str(d / (name + ".padded")), str(d / (name + ".packed"))
                api.write_ray_file(a, sp, p, w0[:nrays], rows[:nrays], nr, stop[:nrays], raynum0=9999999998)
                off = np.concatenate([[0], np.cumsum(nr)]).astype(np.int64)
                packed = np.concatenate([rows[r, :nr[r]] for r in range(nrays)] + [np.zeros((0, 20))])
                api.write_ray_file_packed(b, sp, w0[:nrays], off, packed, stop[:nrays], raynum0=9999999998)
                out[name + ".padded"], out[name + ".packed"] = sha(a), sha(b)
                assert out[name + ".padded"] == out[name + ".packed"], name
            # append: the two rays again, under other numbers, behind the file of two
            name = "ray_n%d_append_t%s" % (nspec, nth)
            a, b = str(d / (name + ".padded")), str(d / (name + ".packed"))
            for path in (a, b):
                api.write_ray_file(path, sp, p, w0, rows, nrows, stop, raynum0=1)
            api.write_ray_file(a, sp, p, w0, rows, nrows, stop, raynum0=3, append=True)
            api.write_ray_file_packed(b, sp, w0, off, packed, stop, raynum0=3, append=True)
            out[name + ".padded"], out[name + ".packed"] = sha(a), sha(b)
            r = api.read_ray_file(a)
            assert r["nspec"] == nspec and r["raynum"].tolist() == [1, 2, 3, 4] and r["kept"].tolist() == [slots, 2] * 2, name
            assert r["stopcond"].tolist() == [0, 6] * 2 and same(r["w0"], r16(np.tile(w0, 2))), name
            assert same(r["qs"], r16(QS[:nspec])) and same(r["ms"], r16(MS[:nspec])), name
            want = np.zeros((2 * len(packed), 20))
            want[:, :16 + nspec] = r16(np.tile(packed, (2, 1)))[:, :16 + nspec]
            assert same(r["rows"], want), name
    rays = str(d / "rays.txt")
    open(rays, "w").write("1 2 3 0 0 1 5000.\n1d0,2,3 , 0 0 1 6.0D3\n 1 2 3\n")
    pos, dr, w = api.read_rays_file(rays)
    assert pos.tolist() == [[1, 2, 3]] * 2 and dr.tolist() == [[0, 0, 1]] * 2 and w.tolist() == [5000.0, 6000.0]


def written(d, monkeypatch):
    out = {}
    write_grids(d, out)
    write_points(d, out)
    write_dumps(d, out)
    write_events(d, out)
    write_tubes(d, out)
    write_bins(d, out)
    write_rays(d, out, monkeypatch)
    return out


# ---- the refusals ------------------------------------------------------------------------------------------------------
def refused(d):
    out = {}

    def put(name, text):
        p = d / name
        p.write_bytes(text if isinstance(text, bytes) else text.encode())
        return str(p)

    # grid, text: 2 x 2 x 2, one species, with and without derivative blocks
    F = values(8, 1, special=False).reshape(2, 2, 2, 1)
    good, goodd, goodb = str(d / "g.txt"), str(d / "gd.txt"), str(d / "g.bin")
    api.write_grid_file(good, F, B6, QS[:1], MS[:1])
    api.write_grid_file(goodd, F, B6, QS[:1], MS[:1], derivs=[F] * 7)
    api.write_grid_file(goodb, F, B6, QS[:1], MS[:1], derivs=[F] * 7, binary=True)
    L, Ld, raw = open(good).read().split("\n")[:-1], open(goodd).read().split("\n")[:-1], open(goodb, "rb").read()
    hdr = lambda *v: "%10d%10d%10d%10d%10d" % v  # noqa: E731
    grids = {
        "grid_missing": None,
        "grid_empty": "",
        "grid_cut_sizes": "         0         1         2\n",
        "grid_cut_bounds": L[0] + "\n" + L[1][:72] + "\n",
        "grid_cut_charges": "\n".join(L[:2]) + "\n",
        "grid_cut_masses": "\n".join(L[:3]) + "\n",
        "grid_cut_values": "\n".join(L[:7]) + "\n",
        "grid_cut_derivs": "\n".join(Ld[:4 + 8 + 8 * 3 + 2]) + "\n",
        "grid_token_sizes": "0 one 2 2 2\n" + "\n".join(L[1:]) + "\n",
        "grid_token_bounds": L[0] + "\n" + L[1][:24] + " abc " + L[1][48:] + "\n" + "\n".join(L[2:]) + "\n",
        "grid_token_values": "\n".join(L[:6] + ["xyz"] + L[7:]) + "\n",
        "grid_token_derivs": "\n".join(Ld[:20] + ["1.0.0"] + Ld[21:]) + "\n",
        "grid_nspec0": "\n".join([hdr(0, 0, 2, 2, 2)] + L[1:]) + "\n",
        "grid_nspec5": "\n".join([hdr(0, 5, 2, 2, 2)] + L[1:]) + "\n",
        "grid_one_node": "\n".join([hdr(0, 1, 2, 1, 2)] + L[1:]) + "\n",
        "grid_extra_values": "\n".join(L + L[4:6]) + "\n",
        "grid_bin_magic": b"SRTGRID2" + raw[8:],
        "grid_bin_cut_header": raw[:100],
        "grid_bin_cut_values": raw[:144 + 8 * 8 * 3 + 4],
        "grid_bin_nspec0": raw[:12] + np.int32(0).tobytes() + raw[16:],
        "grid_bin_nspec5": raw[:12] + np.int32(5).tobytes() + raw[16:],
        "grid_bin_one_node": raw[:20] + np.int32(1).tobytes() + raw[24:],
    }
    for name, text in grids.items():
        p = str(d / name) if text is None else put(name, text)
        out[name] = refusal(d, api.read_grid_file, p)
        out[name + ":convert"] = refusal(d, api.convert_grid_file, p, str(d / "o.bin"))
    assert same(api.read_grid_file(put("grid_records", "\n".join(L[:4] + [x + " 9.0" for x in L[4:]]) + "\n"))["F"], r16(F))

    # dump
    f = values(7, 3, special=False).reshape(1, 1, 1, 7)
    api.write_dump_file(str(d / "d.txt"), f, B6)
    D = open(str(d / "d.txt")).read().split("\n")[:-1]
    for name, text in {
            "dump_missing": None, "dump_empty": "",
            "dump_cut_header": D[0] + "\n" + D[1][:96] + "\n",
            "dump_cut_values": "\n".join(D[:5]) + "\n",
            "dump_extra_values": "\n".join(D + D[2:3]) + "\n",
            "dump_token": "\n".join(D[:4] + ["1.0x"] + D[5:]) + "\n",
            "dump_nspec0": "%10d%10d%10d%10d\n" % (0, 1, 1, 1) + "\n".join(D[1:]) + "\n",
            "dump_nspec5": "%10d%10d%10d%10d\n" % (5, 1, 1, 1) + "\n".join(D[1:]) + "\n",
            "dump_nx0": "%10d%10d%10d%10d\n" % (1, 0, 1, 1) + "\n".join(D[1:]) + "\n"}.items():
        out[name] = refusal(d, api.read_dump_file, str(d / name) if text is None else put(name, text))

    # bin
    api.write_bin_file(str(d / "b.txt"), [api.axis(k, e) for k, e in BIN3], [1, 2, 3, 4, 5, 6], None)
    Bn = open(str(d / "b.txt")).read().split("\n")[:-1]
    for name, text in {
            "bin_missing": None, "bin_empty": "",
            "bin_cut_header": Bn[0][:20] + "\n",
            "bin_naxes4": "%10d" % 4 + Bn[0][10:] + "\n" + "\n".join(Bn[1:]) + "\n",
            "bin_cut_axis_header": "\n".join(Bn[:3]) + "\n" + Bn[3][:10] + "\n",
            "bin_axis_kind8": "\n".join(Bn[:1] + ["%10d%10d" % (8, 2)] + Bn[2:]) + "\n",
            "bin_cut_edges": "\n".join(Bn[:1] + Bn[1:2] + [Bn[2][:48]]) + "\n",
            "bin_edges_decrease": "\n".join(Bn[:2] + [Bn[2][48:72] + Bn[2][24:48] + Bn[2][:24]] + Bn[3:]) + "\n",
            "bin_cell_count": "\n".join(Bn[:-1]) + "\n",
            "bin_extra_cell": "\n".join(Bn + Bn[-1:]) + "\n",
            "bin_token": "\n".join(Bn[:-1] + ["nope 1"]) + "\n"}.items():
        out[name] = refusal(d, api.read_bin_file, str(d / name) if text is None else put(name, text))

    # .ray
    p3 = api.make_params(maxsteps=2, outputper=1)
    rows = values(2 * 2 * 20, 8, special=False).reshape(2, 2, 20)
    rows[:, 0, 0], rows[:, 1, 0] = 0.0, 1e-3
    api.write_ray_file(str(d / "r.ray"), (2, QS[:2], MS[:2]), p3, np.array([1e4, 2e4]), rows, np.array([2, 2], dtype=np.int32),
                       np.array([0, 1], dtype=np.int32))
    R = open(str(d / "r.ray")).read().split("\n")[:-1]
    per = 20 + 17 * 24 + 10
    for name, text in {
            "ray_missing": None,
            "ray_cut_first_record": R[0][:300] + "\n",
            "ray_cut_last_record": "\n".join(R[:3] + [R[3][:-48]]) + "\n",
            "ray_nspec0": R[0][:per - 10] + "%10d" % 0 + R[0][per:] + "\n",
            "ray_nspec5": R[0][:per - 10] + "%10d" % 5 + R[0][per:] + "\n",
            "ray_nspec_changes": "\n".join(R[:2] + [R[2][:per - 10] + "%10d" % 1 + R[2][per:]] + R[3:]) + "\n",
            "ray_token": "\n".join(R[:2] + [R[2][:44] + " " * 21 + "***" + R[2][68:]] + R[3:]) + "\n"}.items():
        out[name] = refusal(d, api.read_ray_file, str(d / name) if text is None else put(name, text))
    e = api.read_ray_file(put("ray_empty", ""))
    assert len(e["raynum"]) == 0 and e["rows"].shape == (0, 20) and e["nspec"] == 0
    out["rays_missing"] = refusal(d, api.read_rays_file, str(d / "rays_missing"))

    # points (the text reader behind srt_points_file_convert; the binary reader is reached through a model alone and is
    # driven by tests/native/host_files_main.cpp)
    rec = values(3 * 4, 2, special=False).reshape(3, 4)
    api.write_points_file(str(d / "p.txt"), rec, B6, QS[:1], MS[:1])
    api.write_points_file(str(d / "p.bin"), rec, B6, QS[:1], MS[:1], binary=True)
    P, praw = open(str(d / "p.txt")).read().split("\n")[:-1], open(str(d / "p.bin"), "rb").read()
    for name, text in {
            "points_missing": None, "points_empty": "",
            "points_binary": praw,
            "points_cut_header": P[0] + "\n" + P[1][:96] + "\n",
            "points_cut_masses": "\n".join(P[:3]) + "\n",
            "points_cut_record": "\n".join(P[:5] + [P[5][:48]]) + "\n",
            "points_token": "\n".join(P[:5] + ["a b c d"] + P[6:]) + "\n",
            "points_nspec0": "%10d\n" % 0 + "\n".join(P[1:]) + "\n",
            "points_nspec5": "%10d\n" % 5 + "\n".join(P[1:]) + "\n"}.items():
        out[name] = refusal(d, api.convert_points_file, str(d / name) if text is None else put(name, text), str(d / "o.bin"))
    out["points_bin_magic:is_binary"] = api.points_file_is_binary(put("points_bin_magic", b"SRTPTS02" + praw[8:]))
    out["points_short:is_binary"] = api.points_file_is_binary(put("points_short", praw[:7]))
    out["grid_bin_magic:is_binary"] = api.grid_file_is_binary(str(d / "grid_bin_magic"))
    out["grid_missing:is_binary"] = api.grid_file_is_binary(str(d / "grid_missing"))

    # what the writers refuse: a file that cannot be opened, a ray number beyond i10, packed offsets that are none
    nodir = str(d / "no" / "such")
    ev = (np.array([1], dtype=np.int64), np.zeros((1, 4), dtype=np.int32))
    sp, one, st = (1, QS[:1], MS[:1]), np.ones(1), np.zeros(1, dtype=np.int32)
    off2, rows1 = np.array([0, 1], dtype=np.int64), np.zeros((1, 20))
    p1 = api.make_params(maxsteps=1, outputper=1)
    out["open_grid_text"] = refusal(d, api.write_grid_file, nodir, F, B6, QS[:1], MS[:1])
    out["open_grid_binary"] = refusal(d, lambda: api.write_grid_file(nodir, F, B6, QS[:1], MS[:1], binary=True))
    out["open_points_text"] = refusal(d, api.write_points_file, nodir, rec, B6, QS[:1], MS[:1])
    out["open_points_binary"] = refusal(d, lambda: api.write_points_file(nodir, rec, B6, QS[:1], MS[:1], binary=True))
    out["open_dump"] = refusal(d, api.write_dump_file, nodir, f, B6)
    out["open_crossings"] = refusal(d, api.write_crossings_file, nodir, ev[0], ev[1], rows1)
    out["open_approaches"] = refusal(d, api.write_approaches_file, nodir, ev[0], ev[1], one, rows1)
    out["open_tubes"] = refusal(d, api.write_tubes_file, nodir, ev[0], off2, rows1, np.zeros((1, 4)), st)
    out["open_bin"] = refusal(d, api.write_bin_file, nodir, [api.axis(*BIN1[0])], [1], [1])
    out["open_ray"] = refusal(d, api.write_ray_file, nodir, sp, p1, one, rows1.reshape(1, 1, 20), st + 1, st)
    out["open_ray_packed"] = refusal(d, api.write_ray_file_packed, nodir, sp, one, off2, rows1, st)
    ok = str(d / "w.txt")
    big = np.array([10 ** 10], dtype=np.int64)
    out["i10_ray"] = refusal(d, lambda: api.write_ray_file(ok, sp, p1, one, rows1.reshape(1, 1, 20), st + 1, st, raynum0=10 ** 10))
    out["i10_ray_negative"] = refusal(d, lambda: api.write_ray_file_packed(ok, sp, one, off2, rows1, st, raynum0=-1))
    out["i10_crossings"] = refusal(d, api.write_crossings_file, ok, big, ev[1], rows1)
    out["i10_approaches"] = refusal(d, api.write_approaches_file, ok, -big, ev[1], one, rows1)
    out["i10_tubes"] = refusal(d, api.write_tubes_file, ok, big, off2, rows1, np.zeros((1, 4)), st)
    lib, i64p = api.lib(), C.POINTER(C.c_int64)
    for name, offs in (("offsets_first", [1, 2, 3]), ("offsets_decrease", [0, 2, 1])):
        o = np.array(offs, dtype=np.int64)
        r3, w2, s2, n2 = np.zeros((3, 20)), np.ones(2), np.zeros(3, dtype=np.int32), np.array([1, 2], dtype=np.int64)
        for who, call in (("ray_packed", lambda: lib.srt_write_ray_file_packed(
                              ok.encode(), 0, 1, 2, 1, api._dp(QS), api._dp(MS), api._dp(w2), o.ctypes.data_as(i64p), api._dp(r3),
                              s2.ctypes.data_as(api.ip))),
                          ("tubes", lambda: lib.srt_tubes_file_write(
                              ok.encode(), 2, n2.ctypes.data_as(i64p), o.ctypes.data_as(i64p), api._dp(r3), api._dp(np.zeros((3, 4))),
                              s2.ctypes.data_as(api.ip)))):
            out["%s_%s" % (name, who)] = "srt error %d: %s" % (call(), lib.srt_last_error().decode())
    return out


# ---- the tests ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def recorded():
    return json.load(open(JSON))


def differing(got, want):
    return {k: (got.get(k), want.get(k)) for k in sorted(set(got) | set(want)) if got.get(k) != want.get(k)}


def test_every_writer_gives_the_recorded_bytes(tmp_path, monkeypatch, recorded):
    assert differing(written(tmp_path, monkeypatch), recorded["written"]) == {}


def test_every_reader_refuses_with_the_recorded_code_and_text(tmp_path, recorded):
    assert differing(refused(tmp_path), recorded["refused"]) == {}


def test_a_grid_text_file_the_parallel_reader_cuts_into_pieces(tmp_path):
    """12 x 12 x 12 x 4 values are 172 KB of text, more than the 32 x 4096 bytes below which the reader stays on one thread."""
    F = r16(values(12 * 12 * 12 * 4, 9)).reshape(12, 12, 12, 4)
    p = str(tmp_path / "g.txt")
    api.write_grid_file(p, F, B6, QS, MS)
    assert os.path.getsize(p) >= 32 * 4096
    g = api.read_grid_file(p)
    assert same(g["F"], F) and same(g["bounds"], B6) and g["derivs"] is None
    d = [r16(values(F.size, 100 * a)).reshape(F.shape) for a in range(7)]
    api.write_grid_file(p, F, B6, QS, MS, derivs=d)
    g = api.read_grid_file(p)
    assert same(g["F"], F) and all(same(x, y) for x, y in zip(g["derivs"], d))


if __name__ == "__main__":  # record: python tests/test_host_file_bytes.py
    import pathlib
    import tempfile

    mp = pytest.MonkeyPatch()
    with tempfile.TemporaryDirectory() as a, tempfile.TemporaryDirectory() as b:
        doc = {"written": written(pathlib.Path(a), mp), "refused": refused(pathlib.Path(b))}
    mp.undo()
    json.dump(doc, open(JSON, "w"), indent=1, sort_keys=True)
    open(JSON, "a").write("\n")
    print("%d files, %d refusals -> %s" % (len(doc["written"]), len(doc["refused"]), JSON), file=sys.stderr)
