#!/usr/bin/env python3
"""Are the instruction streams of two builds' kernels the same?  Takes two gfx950 listings of csrc/srt_api.hip
(hipcc -O3 --offload-arch=gfx950 -std=c++17 -S --cuda-device-only -o FILE.s srt_api.hip), one of a parent commit and one of
the working tree, and compares every function whose mangled name contains one of the given words, instruction by instruction
(comments dropped, local labels renumbered).  Prints per function the instruction counts of both and IDENTICAL / DIFFERENT, for
kernels also the registers, spills and scratch of the new listing's metadata; functions only the new listing has are listed with
their counts.  Ends with the number of functions of the parent listing, whatever their names, that the new one changes or lacks.

    python tools/compare_kernel_isa.py parent.s new.s NgoModel Ngo3dModel ngo_norm
"""
import re
import sys


def functions(path):
    out, cur, name, code = {}, None, None, set()
    for ln in open(path):
        t = re.match(r"\s+\.type\s+(\S+),@function", ln)
        if t:
            code.add(t.group(1))  # (data symbols have labels of the same shape)
        m = re.match(r"^(_Z\w+):\s*(;.*)?$", ln)
        if m and m.group(1) not in code:
            name = None
        elif m:
            name = m.group(1)
            cur = out.setdefault(name, [])
            continue
        if name is None:
            continue
        s = ln.strip()
        if s.startswith(".Lfunc_end"):
            name = None
            continue
        if not s or s.startswith((";", ".", "#")) or s.endswith(":"):
            continue
        s = re.sub(r"\s*;.*$", "", s)
        cur.append(re.sub(r"\.LBB\d+_\d+", ".LBB", re.sub(r"\.Lfunc_\w+", ".L", s)))
    return out


def metadata(path):
    md = {}
    for blk in re.split(r"\n  - \.agpr_count:", open(path).read())[1:]:
        d = dict(re.findall(r"\.(\w+):\s+(\S+)\s*\n", ".agpr_count:" + blk))
        if "name" in d:
            md[d["name"]] = d
    return md


def main():
    parent, new, words = sys.argv[1], sys.argv[2], sys.argv[3:]
    P, N, M = functions(parent), functions(new), metadata(new)
    keys = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")
    for k in sorted(N):
        if not any(w in k for w in words):
            continue
        md = M.get(k)
        reg = " vgpr %s agpr %s sgpr %s vgpr_spills %s sgpr_spills %s scratch_bytes %s" % tuple(md.get(q, "-") for q in keys) if md else ""
        if k in P:
            print("%s instructions parent %d new %d %s%s" % (k, len(P[k]), len(N[k]), "IDENTICAL" if P[k] == N[k] else "DIFFERENT", reg))
        else:
            print("%s instructions new %d (not in the parent)%s" % (k, len(N[k]), reg))
    changed = [k for k in P if k not in N or P[k] != N[k]]
    print("# functions of the parent listing: %d; changed or missing in the new one: %d %s" % (len(P), len(changed), changed[:8]))
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main())
