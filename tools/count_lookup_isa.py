#!/usr/bin/env python3
"""Instruction counts of the interp lookup's species loop (csrc/srt_models.hpp: InterpModel::density_stencil) in compiled ISA.

With one wave per SIMD a launch's time is the sum of the wave's own issue slots, so what the species loop compiles to is counted
here rather than guessed: for every trace_kernel<InterpModel, ...>, rkstep_kernel and gradients_kernel that inlines the lookup,

  * per copy of the species loop (from the loop's label to its back edge; the loop is found by its head wait, vmcnt(24)): the
    body's size, FMA + FMAC, v_cndmask, register moves, writes of M0, s_nop, LDS-DMA instructions, the most M0 writes in front
    of any streamed unit's eight DMA instructions, scratch accesses and vmcnt(0) waits outside the asm statements;
  * per kernel: instructions, code bytes, registers (arch + acc), spilled registers, scratch and LDS bytes.

    python tools/count_lookup_isa.py            # compiles csrc/srt_api.hip for gfx950 with build.py's flags
    python tools/count_lookup_isa.py FILE.s ... # or counts listings made with  hipcc ... -S --cuda-device-only
"""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = re.compile(r"^(_ZN3srt(?:12trace_kernelINS_11InterpModelE|13rkstep_kernelINS_11InterpModelE|"
                     r"16gradients_kernelINS_11InterpModelE)\w+):")


def listing():
    sys.path.insert(0, ROOT)
    from stanford_raytracer_amd import build

    out = os.path.join(tempfile.mkdtemp(prefix="srt_isa_"), "srt_api.s")
    subprocess.check_call([build._hipcc(), "-O3", "--offload-arch=" + build.ARCH, "-std=c++17", "-S", "--cuda-device-only",
                           "-o", out, os.path.join(build.CSRC, "srt_api.hip")])
    return out


def is_ins(line):
    s = line.strip()
    return bool(s) and not s.startswith((";", ".", "#")) and not s.endswith(":")


def demangled(name):
    try:
        return subprocess.run(["c++filt", name], capture_output=True, text=True, check=True).stdout.strip().split("(")[0]
    except (OSError, subprocess.CalledProcessError):
        return name


def metadata(lines):
    """.name -> {key: value} from the amdhsa.kernels notes at the end of the listing"""
    md, cur = {}, {}
    for ln in lines:
        m = re.match(r"\s+(?:- )?\.(\w+):\s+(\S+)\s*$", ln)
        if not m:
            continue
        if ln.lstrip().startswith("- .") and m.group(1) in ("agpr_count", "args") and cur.get("name"):
            cur = {}
        cur[m.group(1)] = m.group(2)
        if m.group(1) == "name":
            md[m.group(2)] = cur
    return md


def loops(lines, st, en):
    """[(first, last)] line ranges of the species-loop bodies of the function in lines[st:en]"""
    pos = {}
    for i in range(st, en):
        m = re.match(r"^(\.LBB\d+_\d+):", lines[i])
        if m:
            pos[m.group(1)] = i
    out = []
    for h in (i for i in range(st, en) if "vmcnt(24)" in lines[i]):
        if out and out[-1][0] <= h <= out[-1][1]:
            continue
        for i in range(h, en):
            m = re.search(r"s_c?branch\S*\s+(\.LBB\d+_\d+)", lines[i])
            if m and pos.get(m.group(1), en) <= h:
                out.append((pos[m.group(1)], i))
                break
    return out


def count_body(lines, a, b):
    c, inasm = collections.Counter(), False
    dma_run, m0_since, worst_m0, units = 0, 0, 0, 0
    for i in range(a, b + 1):
        t = lines[i].strip()
        if t.startswith(";;#ASMSTART"):
            inasm = True
        elif t.startswith(";;#ASMEND"):
            inasm = False
        if not is_ins(lines[i]):
            continue
        op = t.split()[0]
        c["body"] += 1
        c["fma"] += op in ("v_fma_f64", "v_fmac_f64_e32", "v_fmac_f64_e64")
        c["cndmask"] += op.startswith("v_cndmask")
        c["mov"] += op.startswith(("v_mov_b", "v_accvgpr_"))
        c["s_nop"] += op == "s_nop"
        c["scratch"] += op.startswith("scratch_")
        c["own_vmcnt0"] += (not inasm) and op == "s_waitcnt" and "vmcnt(0)" in t
        if re.match(r"s_\w+\s+m0,", t):
            c["m0"] += 1
            m0_since += 1
        if op.startswith("global_load_lds"):
            c["dma"] += 1
            dma_run += 1
            if dma_run == 8:
                worst_m0, units, dma_run, m0_since = max(worst_m0, m0_since), units + 1, 0, 0
    c["units"], c["m0_per_unit"] = units, worst_m0
    return c


def report(path):
    lines = open(path).read().split("\n")
    md = metadata(lines)
    print("== %s" % path)
    print("%-52s %6s %5s %8s %5s %5s %5s %4s %7s %7s %6s" % ("kernel / species-loop body (lines)", "body", "fma", "cndmask", "mov",
                                                             "m0", "nop", "dma", "m0/unit", "scratch", "vmcnt0"))
    found = 0
    for st, ln in enumerate(lines):
        m = KERNELS.match(ln)
        if not m:
            continue
        name = m.group(1)
        en = st
        while not lines[en].startswith(".Lfunc_end"):
            en += 1
        bodies = loops(lines, st, en)
        if not bodies:
            continue
        found += 1
        print(demangled(name))
        for a, b in bodies:
            c = count_body(lines, a, b)
            print("  %-50s %6d %5d %8d %5d %5d %5d %4d %7d %7d %6d" % ("loop %d-%d" % (a + 1, b + 1), c["body"], c["fma"], c["cndmask"],
                                                                      c["mov"], c["m0"], c["s_nop"], c["dma"], c["m0_per_unit"],
                                                                      c["scratch"], c["own_vmcnt0"]))
        info = {}
        for i in range(en, min(en + 80, len(lines))):
            k = re.match(r"; (\w+)\s*[:=]\s*(\d+)", lines[i])
            if k:
                info.setdefault(k.group(1), int(k.group(2)))
        k = md.get(name, {})
        print("  kernel: %d instructions, %d code bytes, registers %d (%d + %d acc), spilled %s vector / %s scalar, scratch %d B, LDS %d B"
              % (sum(is_ins(l) for l in lines[st:en]), info.get("codeLenInByte", -1), info.get("TotalNumVgprs", -1),
                 info.get("NumVgprs", -1), info.get("NumAgprs", -1), k.get("vgpr_spill_count", "?"), k.get("sgpr_spill_count", "?"),
                 info.get("ScratchSize", -1), info.get("LDSByteSize", -1)))
    if not found:
        raise SystemExit("no species loop found: is this the listing of srt_api.hip?")


def main():
    for path in (sys.argv[1:] or [listing()]):
        report(path)


if __name__ == "__main__":
    main()
