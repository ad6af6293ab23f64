#!/usr/bin/env python3
"""ISA check of the interp lookup's read-ahead (csrc/srt_models.hpp: read_unit_issue / wait_lgkm in density_stencil).

read_unit_issue is an asm statement of eight ds_read_b128 WITHOUT a wait; the wait that releases them (wait_lgkm) is a later
statement.  In between the compiler takes the eight destination registers for written.  The source cannot forbid it to copy,
spill or move one of them to an accumulator register inside that window (it would save stale data), nor to put an access of its
own that it then waits for with lgkmcnt(0) there (which would undo the overlap).  So the compiled code is checked instead, in
every function that holds such reads (the six trace_kernel<InterpModel, ...>, rkstep_kernel and gradients_kernel): from a unit's
first read to the s_waitcnt lgkmcnt inside an asm statement that releases it,

  * no instruction outside the asm statements names a register whose read is still in flight,
  * no scalar load, no LDS access and no s_waitcnt of the compiler's own sits in the window.

The scan is linear over the listing, through both arms of the wave-uniform branches in the window (is another species to be
staged?): conservative.  Run it again after a change of compiler, of build flags or of the lookup's register pressure:

    python tools/check_read_ahead_isa.py            # compiles csrc/srt_api.hip for gfx950 with build.py's flags (about 2 min)
    python tools/check_read_ahead_isa.py FILE.s     # or checks a listing made with  hipcc ... -S --cuda-device-only
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def listing():
    sys.path.insert(0, ROOT)
    from stanford_raytracer_amd import build

    out = os.path.join(tempfile.mkdtemp(prefix="srt_isa_"), "srt_api.s")
    subprocess.check_call([build._hipcc(), "-O3", "--offload-arch=" + build.ARCH, "-std=c++17", "-S", "--cuda-device-only",
                           "-o", out, os.path.join(build.CSRC, "srt_api.hip")])
    return out


def regs(tok):
    m = re.match(r"v\[(\d+):(\d+)\]", tok)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r"v(\d+)$", tok)
    return {int(m.group(1))} if m else set()


def check(lines):
    """-> (windows per function, problems)"""
    windows, problems, func = {}, [], "?"
    i, in_stmt = 0, False
    while i < len(lines):
        t = lines[i].strip()
        m = re.match(r"^(_Z\w+):", lines[i])
        if m:
            func = m.group(1)
        if t.startswith(";;#ASM"):
            in_stmt = t.startswith(";;#ASMSTART")
        # (the compiler's own LDS reads carry its own waits; the scattered model's asm reads are another pattern, not this one)
        if not (in_stmt and t.startswith("ds_read_b128") and "InterpModel" in func):
            i += 1
            continue
        pending, j = [], i
        while lines[j].strip().startswith("ds_read_b128"):
            pending.append(regs(lines[j].split()[1].rstrip(",")))
            j += 1
        if "lgkmcnt" in lines[j]:  # read_unit: the wait is part of the same statement
            i = j + 1
            continue
        windows[func] = windows.get(func, 0) + 1
        inasm, k = True, j
        while pending:
            t = lines[k].strip()
            if t.startswith(";;#ASMSTART"):
                inasm = True
            elif t.startswith(";;#ASMEND"):
                inasm = False
            elif t.startswith(".end_amdhsa_kernel") or k + 1 >= len(lines):
                problems.append("%s: line %d: reads never released" % (func, i + 1))
                break
            elif t and not t.startswith((";", ".")) and not t.endswith(":"):
                w = re.match(r"s_waitcnt lgkmcnt\((\d+)\)$", t)
                if inasm and t.startswith("ds_read_b128"):
                    pending.append(regs(t.split()[1].rstrip(",")))
                elif inasm and w:
                    n = int(w.group(1))
                    pending = pending[len(pending) - n:] if n else []
                elif not inasm:
                    if re.match(r"(s_load|s_buffer_load|ds_|s_waitcnt)", t):
                        problems.append("%s: line %d: in a read window: %s" % (func, k + 1, t))
                    used = set()
                    for tok in re.findall(r"v\[\d+:\d+\]|\bv\d+\b", t):
                        used |= regs(tok)
                    if any(used & p for p in pending):
                        problems.append("%s: line %d: names a register whose read is in flight: %s" % (func, k + 1, t))
            k += 1
        i, in_stmt = k + 1, True  # the releasing wait sits inside a statement
    return windows, problems


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else listing()
    windows, problems = check(open(path).read().split("\n"))
    for f in sorted(windows):
        print("%3d read-ahead windows  %s" % (windows[f], f))
    for p in problems:
        print("PROBLEM", p)
    if not windows:
        raise SystemExit("no read-ahead reads found: is this the listing of srt_api.hip?")
    print("%d functions, %d windows, %d problems" % (len(windows), sum(windows.values()), len(problems)))
    raise SystemExit(1 if problems else 0)


if __name__ == "__main__":
    main()
