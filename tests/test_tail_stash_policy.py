"""CPU: the policy functions of the tail stash (csrc/srt_tail_stash.hpp) swept by a stand-alone program with its own main
(tests/native/tail_stash_policy_main.cpp), built with the address and undefined-behaviour sanitizers: the marks and quotas of
a launch, which mark a step count stands on, and the pick -- never from an empty level, always emptying the stash, the
largest remainder that fits before the wave's expected end, else the smallest."""
import os
import subprocess

from conftest import ROOT


def test_policy_sweep(tmp_path):
    exe = str(tmp_path / "tail_stash_policy")
    src = os.path.join(ROOT, "tests", "native", "tail_stash_policy_main.cpp")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) > 100000, r.stdout[-500:]
