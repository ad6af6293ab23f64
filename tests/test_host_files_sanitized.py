"""CPU: the host file formats (csrc/srt_host.cpp, csrc/srt_scattered_host.cpp) driven by a stand-alone program with its own
main (tests/native/host_files_main.cpp), built with the address and undefined-behaviour sanitizers: every writer and reader on
small files, every reader on files cut short or spoilt, and the two files whose headers announce far more than they hold -- a
136-byte binary sample file of 2^40 samples, a text grid of 100000^3 nodes with four value lines.  Those two are refused with
the readers' usual words; before the readers looked at the file's size they allocated what the header asked for and took the
calling process down."""
import os
import subprocess

from conftest import ROOT


def test_every_format_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "host_files")
    csrc = os.path.join(ROOT, "stanford_raytracer_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "native", "host_files_main.cpp"), os.path.join(csrc, "srt_host.cpp"),
            os.path.join(csrc, "srt_scattered_host.cpp")]
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                           "-o", exe] + srcs)
    work = tmp_path / "files"
    work.mkdir()
    r = subprocess.run([exe, str(work), "both"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-2000:] + r.stderr[-2000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) >= 249, r.stdout[-500:]
