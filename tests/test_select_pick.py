"""The digit pick of the radix select (visfd_amd/csrc/select_pick.hpp) as host code: tests/select_pick_check.cpp, compiled by the
host compiler, walks hand-made histograms -- the cut in the top bin, in the bottom bin, all mass in one bin, k on every bin
boundary, 64-bit counts above 2^32 -- and compares bin and remainder with a sorted array; the pick kernel's two-level walk is
compared with the flat one, and the rank floor((float)n * fraction) with the single-precision product.  The same function
runs in the host select, in the slab select and in the kernel that picks the digit on the device."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visfd_amd", "csrc")


def test_pick_matches_a_sorted_array(tmp_path):
    exe = str(tmp_path / "select_pick_check")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(ROOT, "tests", "select_pick_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    m = re.search(r"checked (\d+) facts, 0 mismatches", r.stdout)
    assert m and int(m.group(1)) > 10000, r.stdout
