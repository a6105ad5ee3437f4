"""csrc/exact_div.hpp, the correctly rounded quotient from a known reciprocal that the single sweep and the pair route use
for the interior normaliser: tests/shim_exact_div_check.cpp, compiled by the host compiler with -ffp-contract=off, compares
it bit for bit with the division over some millions of numerators -- every divisor within 300 ulps of 1, divisors far from
1, the numerators at either bound of the guard -- and checks that zeros, denormals, infinities and NaN are turned away."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visfd_amd", "csrc")


def _build(tmp_path, extra=()):
    exe = str(tmp_path / "shim_exact_div_check")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas", *extra, "-I", CSRC,
           os.path.join(ROOT, "tests", "shim_exact_div_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_exact_div_has_the_bits_of_the_division(tmp_path):
    r = subprocess.run([_build(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    m = re.search(r"checked (\d+) quotients", r.stdout)
    assert m and int(m.group(1)) > 6_000_000, r.stdout
    assert "mismatch" not in r.stdout
