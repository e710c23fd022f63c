"""CPU: the witness solver's indicator rows (polymath_amd/host/solve_plan.hpp: indicator_row, KIND_INDICATOR; csrc/divrem.cuh:
marker_byte, indicator_of), compiled with g++ into tests/native/solve_indicator_selftest.cpp.  The accepted shapes against
hand-written plans (u in A and in B, k = 1 and 7, the guards inp - i, i - inp and a - b between two signals; chain and wide launch,
neither dividing); byte 3 elsewhere (an ordinary row -- C_r not empty, a rest beside u, an empty other side --, beside a second
unknown, as a bit of a decomposition, as a pair's flag), where every plan is the plain marker's; two assignments that mark one column
with different markers, and marker_byte on the three markers and their near-misses (both bits clear, a cleared top bit, ...fffffffc);
a corpus -- a width-40 decoder, a table walk, a system that mixes indicators with a division and an is-zero pair -- that in matrix
order is build_plan field by field and, reversed and under three seeded permutations, plans with every column at its level and
executes with the host field type, through the routine the kernels call, to the same assignment; the same corpus with the plain
marker, which plans as it always did and sticks at the hit row; a guard row that waits for its index; and a guard that releases an
opener registered over its indicator.  Both curves; once more as a stand-alone program under AddressSanitizer and UBSan."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "native", "solve_indicator_selftest.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_solve_indicator_host_selftest(tmp_path, flags):
    exe = str(tmp_path / "solve_indicator_selftest")
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-o", exe, SOURCE])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    # shapes 12 x (2 x 4 + 1); marker elsewhere 6 + 1, 5, 1, 1; markers 9;
    # corpus 3 x (2 x 2 + 1 + rounds + 1 + 1 + rounds + 4 x 2 x (4 + rounds)) with rounds 3, 2, 2; waiting guard 6
    for curve in ("bls12_381", "bn254"):
        assert "%s: 0 failures of 324" % curve in out.stdout.splitlines(), out.stdout
    # every plan the program builds, error plans with their messages included, folded field by field into one FNV-1a digest per curve
    # (tests/native/solve_selftest.hpp); recorded from the planner as it stood before its rules were stated once
    for curve, digest in (("bls12_381", "20a758e1ba1931e3"), ("bn254", "a5498f6e2cbf9e25")):
        assert "%s: 136 plans, digest %s" % (curve, digest) in out.stdout.splitlines(), out.stdout
