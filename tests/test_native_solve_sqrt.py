"""CPU: the witness solver's square-root rows (polymath_amd/host/solve_plan.hpp: sqrt_row, KIND_SQRT; csrc/sqrt.cuh: fr_sqrt;
csrc/divrem.cuh: marker_byte), compiled with g++ from tests/native/solve_sqrt_selftest.cpp.  The accepted shapes against hand-written
plans (ka, kb in {1, 7, -1}; C_r empty, a constant, a combination of two signals; a stored zero coefficient in front of u in A_r or
in B_r; chain and wide launch, both dividing); byte 4 elsewhere (an ordinary row, beside a second unknown, a rest beside u, u in C_r,
a bit of a decomposition, a pair's flag or multiplier, a quotient's position), where every plan is the plain marker's; marker_byte on
the four markers, the near-misses that were and the new ones (bit 192 clear with bit 0 or bit 64 clear, bit 193 clear); fr_sqrt on
0, 1, 4, r - 1, the generator (a non-residue) and one operand per iteration of its loop nest against literals computed with Python
integers, and both roots' squares giving the one small root; a corpus -- a level of 40 square roots, the decompression of three
Edwards points, a system that mixes a square root with a division and an is-zero pair -- that in matrix order is build_plan field by
field and, reversed and under three seeded permutations, plans with every column at its level and executes with the host field type,
through the routines the kernels call, to the same assignment; the same corpus with the plain marker, refused in the words it always
had; a square-root row that waits for its C side, and one that releases an opener registered over its root; a non-residue stuck at
its own row, and reported as the root cause under a reordered plan.  Both curves; once more as a stand-alone program under
AddressSanitizer and UBSan."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "native", "solve_sqrt_selftest.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_solve_sqrt_host_selftest(tmp_path, flags):
    exe = str(tmp_path / "solve_sqrt_selftest")
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-o", exe, SOURCE])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    # shapes 81 x (2 x 3 + 1) + 1; marker elsewhere 10 x 2 + 3; markers 6; roots 1 + 2 x (5 + s + 1) + 16 with s = 32 / 28;
    # corpus 3 x (2 x 2 + 1 + rounds + 1 + 2 + 4 x 2 x (4 + rounds)) with rounds 2; waiting root 5; stuck 4
    for curve, checks in (("bls12_381", 873), ("bn254", 865)):
        assert "%s: 0 failures of %d" % (curve, checks) in out.stdout.splitlines(), out.stdout
    # every plan the program builds, error plans with their messages included, folded field by field into one FNV-1a digest per curve
    # (tests/native/solve_selftest.hpp)
    for curve, digest in (("bls12_381", "2bebd688a48c0352"), ("bn254", "8ccdf5a8c45a5b11")):
        assert "%s: 501 plans, digest %s" % (curve, digest) in out.stdout.splitlines(), out.stdout
