"""CPU: the witness solver's plan builder with the field's modulus (polymath_amd/host/solve_plan.hpp: booleanity rows and bit
decompositions), compiled with g++ into tests/native/solve_bits_selftest.cpp.  Accepted: kinds A, B and C, c != 1, permuted
exponents, known entries beside the bits, a boolean-pending column that an ordinary row solves, a decomposition at a later level,
k = bitlength(r) - 1 -- step, columns in exponent order, level and launch against hand-written expectations, and each plan executed
serially with the host field type over marker words, stuck rows (T >= 2^k, a zero divisor) included.  Refused, with row or column:
booleanity after the decomposition, a gap, a repeated coefficient, an unknown that is not boolean-pending, a bit in a second matrix,
k = bitlength(r), a boolean column nothing determines, every other shape of one unknown in two matrices.  Without the modulus the
builder gives the earlier errors and plans.  Both curves; once more as a stand-alone program under AddressSanitizer and UBSan."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "native", "solve_bits_selftest.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_solve_bits_host_selftest(tmp_path, flags):
    exe = str(tmp_path / "solve_bits_selftest")
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-o", exe, SOURCE])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    # accepted 12 + 4 x 2 + 3, widest 4, refused 1 + 3 + 1 + 2 + 1 + 2 + 6 + 1, equivalence 2 + 2 + 2 + 2
    for curve in ("bls12_381", "bn254"):
        assert "%s: 0 failures of 52" % curve in out.stdout.splitlines(), out.stdout
    # every plan the program builds, error plans with their messages included, folded field by field into one FNV-1a digest per curve
    # (tests/native/solve_selftest.hpp); recorded from the planner as it stood before its rules were stated once
    for curve, digest in (("bls12_381", "ccb5d308250dc75c"), ("bn254", "dfd81707c06e053c")):
        assert "%s: 34 plans, digest %s" % (curve, digest) in out.stdout.splitlines(), out.stdout
