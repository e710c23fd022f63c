"""CPU: the witness solver's Euclidean division rows (polymath_amd/host/solve_plan.hpp: division_row, KIND_DIVREM; csrc/divrem.cuh:
marker_byte, divrem256, euclid_divrem), compiled with g++ into tests/native/solve_divrem_selftest.cpp.  The accepted shapes against
hand-written plans (q in A and in B, cq = 1 and 7 with cr = -cq, with and without a known rest; chain and wide launch); every refusal
at its row with the row's earlier message as a prefix (cr != -cq, rem in A or B, rem named twice, the other side not known, the
quotient named twice, a third unknown), in matrix order and in any order; a byte-2 column solved by an ordinary row, named as a
pair's flag, and as a bit; two assignments that mark one column with different markers; a division row beside an is-zero pair over
the same known side (no opener is registered, the pair still closes, d = 0 sticks the division only); a corpus -- 40 range-checked
divisions in one wide level, a 12-step modular chain, a mixed system -- that in matrix order is build_plan field by field and,
reversed and under three seeded permutations, plans with every column at its level and executes with the host field type, through
the routine the kernels call, to the same assignment; a ready division row releasing an opener registered over its remainder; and
the edge operands (d = 1, r - 1, 2^64, 2^192 + 1 against a = 0, d - 1, d, r - 1, random sizes, d = 0 stuck) against divmod literals.
Both curves; once more as a stand-alone program under AddressSanitizer and UBSan."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "native", "solve_divrem_selftest.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_solve_divrem_host_selftest(tmp_path, flags):
    exe = str(tmp_path / "solve_divrem_selftest")
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-o", exe, SOURCE])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    # shapes 8 x (2 x 3 + 1); refusals 10 x 4; marker elsewhere 4; mixed markers 5; beside pairs 5;
    # corpus 3 x (2 x 2 + 1 or 0 + rounds + 4 x 2 x (4 + rounds)) with rounds 2, 2, 2, + 2; edges 1 + 18 + 2
    for curve in ("bls12_381", "bn254"):
        assert "%s: 0 failures of 297" % curve in out.stdout.splitlines(), out.stdout
    # every plan the program builds, error plans with their messages included, folded field by field into one FNV-1a digest per curve
    # (tests/native/solve_selftest.hpp); recorded from the planner as it stood before its rules were stated once
    for curve, digest in (("bls12_381", "15edcd0305e2ab0f"), ("bn254", "2b08190d2b3575d7")):
        assert "%s: 131 plans, digest %s" % (curve, digest) in out.stdout.splitlines(), out.stdout
