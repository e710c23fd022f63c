"""CPU: the witness solver's any-order plan builder (polymath_amd/host/solve_plan.hpp: build_plan_any_order and its waiting-row
scheduler), compiled with g++ into tests/native/solve_order_selftest.cpp.  In matrix order the new builder is build_plan field by
field (a chain of all three kinds, one wide level, decompositions in C, A and B, is-zero pairs in both forms at two levels, a mixed
system; wide and narrow launch thresholds).  The same systems reversed and under five seeded row permutations (a pair's rows keep
their relative order) plan, reordered exactly where build_plan refuses, with every column at its in-order level, the steps sorted
by (level, kind, row), and execute with the host field type to the in-order assignment, pairs with d != 0 and d = 0.  The waiting
cases by hand: booleanity rows after their decomposition, a row that names a multiplier before the closer, a * a = e before the row
that determines a, an opener-shaped ordinary row released by the row that determines its multiplier.  Refused with build_plan's
code, row, column and message as a prefix: two unknowns no order separates, an unclosed opener, a mismatched closer, k + 1 bits, an
undetermined column, column 0 (as it is).  The stuck key (level, row) names row 1 where the smaller row 0 is the consequence.  A
dependency chain of 2^18 rows stored in reverse plans within 50 x the in-order time (a sweep per level is over 10^4 x).  Both
curves; once more as a stand-alone program under AddressSanitizer and UBSan."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "native", "solve_order_selftest.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_solve_order_host_selftest(tmp_path, flags):
    exe = str(tmp_path / "solve_order_selftest")
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-o", exe, SOURCE])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    # corpus 6 x (2 x 2 + rounds + 6 x 2 x (5 + rounds)) with rounds 1, 1, 3, 4, 4, 2; waiting 3 + 4 + 3 + 2; refused 4 + 2 x 2 + 2; root cause 5; blow-up 2
    for curve in ("bls12_381", "bn254"):
        assert "%s: 0 failures of 608" % curve in out.stdout.splitlines(), out.stdout
        times = re.search(r"^%s: chain of 2\^18 rows: build_plan in order ([0-9.]+) ms, build_plan_any_order reversed ([0-9.]+) ms" % curve, out.stdout, flags=re.M)
        assert times and float(times.group(2)) <= 50 * float(times.group(1)), out.stdout
    # every plan the program builds, error plans with their messages included, folded field by field into one FNV-1a digest per curve
    # (tests/native/solve_selftest.hpp); recorded from the planner as it stood before its rules were stated once
    for curve, digest in (("bls12_381", "4977861ae1ae1509"), ("bn254", "e410dff4f49be2be")):
        assert "%s: 199 plans, digest %s" % (curve, digest) in out.stdout.splitlines(), out.stdout
