"""CPU: the witness solver's plan builder (polymath_amd/host/solve_plan.hpp, header-only, no HIP), compiled with g++ into
tests/native/solve_plan_selftest.cpp: a 3-round MiMC-shaped system, one-level diagonals on both sides of the width threshold, a
random-gate system under three thresholds and a hand-built system with unknowns in A and in B -- step lists, kinds, levels, level_ptr
and the launch schedule against hand-written expectations; every structural error with its row or column; a zero coefficient that
names no variable; and each plan executed serially with the host field type against direct evaluation, stuck rows included --
both curves."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_solve_plan_host_selftest(tmp_path):
    exe = str(tmp_path / "solve_plan_selftest")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "native", "solve_plan_selftest.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    # mimc3 6, diagonal 4 x 3, random gates 3 x 4, kinds 8, errors 8
    for curve in ("bls12_381", "bn254"):
        assert "%s: 0 failures of 46" % curve in out.stdout.splitlines(), out.stdout
    # every plan the program builds, error plans with their messages included, folded field by field into one FNV-1a digest per curve
    # (tests/native/solve_selftest.hpp); recorded from the planner as it stood before its rules were stated once
    for curve, digest in (("bls12_381", "52d217478e3503b8"), ("bn254", "039a04815ec996e7")):
        assert "%s: 16 plans, digest %s" % (curve, digest) in out.stdout.splitlines(), out.stdout
