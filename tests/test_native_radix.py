"""CPU: the radix-5*2^a recoding of the table-mode MSM (csrc/radix.cuh), compiled for the HOST with g++ (the header is plain
C++), against big-integer arithmetic: sum d_j R^j = k, |d_j| <= R/2 and no carry out of the last window for 0, 1, r - 1,
(r - 1)/2, R^j, R^j +- 1, (R/2) R^j +- 1, all-digits R/2 + 1 and R - 1, 2^255 - 19 mod r and 10 000 seeded random scalars, on both
curves and (W, R) in {(12, 5*2^19), (11, 5*2^21), (13, 5*2^18)} plus the small radices of the GPU tests; and the planner's
exactness check on the radices of DESIGN.md section 4.2, with 5*2^18 on 12 windows rejected."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_radix_host_selftest(tmp_path):
    exe = str(tmp_path / "radix_selftest")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "native", "radix_selftest.cpp")])
    out = subprocess.run([exe, "10000"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    for curve in ("bls12_381", "bn254"):
        assert curve + ": 0 failures" in out.stdout, out.stdout
        assert curve + " exactness check: 0 failures" in out.stdout, out.stdout
        for w, a in ((12, 19), (11, 21), (13, 18), (14, 16), (16, 14)):
            line = [l for l in out.stdout.splitlines() if l.startswith("%s recode W=%d R=5*2^%d:" % (curve, w, a))]
            assert len(line) == 1 and " 0 failures of " in line[0], out.stdout
            assert int(line[0].split(" of ")[1].split()[0]) >= 10000 + 4 + 4 * w, out.stdout
