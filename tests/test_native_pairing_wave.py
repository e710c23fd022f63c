"""CPU: the wave-cooperative pairing's decomposition (csrc/pairing_wave.cuh), compiled for the HOST with g++ and run lane after lane,
both curves: 36 products and their collection against mul12 and sqr12, 18 products against mul_line, the coefficient-wise Frobenius
against frob12, the conjugate; operands random and 0, 1, -1, a lone coefficient in each position (all 36 pairs of positions), lines
with a zero coefficient, a pair at infinity (the line 1); the fixed-base table sum against xyzz_mul_words for 0, 1, r - 1, a single
digit in the lowest and the highest window, equal digits in one lane's two windows and random words, and G = O.  Run plain and as the
same stand-alone program under AddressSanitizer and UBSan."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "pairing_wave_selftest.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_pairing_wave_host_selftest(tmp_path, flags):
    exe = str(tmp_path / "pairing_wave_selftest")
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    # per curve: 5 checks for each of 10 + 36 + 6 pairs of ring operands, 16 line cases, 1 infinity, 12 "== 1", 14 scalars, G = O
    for curve in ("bls12_381", "bn254"):
        assert "%s: 0 failures of 304" % curve in out.stdout.splitlines(), out.stdout


def test_the_kernel_calls_the_text_the_host_ran():
    """the seam is one text: every piece the self-test runs is what the kernel calls, and the kernel carries no second copy"""
    hip = open(os.path.join(ROOT, "polymath_amd", "csrc", "pairing_wave.hip")).read()
    for piece in ("W::product(", "W::collect(", "W::line_coeff(", "W::frob_coeff(", "W::conj_coeff(", "W::is_one_coeff(", "W::fixed_base_lane(",
                  "W::fixed_base_tree_step(", "WaveTower<C>::fixed_base_build("):
        assert piece in hip and piece.split("::")[1] in open(SRC).read(), piece
    assert "asm" not in hip and "mul_xi" not in hip and "gamma[" not in hip
