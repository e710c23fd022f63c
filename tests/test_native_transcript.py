"""CPU: the device transcripts (csrc/transcript.cuh: Keccak-256, BLAKE3 and STROBE-128 / Merlin as streaming PODs, the per-kind
transcript front ends, fs_lagrange_sum and fs_verifier_challenges), compiled for the HOST with g++ against their specification,
host/hashes.hpp and Polymath::verifier_challenges / compute_pi_at_x1 of host/polymath.hpp:

  hashes     Keccak-256 at every length 0 .. 3 * 136 + 2 (the padding's edge cases, which the entry points' message lengths never
             reach); BLAKE3 at 17 lengths around the block, chunk and tree boundaries up to 7 chunks + 1; Merlin with two appends and
             two 64-byte challenges, the first message 0 .. 2 * 166 + 2 bytes long -- each message fed whole and in pieces of
             1, 7, 8, 13 and 64 bytes: (411 + 17 + 335) * 6 = 4578 comparisons
  per curve  3 transcripts x n_inputs in {0, 1, 2, 3, 27, 28, 59, 60} x (3 random cases; inputs of 0 and r - 1 with a_at_x1 = 0 and
             r - 1; a_at_x1 = r and 2^256 - 1 refused): 22 comparisons each = 528; the Lagrange sum alone at x1 = omega^0, omega^m0,
             omega^(2 m0 - 1), omega^(2 m0) and a random point, with the extra inverse (once of 0): 8 x 5 x 2 = 80

The same program is built and run a second time under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone host program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "transcript_selftest.cpp")
WANT = ("hashes: 0 failures of 4578", "bls12_381: 0 failures of 608", "bn254: 0 failures of 608")


@pytest.mark.parametrize("flags", (["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]), ids=("plain", "sanitizers"))
def test_transcript_host_selftest(tmp_path, flags):
    exe = str(tmp_path / "transcript_selftest")
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    for line in WANT:
        assert line in out.stdout.splitlines(), out.stdout
