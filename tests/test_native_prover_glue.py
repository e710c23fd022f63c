"""CPU: the batch prover's device glue (csrc/transcript.cuh: fs_prover_x1 / fs_prover_x2; csrc/g1_record.cuh: g1_record_words;
csrc/batch_row.cuh: fill_batch_row), compiled for the HOST with g++ against its specification, Polymath::glue_x1 / glue_x2,
compute_pi_at_x1, ser_g1 and Proof::to_bytes of host/polymath.hpp, word for word:

  per curve  3 transcripts x m0 in {1, 2, 3, 7, 8, 9, 12, 20} (2 m0 straddles FS_INV_CHUNK at 8) x 6 cases -- a well-formed instance,
             a random element 0, [a]_1 at infinity, [c]_1 at infinity, r_a = (0, 0), x1 moved onto the domain element omega^m0 --
             x 5 comparisons: the three compressed records; x1, y1^alpha, y1^gamma; a(x1), pi(x1), c(x1), x2; the assembled proof
             bytes; the phase-3 BatchRow record (numerator constants, reduced-radix multipliers, level powers) = 720

The same program is built and run a second time under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone host program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "prover_glue_selftest.cpp")
WANT = ("bls12_381: 0 failures of 720", "bn254: 0 failures of 720")


@pytest.mark.parametrize("flags", (["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]), ids=("plain", "sanitizers"))
def test_prover_glue_host_selftest(tmp_path, flags):
    exe = str(tmp_path / "prover_glue_selftest")
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    for line in WANT:
        assert line in out.stdout.splitlines(), out.stdout
