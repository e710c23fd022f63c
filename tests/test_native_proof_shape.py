"""CPU: the one host-side description of a proof's shape (csrc/prove_common.cuh: proof_shape -- Lz, len_a, len_c, num_len, len_d and
the division scan's level plan) and the flag-word-to-status functions both provers use, compiled for the host only into
tests/native/proof_shape_selftest.cpp: n = 4 (one lane divides), 8 (one chunked level of 7), 128 (82 and 6) and 2^20 (five levels)
against hand-computed values, and all sixteen flag words."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_proof_shape_host_selftest(tmp_path):
    exe = str(tmp_path / "proof_shape_selftest")
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-host-only", "-O1", "-std=c++17", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "proof_shape_selftest.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    # 4 shapes (9 + 2 * levels checks each: levels 0, 1, 2, 5), 16 flag words for two phases, the unread bits
    assert "proof_shape: 0 failures of 85" in out.stdout.splitlines(), out.stdout
