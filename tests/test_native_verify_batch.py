"""CPU: the batch verifier's device functions (csrc/verify_batch.cuh: verify_term -- one proof's U = rho A + rho x2 C, V = rho D,
W = rho x1 D on the reduced-radix registers -- and verify_tree_add, one node of the sum tree), compiled for the HOST with g++
against the dense double-and-add of Polymath::verify: random subgroup points and scalars, A = +-C, sums that cancel, each point
at infinity, rho = 1 and 2^128 - 1, x1, x2 in {0, 1, r - 1}, trees of 1, 2, 3, 5, 8 terms with a cancelling and a doubling pair;
that double-and-add (ec.cuh: xyzz_mul_words) against repeated addition; verify_weigh and verify_node_points, which the host and the
lanes share, against scalar arithmetic mod r without Montgomery form -- both curves."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_verify_batch_host_selftest(tmp_path):
    exe = str(tmp_path / "verify_batch_selftest")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "native", "verify_batch_selftest.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    # 24 term cases (6 random, 4 with A = +-C, 3 infinities, 2 weights, 9 challenge pairs) and 5 trees, U, V and W each: 87;
    # xyzz_mul_words: 14; verify_weigh: 6 rows; verify_node_points: 5 nodes of three points
    for curve in ("bls12_381", "bn254"):
        assert "%s: 0 failures of 122" % curve in out.stdout.splitlines(), out.stdout
