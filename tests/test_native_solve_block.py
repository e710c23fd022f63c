"""CPU: the witness solver's linear blocks (polymath_amd/host/solve_plan.hpp: linear_row, block_step, KIND_BLOCK; csrc/solve_steps.cuh:
solve_block_invert, solve_block_inverses, solve_block), compiled with g++ from tests/native/solve_block_selftest.cpp.  The accepted
shapes against hand-written plans (k = 2, 3, 7; a row at the point 0 in front of a block of 2l - 2; an empty A side, an empty B side;
a block beside a decomposition, an is-zero pair and a division row; marker bytes 2 - 4 on block columns; a (k + 1)-th row, which is a
check row); 40 products with one matrix and five random systems with five; solve_block_invert on Vandermonde matrices at k = 2, 7, 64
and on a matrix that needs a row swap against literals computed with Python integers, M M^-1 = I computed in the program, and the
pivot column of two equal rows, a zero column and a zero row; a corpus (independent products from the point 1 and from the point 0, a
chain of products, random systems, one block of 64) that in matrix order, reversed and under three seeded permutations plans with
every column at the same level and executes with the host field type, through the routines the kernels call, to the assignment that
schoolbook multiplication gives; the refusals (k - 1 rows, 65 unknowns, an unknown in A_r as well, a boolean-pending column) with the
message they had as a prefix; without the modulus, nothing.  Both curves; once more as a stand-alone program under AddressSanitizer
and UBSan.  The generators of polymath_amd.circuits (LimbProduct, ProductChain, LinearBlocks) are checked on Python integers."""
import os
import subprocess

import pytest

from oracle.pyref.fields import CURVES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "native", "solve_block_selftest.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_solve_block_host_selftest(tmp_path, flags):
    exe = str(tmp_path / "solve_block_selftest")
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-o", exe, SOURCE])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    # shapes 2 x (1 + 2 x 2 + 1 + 2) + 3 x 2 + 2 + 1 + 2; dedupe 2 + 2; invert 4 x 3 + 3 + 1;
    # corpus 4 x (2 + rounds) + 1 + 4 x 5 x 2 x (3 + rounds) with rounds 2, and 2 for the block of 64; refused 5; regression 2
    for curve in ("bls12_381", "bn254"):
        assert "%s: 0 failures of 273" % curve in out.stdout.splitlines(), out.stdout
    # every plan the program builds, error plans with their messages included, folded field by field into one FNV-1a digest per curve
    # (tests/native/solve_selftest.hpp)
    for curve, digest in (("bls12_381", "72c14ac8cf813014"), ("bn254", "b3a7fa431466fd44")):
        assert "%s: 81 plans, digest %s" % (curve, digest) in out.stdout.splitlines(), out.stdout


def _holds(cs):
    r = cs.r
    col = lambda v: cs.instance[v[1]] if v[0] in ("one", "inst") else cs.witness[v[1]]
    dot = lambda lc: sum(coef * col(v) for coef, v in lc) % r
    return all(dot(a) * dot(b) % r == dot(c) for a, b, c in cs.rows)


@pytest.mark.parametrize("curve", ["bls12_381", "bn254"])
def test_generators_on_python_integers(curve):
    """native() against generate_constraints, the rows on the assignment, the layout partial() promises, and Reordered"""
    from polymath_amd import circuits as PC
    from polymath_amd.polymath import ConstraintSystem
    r = CURVES[curve].r
    assert PC.limb_product([3, 4], [5, 6], r) == [15, 38, 24] and PC.limb_product([r - 1, 2], [2, 0], r) == [r - 2, 4, 0]
    g = PC.SplitMix64(16000)
    cases = [(PC.LimbProduct(PC.limb_products(r, 3, 4, 16001)), 3 * (7 + 1) + 1, 3 * 7 + 3),
             (PC.LimbProduct(PC.limb_products(r, 2, 2, 16002), first=0), 2 * (3 + 1) + 1, 2 * 3 + 2),
             (PC.ProductChain([g.fr(r) for _ in range(3)], [g.fr(r) for _ in range(3)], 5), 5 * (5 + 1) + 1, 5 * 5 + 5),
             (PC.LinearBlocks(5, 3, 16003), 3 * (5 + 1) + 1, 3 * 5 + 3)]
    for circuit, rows, unknowns in cases:
        cs = ConstraintSystem(r)
        circuit.generate_constraints(cs)
        assert len(cs.rows) == rows and _holds(cs)
        assert circuit.native(r) == (cs.instance, cs.witness)
        inst, wit = circuit.partial(r)
        assert inst == [1, None] and sum(v is None for v in wit) == unknowns
        assert all(v is None or v == w for v, w in zip(wit, cs.witness))
        for order in ("reverse", 16004):
            shuffled = ConstraintSystem(r)
            PC.Reordered(circuit, order).generate_constraints(shuffled)
            assert _holds(shuffled) and sorted(map(repr, shuffled.rows)) == sorted(map(repr, cs.rows)) and shuffled.rows != cs.rows
            assert PC.Reordered(circuit, order).native(r) == circuit.native(r) and PC.Reordered(circuit, order).partial(r) == (inst, wit)
    # the point 0 writes no zero coefficient: the row is a_0 b_0 = p_0
    cs = ConstraintSystem(r)
    PC.LimbProduct([([3, 4], [5, 6])], first=0).generate_constraints(cs)
    assert [len(lc) for lc in cs.rows[0]] == [1, 1, 1] and [len(lc) for lc in cs.rows[1]] == [2, 2, 3]
    # a drawn matrix is invertible; a singular one is recognised
    assert PC._invertible([[1, 2], [3, 4]], r) and not PC._invertible([[1, 3], [2, 6]], r) and not PC._invertible([[0, 0], [1, 1]], r)
