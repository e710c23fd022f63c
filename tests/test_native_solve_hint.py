"""CPU: the witness solver's declared long-division hints (polymath_amd/host/solve_plan.hpp: decode_hints, hint_step, the hint-owned
columns of the scheduler, KIND_LONGDIV; csrc/solve_steps.cuh: add_shifted, limb_at, longdiv, solve_longdiv -- the text the kernel
k_solve_longdiv calls), compiled with g++ from tests/native/solve_hint_selftest.cpp.  Long divisions against literals computed with
Python integers (solve_hint_cases.hpp, which tools/gen_solve_hint_cases.py writes into the test's directory before the program is built: D = 0, D < E, E = 1, D = 2^1024 - 1,
E = 2^512 - 1, D = E, n = 1, 32, 64, 86, 128, limbs that carry across several limbs, a limb equal to r - 1, literal divisors, the five
stuck conditions at their boundary and one below); every refusal of the declaration and of the planner with its text; an inert hint,
whose plan is the plan without the declaration; a hint that waits for a block and wakes decompositions; rows in order, reversed and
shuffled; LimbModMul and ModMulChain executed to (a b) mod p.  Both curves; once more as a stand-alone program under AddressSanitizer
and UBSan.  The generators of polymath_amd.circuits are checked on Python integers."""
import os
import subprocess
import sys

import pytest

from oracle.pyref.fields import CURVES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "native", "solve_hint_selftest.cpp")
SECP = 2 ** 256 - 2 ** 32 - 977
P381 = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_solve_hint_host_selftest(tmp_path, flags):
    exe = str(tmp_path / "solve_hint_selftest")
    cases = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_solve_hint_cases.py")], capture_output=True, text=True, check=True).stdout
    (tmp_path / "solve_hint_cases.hpp").write_text(cases)          # the program's literals: Python's divmod, written fresh
    subprocess.check_call(["g++", "-std=c++17", "-I", str(tmp_path)] + flags + ["-o", exe, SOURCE])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    # 36 divisions x 4; 46 refusals; 12 circuits x 6 and 2 more for the first; 3 for the stuck word; 2 for the mixed launch
    for curve in ("bls12_381", "bn254"):
        assert "%s: 0 failures of 272" % curve in out.stdout.splitlines(), out.stdout


def _holds(cs):
    r = cs.r
    col = lambda v: cs.instance[v[1]] if v[0] in ("one", "inst") else cs.witness[v[1]]
    dot = lambda lc: sum(coef * col(v) for coef, v in lc) % r
    return all(dot(a) * dot(b) % r == dot(c) for a, b, c in cs.rows)


@pytest.mark.parametrize("curve", ["bls12_381", "bn254"])
def test_generators_on_python_integers(curve):
    """native() against generate_constraints, the rows on the assignment, what partial() leaves to the device, hints() against
    Python's divmod on the assignment's columns, and Reordered"""
    from polymath_amd import api, circuits as PC
    from polymath_amd.polymath import ConstraintSystem
    r = CURVES[curve].r
    small = [(a % (1 << 380), b % (1 << 380)) for a, b in PC.modmul_pairs(P381, 2, 18002)]
    small = [(sum(((a >> (128 * i)) & ((1 << 124) - 1)) << (128 * i) for i in range(3)), sum(((b >> (128 * i)) & ((1 << 124) - 1)) << (128 * i) for i in range(3))) for a, b in small]
    cases = [(PC.LimbModMul(PC.modmul_pairs(SECP, 3, 18000), SECP, 64, 4), 3, 4, 64),
             (PC.LimbModMul(PC.modmul_pairs(SECP, 2, 18001), SECP, 86, 3), 2, 3, 86),
             (PC.LimbModMul(small, P381, 128, 4), 2, 4, 128),
             (PC.LimbModMul(PC.modmul_pairs(SECP, 2, 18003), SECP, 86, 3, decompose=False), 2, 3, 86),
             (PC.ModMulChain(12345678901234567890123, 98765432109876543210987654321, SECP, 64, 4, 3), 3, 4, 64),
             (PC.ModMulChain(12345678901234567890123, 98765432109876543210987654321, SECP, 64, 4, 3, witness_modulus=True), 3, 4, 64)]
    for circuit, count, l, n in cases:
        cs = ConstraintSystem(r)
        circuit.generate_constraints(cs)
        assert _holds(cs) and circuit.native(r) == (cs.instance, cs.witness)
        inst, wit = circuit.partial(r)
        given = (2 * l * count) if isinstance(circuit, PC.LimbModMul) else (3 * l if circuit.witness_modulus else 2 * l)
        assert inst == [1, None] and sum(v is not None for v in wit) == given and all(v is None or v == w for v, w in zip(wit, cs.witness))
        m0 = len(cs.instance)
        hints = circuit.hints(m0)
        assert len(hints) == count
        z = cs.instance + cs.witness
        for hint in hints:
            assert hint["n"] == n and wit[hint["q"][0] - m0] is None and wit[hint["rem"][-1] - m0] is None
            dividend = sum(z[c] << (n * j) for j, c in enumerate(hint["D"]))
            divisor = PC.limbs_int(hint["literal"], n) if "literal" in hint else sum(z[c] << (n * j) for j, c in enumerate(hint["E"]))
            assert divisor == circuit.modulus
            q, rem = divmod(dividend, divisor)
            assert PC.int_limbs(q, n, l) == [z[c] for c in hint["q"]] and PC.int_limbs(rem, n, l) == [z[c] for c in hint["rem"]]
        assert api.decode_hints(api.encode_hints(hints)) == hints
        for order in ("reverse", 18004):
            shuffled = ConstraintSystem(r)
            PC.Reordered(circuit, order).generate_constraints(shuffled)
            assert _holds(shuffled) and sorted(map(repr, shuffled.rows)) == sorted(map(repr, cs.rows)) and shuffled.rows != cs.rows
    # LimbModMul: the remainders are (a b) mod p and the public input their limbs' sum
    pairs = PC.modmul_pairs(SECP, 3, 18000)
    inst, wit = PC.LimbModMul(pairs, SECP, 64, 4).native(r)
    per = len(wit) // 3
    rems = [PC.limbs_int(wit[i * per + 8 + 7 + 4:i * per + 8 + 7 + 8], 64) for i in range(3)]
    assert rems == [a * b % SECP for a, b in pairs] and inst == [1, sum(sum(PC.int_limbs(v, 64, 4)) for v in rems) % r]
    # a product limb that would reach r is refused by the generator: the hint's dividend would not be a b
    with pytest.raises(AssertionError):
        PC.LimbModMul([((1 << 512) - 1, (1 << 512) - 1)], P381, 128, 4).native(r)
