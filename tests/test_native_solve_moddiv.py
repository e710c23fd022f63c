"""CPU: the witness solver's declared modular-division hints (polymath_amd/host/solve_plan.hpp: decode_hints' opcode 3, KIND_MODDIV,
LAUNCH_MODDIV; csrc/solve_steps.cuh: modinv_odd, solve_moddiv -- the text the kernel k_solve_moddiv calls), compiled with g++ from
tests/native/solve_moddiv_selftest.cpp.  Modular divisions against literals computed with Python's pow(D, -1, P)
(solve_moddiv_cases.hpp, which tools/gen_solve_moddiv_cases.py writes into the test's directory before the program is built): P =
secp256k1's prime, BLS12-381's q, 2^512 - 1, 3 and a composite; D = 1, P - 1, (P +- 1) / 2, 2^(L - 1), 0, P, a shared factor, limbs
that carry, D+ < D-, N = 1; every stuck condition at its boundary; every refusal with its text; both opcodes in one declaration; the
levels and launches where the two opcodes meet; a chain in order, reversed and shuffled.  Both curves; once more as a stand-alone
program under AddressSanitizer and UBSan.  The generators of polymath_amd.circuits are checked on Python integers."""
import os
import subprocess
import sys

import pytest

from oracle.pyref.fields import CURVES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "native", "solve_moddiv_selftest.cpp")
SECP = 2 ** 256 - 2 ** 32 - 977
G = (0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798, 0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8)


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_solve_moddiv_host_selftest(tmp_path, flags):
    exe = str(tmp_path / "solve_moddiv_selftest")
    cases = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_solve_moddiv_cases.py")], capture_output=True, text=True, check=True).stdout
    (tmp_path / "solve_moddiv_cases.hpp").write_text(cases)          # the program's literals: Python's pow, written fresh
    subprocess.check_call(["g++", "-std=c++17", "-I", str(tmp_path)] + flags + ["-o", exe, SOURCE])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    # 97 divisions x 4; 70 more: the declaration and the planner, the meeting opcodes, the chain, the stuck word, the mixed launch
    for curve in ("bls12_381", "bn254"):
        assert "%s: 0 failures of 458" % curve in out.stdout.splitlines(), out.stdout
    for worst in ("D = 2^(L - 1), the bound's worst case of halvings", "D = P - 1", "D = (P + 1) / 2", "D = (P - 1) / 2"):
        assert worst in cases          # the trip-count bound's worst cases are in the table by name


def _holds(cs):
    r = cs.r
    col = lambda v: cs.instance[v[1]] if v[0] in ("one", "inst") else cs.witness[v[1]]
    dot = lambda lc: sum(coef * col(v) for coef, v in lc) % r
    return all(dot(a) * dot(b) % r == dot(c) for a, b, c in cs.rows)


def _ec_add(p1, p2):
    """affine addition or doubling on secp256k1, Python integers"""
    (x1, y1), (x2, y2) = p1, p2
    lam = (3 * x1 * x1) * pow(2 * y1, -1, SECP) % SECP if p1 == p2 else (y2 - y1) * pow(x2 - x1, -1, SECP) % SECP
    x3 = (lam * lam - x1 - x2) % SECP
    return x3, (lam * (x1 - x3) - y1) % SECP


@pytest.mark.parametrize("curve", ["bls12_381", "bn254"])
def test_generators_on_python_integers(curve):
    """native() against generate_constraints, the rows on the assignment, what partial() leaves to the device, hints() against Python's
    pow and divmod on the assignment's columns, and Reordered"""
    from polymath_amd import api, circuits as PC
    from polymath_amd.polymath import ConstraintSystem
    r = CURVES[curve].r
    narrow = PC.narrow_modulus(128, 4, 120)
    G2 = _ec_add(G, G)
    G3 = _ec_add(G2, G)
    cases = [(PC.LimbModDiv(PC.moddiv_cases(SECP, 3, 20000, inverses=1), SECP, 64, 4), 64, 4, 10 * 4),
             (PC.LimbModDiv(PC.moddiv_cases(SECP, 2, 20001), SECP, 86, 3), 86, 3, 8 * 3),
             (PC.LimbModDiv(PC.moddiv_cases(narrow, 2, 20002, inverses=1, narrow=(128, 4, 120)), narrow, 128, 4, operand_bits=120), 128, 4, 6 * 4),
             (PC.LimbModDiv(PC.moddiv_cases(65521 * 65519, 4, 20003, inverses=2), 65521 * 65519, 16, 2, decompose=False), 16, 2, 12 * 2),
             (PC.EcAddChain(G3, G2, SECP, 64, 4, 2), 64, 4, 4 * 4)]
    for circuit, n, l, given in cases:
        cs = ConstraintSystem(r)
        circuit.generate_constraints(cs)
        assert _holds(cs) and circuit.native(r) == (cs.instance, cs.witness)
        inst, wit = circuit.partial(r)
        assert inst == [1, None] and sum(v is not None for v in wit) == given and all(v is None or v == w for v, w in zip(wit, cs.witness))
        m0 = len(cs.instance)
        hints = circuit.hints(m0)
        z = cs.instance + cs.witness
        value = lambda cols: sum(z[c] << (n * j) for j, c in enumerate(cols))
        for hint in hints:
            assert hint["n"] == n and PC.limbs_int(hint["literal"], n) == circuit.modulus
            if hint.get("op") == "moddiv":
                assert all(wit[c - m0] is None for c in hint["z"])
                N = (value(hint["Np"]) - value(hint["Nm"])) % circuit.modulus if hint["Np"] or hint["Nm"] else 1
                assert value(hint["z"]) == N * pow(value(hint["Dp"]) - value(hint["Dm"]), -1, circuit.modulus) % circuit.modulus
            else:
                assert all(wit[c - m0] is None for c in hint["q"] + hint["rem"])
                q, rem = divmod(value(hint["D"]), circuit.modulus)
                assert PC.int_limbs(q, n, len(hint["q"])) == [z[c] for c in hint["q"]] and PC.int_limbs(rem, n, l) == [z[c] for c in hint["rem"]]
        assert api.decode_hints(api.encode_hints(hints)) == hints
        for order in ("reverse", 20004):
            shuffled = ConstraintSystem(r)
            PC.Reordered(circuit, order).generate_constraints(shuffled)
            assert _holds(shuffled) and sorted(map(repr, shuffled.rows)) == sorted(map(repr, cs.rows)) and shuffled.rows != cs.rows
    # LimbModDiv: every check division is exact (its remainder columns are zero), and an inverse is an inverse
    circuit = cases[0][0]
    inst, wit = circuit.native(r)
    hints = circuit.hints(2)
    assert [h.get("op", "longdiv") for h in hints] == ["moddiv", "longdiv"] * 3
    assert all(wit[c - 2] == 0 for h in hints if "rem" in h for c in h["rem"])
    Dp, Dm = circuit.cases[2][2:]
    assert circuit.cases[2][:2] == (None, None) and PC.limbs_int([wit[c - 2] for c in hints[4]["z"]], 64) * (Dp - Dm) % SECP == 1
    # EcAddChain equals plain affine addition on secp256k1: G3 + G2 + G2 = 7 G, by repeated addition of G
    G7 = G
    for _ in range(6):
        G7 = _ec_add(G7, G)
    chain = cases[4][0]
    inst, wit = chain.native(r)
    hints = chain.hints(2)
    assert [h.get("op", "longdiv") for h in hints] == ["moddiv", "longdiv", "longdiv", "longdiv"] * 2
    X3, Y3 = (PC.limbs_int([wit[c - 2] for c in h["rem"]], 64) for h in hints[-2:])
    assert (X3, Y3) == G7 == chain.result() and (Y3 * Y3 - X3 ** 3 - 7) % SECP == 0
    assert all(wit[c - 2] == 0 for h in (hints[1], hints[5]) for c in h["rem"])          # the slope checks are exact
    # the padding constant: a multiple of the modulus, every limb at least what a subtrahend limb can be
    for modulus, n, l, bits in ((SECP, 64, 4, None), (SECP, 86, 3, None), (65521 * 65519, 16, 2, None), (narrow, 128, 4, 120)):
        pad = PC.subtraction_pad(modulus, n, l, bits)
        assert PC.limbs_int(pad, n) % modulus == 0 and PC.limbs_int(pad, n) > 0 and min(pad) >= (1 << (bits or n)) - 1 and max(pad) < 1 << ((bits or n) + 1)
    with pytest.raises(AssertionError):
        PC.subtraction_pad(2 ** 64 + 13, 32, 3, 16)              # no narrow pad where a limb of the modulus is small
    # a product limb that could reach r is refused by the generator: full 128-bit limbs
    with pytest.raises(AssertionError):
        PC.LimbModDiv(PC.moddiv_cases(narrow, 1, 20005), narrow, 128, 4).native(r)
    # points whose x-coordinates meet have no chord
    with pytest.raises(AssertionError):
        PC.EcAddChain(G2, G2, SECP, 64, 4, 1).native(r)
