"""CPU: the witness solver's declared modular multiply-divide hints (polymath_amd/host/solve_plan.hpp: decode_hints' opcode 7,
KIND_MODMULDIV, LAUNCH_MODMULDIV; csrc/solve_steps.cuh: shift_up, solve_modmuldiv -- the text the kernel k_solve_modmuldiv calls),
compiled with g++ from tests/native/solve_modmuldiv_selftest.cpp.  The Z with cD (D+ - D-) Z = cN (A B + N+ - N-) mod P against
literals computed with Python's pow (solve_modmuldiv_cases.hpp, which tools/gen_solve_modmuldiv_cases.py writes into the test's
directory before the program is built): P = secp256k1's prime, BLS12-381's q, 2^512 - 1, 3 and 65521 * 65519; A, B in {0, 1, P - 1,
limbs that carry, sums just below 2^1024}; every combination of empty lists; A = B on the same columns; the three pairs of literals;
D+ < D-; the Euclid's worst cases by name; every stuck condition at its boundary; every refusal with its text; four opcodes in one
declaration and in one level; a chain in order, reversed and shuffled; the root cause under a reordered plan.  Both curves; once
more as a stand-alone program under AddressSanitizer and UBSan.  The generators of polymath_amd.circuits (LimbModMulDiv,
EcDoubleAddChain, EcdsaVerify) are checked on Python integers.

Fails without the feature: on the code before this record every declaration here is refused with "hint 0: unknown opcode 7", and
neither the step body nor the generators exist."""
import os
import subprocess
import sys

import pytest

from oracle.pyref.fields import CURVES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "native", "solve_modmuldiv_selftest.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_solve_modmuldiv_host_selftest(tmp_path, flags):
    exe = str(tmp_path / "solve_modmuldiv_selftest")
    cases = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_solve_modmuldiv_cases.py")], capture_output=True, text=True, check=True).stdout
    (tmp_path / "solve_modmuldiv_cases.hpp").write_text(cases)          # the program's literals: Python's pow, written fresh
    subprocess.check_call(["g++", "-std=c++17", "-I", str(tmp_path)] + flags + ["-o", exe, SOURCE])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    # 288 multiply-divides x 5; 99 more: the declaration and the planner, the meeting opcodes, the chain, the stuck word
    for curve in ("bls12_381", "bn254"):
        assert "%s: 0 failures of 1539" % curve in out.stdout.splitlines(), out.stdout
    for named in ("D = 2^(L - 1), the bound's worst case of halvings", "D = P - 1", "D = (P + 1) / 2", "D = (P - 1) / 2", "A = B on the same columns",
                  "cD D = 0 mod P though D != 0 mod P", "stuck: A = 2^1024 exactly", "D- = 2^1024 - 1", "stuck: P = 2^512 exactly", "stuck: Z = 2^(n kz)",
                  "cN = 4294967295, cD = 4294967295", "a curve with a != 0"):
        assert named in cases, named          # the cases the contract names are in the table by name


def _failing(cs):
    r = cs.r
    col = lambda v: cs.instance[v[1]] if v[0] in ("one", "inst") else cs.witness[v[1]]
    dot = lambda lc: sum(coef * col(v) for coef, v in lc) % r
    return [i for i, (a, b, c) in enumerate(cs.rows) if dot(a) * dot(b) % r != dot(c)]


def _check_hints(PC, api, circuit, cs, wit, n, moduli):
    """hints() against Python's pow and divmod on the assignment's columns, and the encoding's round trip"""
    m0 = len(cs.instance)
    hints = circuit.hints(m0)
    z = cs.instance + cs.witness
    value = lambda cols: sum(z[c] << (n * j) for j, c in enumerate(cols))
    for hint in hints:
        P = PC.limbs_int(hint["literal"], n)
        assert hint["n"] == n and P in moduli
        outputs = hint["z"] if "z" in hint else hint["q"] + hint["rem"]
        assert all(wit[c - m0] is None for c in outputs)
        if hint.get("op") == "modmuldiv":
            N = hint["cN"] * (value(hint["A"]) * value(hint["B"]) + value(hint["Np"]) - value(hint["Nm"])) % P
            D = hint["cD"] * (value(hint["Dp"]) - value(hint["Dm"]) if hint["Dp"] or hint["Dm"] else 1) % P
            assert value(hint["z"]) == N * pow(D, -1, P) % P
        elif hint.get("op") == "moddiv":
            N = (value(hint["Np"]) - value(hint["Nm"])) % P if hint["Np"] or hint["Nm"] else 1
            assert value(hint["z"]) == N * pow(value(hint["Dp"]) - value(hint["Dm"]), -1, P) % P
        else:
            q, rem = divmod(value(hint["D"]), P)
            assert PC.int_limbs(q, n, len(hint["q"])) == [z[c] for c in hint["q"]] and PC.int_limbs(rem, n, len(hint["rem"])) == [z[c] for c in hint["rem"]]
    assert api.decode_hints(api.encode_hints(hints)) == hints
    return hints


@pytest.mark.parametrize("curve", ["bls12_381", "bn254"])
def test_generators_on_python_integers(curve):
    """native() against generate_constraints, the rows on the assignment, what partial() leaves to the device, hints() against Python's
    pow and divmod on the assignment's columns, and Reordered"""
    from polymath_amd import api, circuits as PC
    from polymath_amd.polymath import ConstraintSystem
    r = CURVES[curve].r
    SECP, _, _, G = PC.SECP256K1
    narrow, small, big = PC.narrow_modulus(128, 4, 120), 65521 * 65519, 2 ** 32 - 1
    cases = [(PC.LimbModMulDiv(PC.modmuldiv_cases(SECP, 3, 21000, cD=2), SECP, 64, 4, 3, 2), 64, 18 * 4),
             (PC.LimbModMulDiv(PC.modmuldiv_cases(SECP, 2, 21001, addend=False), SECP, 86, 3), 86, 8 * 3),
             (PC.LimbModMulDiv(PC.modmuldiv_cases(SECP, 2, 21002, cD=big, denominator=False), SECP, 64, 4, big, big), 64, 8 * 4),
             (PC.LimbModMulDiv(PC.modmuldiv_cases(narrow, 2, 21003, cD=2, narrow=(128, 4, 120)), narrow, 128, 4, 3, 2, operand_bits=120), 128, 12 * 4),
             (PC.LimbModMulDiv(PC.modmuldiv_cases(small, 4, 21004, square=True), small, 16, 2, decompose=False), 16, 20 * 2),
             (PC.EcDoubleAddChain(G, G, SECP, 64, 4, 2), 64, 4 * 4)]
    for circuit, n, given in cases:
        cs = ConstraintSystem(r)
        circuit.generate_constraints(cs)
        assert not _failing(cs) and circuit.native(r) == (cs.instance, cs.witness)
        inst, wit = circuit.partial(r)
        assert inst == [1, None] and sum(v is not None for v in wit) == given and all(v is None or v == w for v, w in zip(wit, cs.witness))
        _check_hints(PC, api, circuit, cs, wit, n, (circuit.modulus,))
        for order in ("reverse", 21005):
            shuffled = ConstraintSystem(r)
            PC.Reordered(circuit, order).generate_constraints(shuffled)
            assert not _failing(shuffled) and sorted(map(repr, shuffled.rows)) == sorted(map(repr, cs.rows)) and shuffled.rows != cs.rows
    # LimbModMulDiv: the one check division is exact, and A = B names A's columns twice
    circuit = cases[0][0]
    inst, wit = circuit.native(r)
    hints = circuit.hints(2)
    assert [h.get("op", "longdiv") for h in hints] == ["modmuldiv", "longdiv"] * 3 and all(h["cN"] == 3 and h["cD"] == 2 for h in hints[::2])
    assert all(wit[c - 2] == 0 for h in hints if "rem" in h for c in h["rem"])
    A, B, Np, Nm, Dp, Dm = circuit.cases[0]
    assert 2 * (Dp - Dm) * PC.limbs_int([wit[c - 2] for c in hints[0]["z"]], 64) % SECP == 3 * (A * B + Np - Nm) % SECP
    square = cases[4][0].hints(2)
    assert all(h["A"] == h["B"] for h in square[::2]) and all(c[1] is None for c in cases[4][0].cases)
    # EcDoubleAddChain equals plain affine arithmetic on secp256k1: 2 (2 G + G) + G = 7 G, by repeated addition of G
    G7 = G
    for _ in range(6):
        G7 = PC.affine_add(SECP, G7, G)
    chain = cases[5][0]
    inst, wit = chain.native(r)
    hints = chain.hints(2)
    assert [h.get("op", "longdiv") for h in hints] == ["modmuldiv", "longdiv", "longdiv", "longdiv", "moddiv", "longdiv", "longdiv", "longdiv"] * 2
    assert hints[0]["A"] == hints[0]["B"] and hints[0]["Np"] == hints[0]["Dm"] == [] and (hints[0]["cN"], hints[0]["cD"]) == (3, 2)
    X3, Y3 = (PC.limbs_int([wit[c - 2] for c in h["rem"]], 64) for h in hints[-2:])
    assert (X3, Y3) == G7 == chain.result() and (Y3 * Y3 - X3 ** 3 - 7) % SECP == 0
    assert all(wit[c - 2] == 0 for h in (hints[1], hints[5], hints[9], hints[13]) for c in h["rem"])          # the slope checks are exact
    # the padding constant for product limbs: a multiple of the modulus, every limb at least the subtrahend's bound
    for modulus, n, bounds in ((SECP, 64, [3 * 4 * 2 ** 128] * 7), (SECP, 86, [2 ** 175, 2 ** 176, 5]), (small, 16, [0, 1, 2 ** 40]), (narrow, 128, [2 ** 244] * 7)):
        pad = PC.product_pad(modulus, n, bounds)
        assert PC.limbs_int(pad, n) % modulus == 0 and PC.limbs_int(pad, n) > 0 and all(v >= hi for v, hi in zip(pad, bounds)) and len(pad) >= len(bounds)
        assert all(v < 2 * (1 << hi.bit_length()) + (1 << n) for v, hi in zip(pad, bounds))
    # a vertical tangent and meeting x-coordinates are asserted
    with pytest.raises(AssertionError):
        PC.EcDoubleAddChain(G, PC.affine_add(SECP, G, G), SECP, 64, 4, 1).native(r)          # 2 G + 2 G: the chord's x-coordinates meet
    with pytest.raises(AssertionError):
        PC.EcDoubleAddChain((1, 0), G, SECP, 64, 4, 1).native(r)                # Y = 0: a vertical tangent


def _is_prime(v):
    return v > 1 and all(v % d for d in range(2, int(v ** 0.5) + 1))


@pytest.mark.parametrize("curve", ["bls12_381", "bn254"])
def test_ecdsa_verify_on_python_integers(curve):
    """the toy curve's parameters re-checked; EcdsaVerify accepts its signatures, and with s + 1 its last check rows fail and nothing else"""
    from polymath_amd import api, circuits as PC
    from polymath_amd.polymath import ConstraintSystem
    r = CURVES[curve].r
    p, b, order, G = PC.TOY_CURVE
    S = PC.TOY_START
    assert p == 2 ** 22 - 3 and _is_prime(p) and _is_prime(order) and order < p < 2 * order
    assert all((y * y - x ** 3 - b) % p == 0 for x, y in (G, S)) and PC.affine_mul(p, order, G) is None and PC.affine_mul(p, order - 1, G) == (G[0], p - G[1])
    sp, sb, sorder, sG = PC.SECP256K1
    assert all((y * y - x ** 3 - sb) % sp == 0 for x, y in (sG, PC.SECP256K1_START)) and PC.affine_mul(sp, sorder, sG) is None
    signatures = PC.ecdsa_cases(PC.TOY_CURVE, 3, 22000)
    for Q, h, r_sig, s in signatures:
        w = pow(s, -1, order)
        R = PC.affine_add(p, PC.affine_mul(p, h * w % order, G), PC.affine_mul(p, r_sig * w % order, Q))
        assert R[0] % order == r_sig and (Q[1] ** 2 - Q[0] ** 3 - b) % p == 0
        assert PC.ecdsa_schedule(PC.TOY_CURVE, S, Q, h * w % order, r_sig * w % order, 22) == R
    Q, h, r_sig, s = signatures[0]
    circuit = PC.EcdsaVerify(PC.TOY_CURVE, Q, h, r_sig, s, 11, 2)
    cs = ConstraintSystem(r)
    circuit.generate_constraints(cs)
    assert not _failing(cs) and circuit.accepts() and circuit.native(r) == (cs.instance, cs.witness) and 15000 < len(cs.rows) < 2 ** 15
    inst, wit = circuit.partial(r)
    assert inst == [1, None] and sum(v is not None for v in wit) == 5 * 2 and wit[:10] == PC.int_limbs(h, 11, 2) + PC.int_limbs(r_sig, 11, 2) + PC.int_limbs(s, 11, 2) + \
        PC.int_limbs(Q[0], 11, 2) + PC.int_limbs(Q[1], 11, 2)
    hints = _check_hints(PC, api, circuit, cs, wit, 11, (p, order))
    ops = [h_.get("op", "longdiv") for h_ in hints]
    assert ops[:4] == ["moddiv", "longdiv"] * 2 and ops.count("modmuldiv") == 22 and ops.count("moddiv") == 2 + 2 * 22 + 1 and ops[-1] == "longdiv"
    assert PC.limbs_int(hints[0]["literal"], 11) == order and PC.limbs_int(hints[4]["literal"], 11) == p and PC.limbs_int(hints[-1]["literal"], 11) == order
    # 67 point operations: 22 doublings, 44 additions, the correction
    assert ops.count("modmuldiv") + ops.count("moddiv") - 2 == 67
    # the last rows are the l check rows rem_j - r_j = 0
    assert all(b_ == [(1, ConstraintSystem.ONE)] and c == [] for _, b_, c in cs.rows[-2:])
    forged = PC.EcdsaVerify(PC.TOY_CURVE, Q, h, r_sig, (s + 1) % order, 11, 2)
    bad = ConstraintSystem(r)
    forged.generate_constraints(bad)
    failing = _failing(bad)
    assert not forged.accepts() and failing and set(failing) <= {len(bad.rows) - 2, len(bad.rows) - 1} and len(bad.rows) == len(cs.rows)
    with pytest.raises(ValueError):
        PC.EcdsaVerify(PC.TOY_CURVE, Q, h, r_sig, 0, 11, 2).native(r)          # s = 0 has no inverse
