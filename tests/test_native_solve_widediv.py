"""CPU: the witness solver's declared wide long-division hints (polymath_amd/host/solve_plan.hpp: decode_hints' opcode 5,
KIND_LONGDIV_WIDE, LAUNCH_LONGDIV_WIDE; csrc/solve_steps.cuh: wide_estimate, longdiv_wide_words -- the digit recurrence that the
kernel k_solve_longdiv_wide distributes over a wave -- and solve_longdiv_wide), compiled with g++ from
tests/native/solve_widediv_selftest.cpp.  Wide divisions against literals computed with Python's divmod (solve_widediv_cases.hpp,
which tools/gen_solve_widediv_cases.py writes into the test's directory before the program is built): the six shapes and the operand
families of the GPU test; by the recurrence's counters the add-back family executes an add-back and the saturating family a saturated
estimate at every listed size, which random operands do not; every stuck condition at its boundary; every refusal with its text and at
its boundary (n (kD - 1) = 8192 and 8190: 8191 is prime and no record reaches it); opcodes 2 and 4 refused; opcode 1 not widened;
the three opcodes in one declaration; the levels and launches where they meet; markers; a corpus in order, reversed and shuffled; the
stuck word.  Both curves; once more as a stand-alone program under AddressSanitizer and UBSan.  The generators of
polymath_amd.circuits are checked on Python integers."""
import os
import subprocess
import sys

import pytest

from oracle.pyref.fields import CURVES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "native", "solve_widediv_selftest.cpp")


@pytest.fixture(scope="module")
def cases():
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_solve_widediv_cases.py")], capture_output=True, text=True, check=True).stdout


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_solve_widediv_host_selftest(tmp_path, flags, cases):
    exe = str(tmp_path / "solve_widediv_selftest")
    (tmp_path / "solve_widediv_cases.hpp").write_text(cases)          # the program's literals: Python's divmod, written fresh
    subprocess.check_call(["g++", "-std=c++17", "-I", str(tmp_path)] + flags + ["-o", exe, SOURCE])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    for curve in ("bls12_381", "bn254"):
        assert "%s: 0 failures of 734" % curve in out.stdout.splitlines(), out.stdout
    # the families that reach algorithm D's rare branches are in the table by name, at every listed size that fits a shape
    for m in (3, 64, 65, 128):
        assert "saturating m = %d" % m in cases
        for k in (1, 2, 3):
            assert "add-back m = %d k = %d" % (m, k) in cases
    for m in (2, 3, 63, 64, 65, 127, 128):
        assert "a divisor of %d significant words" % m in cases
    for name in ("a divisor of one significant word", "normalising shift 0", "normalising shift 31", "E = 2^4096 - 1 under D = 2^8192 - 1", "every limb r - 1"):
        assert name in cases


def test_random_operands_never_add_back():
    """why the families are named: a Python model of algorithm D on 200 random 4096 / 2048-bit pairs executes no add-back and no
    saturated estimate (the chance is about 2 / 2^32 a digit)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_solve_widediv_cases as gen
    finally:
        sys.path.pop(0)
    from polymath_amd import circuits as PC
    g = PC.SplitMix64(0x72616E646F6D)
    draw = lambda bits: sum(g.next_u64() << (64 * i) for i in range(bits // 64)) | 1 << (bits - 1)
    for _ in range(200):
        D, E = draw(4096), draw(2048)
        assert gen.model(D, E)[2:] == (0, 0)
    for m in (3, 64, 65, 128):
        E = (1 << (32 * m - 1)) + 1
        assert all(gen.model(((E - 1) << (32 * k)) | 3, E)[2] >= 1 for k in (1, 2, 3))
        E = (0xFFFFFFFF << (32 * (m - 1))) | 5
        assert gen.model((E << 32) - 1, E)[3] >= 1


def _holds(cs):
    r = cs.r
    col = lambda v: cs.instance[v[1]] if v[0] in ("one", "inst") else cs.witness[v[1]]
    dot = lambda lc: sum(coef * col(v) for coef, v in lc) % r
    return all(dot(a) * dot(b) % r == dot(c) for a, b, c in cs.rows)


@pytest.mark.parametrize("curve", ["bls12_381", "bn254"])
def test_generators_on_python_integers(curve):
    """native() against generate_constraints, the rows on the assignment, what partial() leaves to the device, hints() against Python's
    divmod on the assignment's columns, Reordered, and the encode / decode round trip"""
    from polymath_amd import api, circuits as PC
    from polymath_amd.polymath import ConstraintSystem
    r = CURVES[curve].r
    modulus, signature = PC.rsa_modulus(2048, 22000)
    assert modulus.bit_length() == 2048 and modulus & 1 and 0 <= signature < modulus
    families = PC.division_cases(64, 33, 16, r, 22001)
    cases = [(PC.RsaVerify(signature, modulus, 64, 32, squarings=3), 64, 32),
             (PC.RsaVerify(signature, modulus, 121, 17, squarings=2, witness_modulus=True), 121, 2 * 17),
             (PC.RsaVerify(signature % (2 ** 61 - 1), 2 ** 61 - 1, 16, 4, squarings=16, decompose=True), 16, 4),
             (PC.LimbModMul(PC.modmul_pairs(modulus, 2, 22002), modulus, 64, 32, decompose=False, wide=True), 64, 2 * 2 * 32),
             (PC.ModMulChain(signature, 65537, modulus, 64, 32, 2, witness_modulus=True, decompose=False, wide=True), 64, 3 * 32),
             (PC.LimbDivision([(D, E) for _, D, E in families], 64, 33, 16), 64, sum(len(D) + len(E) for _, D, E in families)),
             (PC.LimbDivision([(D, E) for _, D, E in families[:5]], 64, 33, 16, divisor="literal"), 64, sum(len(D) for _, D, _ in families[:5]))]
    for circuit, n, given in cases:
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
            assert hint["op"] == "longdiv_wide" and hint["n"] == n and list(hint)[0] == "op"
            assert all(wit[c - m0] is None for c in hint["q"] + hint["rem"])
            E = value(hint["E"]) if "E" in hint else PC.limbs_int(hint["literal"], n)
            q, rem = divmod(value(hint["D"]), E)
            assert PC.int_limbs(q, n, len(hint["q"])) == [z[c] for c in hint["q"]] and PC.int_limbs(rem, n, len(hint["rem"])) == [z[c] for c in hint["rem"]]
        assert api.decode_hints(api.encode_hints(hints)) == hints and int(api.encode_hints(hints)[0]) == api.HINT_LONGDIV_WIDE == 5
        for order in ("reverse", 22004):
            shuffled = ConstraintSystem(r)
            PC.Reordered(circuit, order).generate_constraints(shuffled)
            assert _holds(shuffled) and sorted(map(repr, shuffled.rows)) == sorted(map(repr, cs.rows)) and shuffled.rows != cs.rows
    # RsaVerify is Python's pow: y = s^(2^squarings + 1) mod N, in the remainder of the last hint
    rsa = PC.RsaVerify(signature, modulus, 64, 32)
    inst, wit = rsa.native(r)
    last = rsa.hints(2)[-1]
    assert len(rsa.hints(2)) == 17 and PC.limbs_int([wit[c - 2] for c in last["rem"]], 64) == pow(signature, 65537, modulus)
    assert inst[1] == sum(wit[c - 2] for c in last["rem"]) % r
    # without wide=True the existing generators declare what they declared: opcode 1, no "op" key
    narrow = PC.LimbModMul(PC.modmul_pairs(2 ** 255 - 19, 1, 22005), 2 ** 255 - 19, 64, 4)
    assert all("op" not in h for h in narrow.hints(2)) and int(api.encode_hints(narrow.hints(2))[0]) == 1
    assert all("op" not in h for h in PC.ModMulChain(3, 5, 2 ** 255 - 19, 64, 4, 2).hints(2))
    # the bytes of opcodes 1 and 3 are unchanged, opcode 5 is opcode 1's record under another first word, 2 and 4 stay refused
    old = [{"n": 64, "q": [10, 11], "rem": [12], "D": [3, 4, 5], "literal": [2 ** 64 - 1, 5]}, {"op": "moddiv", "n": 86, "z": [50], "Np": [], "Nm": [], "Dp": [9], "Dm": [], "P": [7]}]
    words = [int(v) for v in api.encode_hints(old)]
    assert words == [1, 64, 2, 1, 3, 2, 1, 10, 11, 12, 3, 4, 5, 2 ** 64 - 1, 0, 0, 0, 5, 0, 0, 0, 3, 86, 1, 0, 0, 1, 0, 1, 0, 50, 9, 7]
    wide = [int(v) for v in api.encode_hints([dict(old[0], op="longdiv_wide")])]
    assert wide == [5] + words[1:21] and api.decode_hints(wide) == [dict([("op", "longdiv_wide")] + list(old[0].items()))]
    assert api.decode_hints(api.encode_hints(old + [dict(old[0], op="longdiv_wide")])) == old + [dict(old[0], op="longdiv_wide")]
    for opcode in (2, 4):
        with pytest.raises(ValueError):
            api.decode_hints([opcode] + words[1:21])
    assert api.WIDE_LIMITS == {"n": 128, "kq": 128, "kr": 64, "kD": 128, "kE": 64}
    # LimbDivision refuses a stuck case unless told, and then stores zeros
    with pytest.raises(AssertionError):
        PC.LimbDivision([([5], [0])], 64, 1, 1).native(r)
    stuck = PC.LimbDivision([([5], [0]), ([7], [2])], 64, 1, 1, stuck=True)
    assert stuck.stuck_cases() == [True, False] and stuck.native(r)[1] == [5, 0, 0, 0, 0, 7, 2, 3, 1, 4]
    # a product limb that could reach r is refused by the generator: 32 limbs of 128 bits
    with pytest.raises(AssertionError):
        PC.RsaVerify(signature, modulus, 128, 16).native(r)
