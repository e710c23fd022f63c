"""GPU: PM_ASSIGNMENT_SOLVE on circuits that MULTIPLY AND DIVIDE in a foreign field in one hint -- declared modular multiply-divide
hints (csrc/solve.hip: k_solve_modmuldiv; csrc/solve_steps.cuh: solve_modmuldiv; host/solve_plan.hpp: decode_hints' opcode 7,
KIND_MODMULDIV; the declaration: PM_KEY_HINTS of pm_pk_load_bytes, Polymath.set_hints).  The bar is equality, word for word, with
Python integers: the generators' own assignments (polymath_amd.circuits: LimbModMulDiv, EcDoubleAddChain, native(), whose values are
Python's pow(cD D, -1, P)).

Shapes are the smallest at which each mechanism can differ.  k_solve_modmuldiv gives a lane to a (hint, assignment), 64 lanes to a
workgroup: 1, 63, 64, 65 and 257 hints in one level are the workgroup edges, batches of 1, 3 and 70 are grid y.  (n, l) = (64, 4) and
(86, 3) with secp256k1's prime are the word-aligned and the word-crossing limb offsets, (128, 4) the widest limb -- there with a
modulus whose limbs are 121 bits and operand limbs of 120 -- and (16, 2) on the composite 65521 * 65519 the narrowest.  Every key of
the limb-width test carries the list combinations side by side: all six lists, no addend, no denominator, A = B on the same columns,
under the literals (3, 2), (1, 1) and (2^32 - 1, 2^32 - 1).

Fails without the feature: on the code before this record every declaration here is refused with "hint 0: unknown opcode 7"."""
import numpy as np
import pytest
import torch        # noqa: F401  before libpolymath_hip.so is loaded: torch brings its own HIP runtime (tests/ntt_device_child.py)

from oracle.pyref.fields import CURVES
from witness_solve_helpers import BOTH, NONE, PM_ERR_INVALID_ARG, PM_OK, _completes, _rows, _setup, _solve, key_cache

pytestmark = pytest.mark.gpu

_cached = key_cache()
_made = []          # every key this module made: freed when its last test has run (_keys_freed)
SECP = 2 ** 256 - 2 ** 32 - 977
SMALL = 65521 * 65519
BIG = 2 ** 32 - 1
G = (0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798, 0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8)


@pytest.fixture(scope="module", autouse=True)
def _keys_freed():
    """The module's keys (bases and window tables in device memory) go when the module is done, not when the session is"""
    yield
    for s in _made:
        s["pk"].free()
    _made.clear()


class _Beside:
    """several generators in one system, one after the other: instance = 1, then each generator's public input"""

    def __init__(self, parts):
        self.parts = parts

    def generate_constraints(self, cs):
        for part in self.parts:
            part.generate_constraints(cs)

    def hints(self, m0):
        return [hint for part in self.parts for hint in part.hints(m0)]      # each part's columns in the system it was last generated in

    def native(self, r):
        from polymath_amd import circuits as PC
        cs = PC._ValuesOnly(r)
        self.generate_constraints(cs)
        return cs.instance, cs.witness

    def partial(self, r):
        instance, witness = self.native(r)
        chosen = set()
        for part in self.parts:          # a part's _chosen are indices into the system it was generated in: this one
            chosen |= set(part._chosen)
        return [1] + [None] * (len(instance) - 1), [v if j in chosen else None for j, v in enumerate(witness)]


def _modulus(n, limbs):
    from polymath_amd import circuits as PC
    return {(64, 4): SECP, (86, 3): SECP, (16, 2): SMALL}.get((n, limbs)) or PC.narrow_modulus(n, limbs, 120)


def _muldiv(n, limbs, count, seed, cN=1, cD=1, decompose=True, **lists):
    from polymath_amd import circuits as PC
    modulus, narrow = _modulus(n, limbs), (n, limbs, 120) if n == 128 else None
    cases = PC.modmuldiv_cases(modulus, count, seed, cD=cD, narrow=narrow, **lists)
    return PC.LimbModMulDiv(cases, modulus, n, limbs, cN, cD, decompose=decompose, operand_bits=120 if n == 128 else None)


def _combinations(n, limbs, seed):
    """the list combinations side by side: all lists under (3, 2); no addend under (1, 1); no denominator under the largest literals
    (at 128-bit limbs under (3, 2): a product limb scaled by 2^32 would pass r); A = B on the same columns under (1, 1)"""
    big = (3, 2) if n == 128 else (BIG, BIG)
    return _Beside([_muldiv(n, limbs, 1, seed, 3, 2), _muldiv(n, limbs, 1, seed + 1, addend=False), _muldiv(n, limbs, 1, seed + 2, *big, denominator=False),
                    _muldiv(n, limbs, 1, seed + 3, square=True)])


def _declared(gpu_ctx, curve, key, circuit, seed, order=None):
    """a key for `circuit` (its rows in `order`) with the circuit's hints declared"""
    from polymath_amd import circuits as PC

    def make():
        s = _setup(gpu_ctx, curve, circuit if order is None else PC.Reordered(circuit, order), seed)
        s["pm"].set_hints(s["pk"], circuit.hints(s["q"].m0))
        _made.append(s)
        return s
    return _cached((curve, order) + key, make)


# ---- 1. LimbModMulDiv: the limb widths and the list combinations ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", BOTH)
@pytest.mark.parametrize("n,limbs", [(64, 4), (86, 3), (128, 4), (16, 2)])
def test_limb_modmuldiv(gpu_ctx, curve, n, limbs):
    from polymath_amd import circuits as PC
    r, modulus = CURVES[curve].r, _modulus(n, limbs)
    circuit = _combinations(n, limbs, 23100)
    s = _declared(gpu_ctx, curve, ("combinations", n, limbs), circuit, 23100 + n)
    hints = circuit.hints(s["q"].m0)
    assert [h.get("op", "longdiv") for h in hints] == ["modmuldiv", "longdiv"] * 4 and hints[6]["A"] == hints[6]["B"] and hints[2]["Np"] == hints[4]["Dp"] == []
    assert [(h["cN"], h["cD"]) for h in hints[::2]] == [(3, 2), (1, 1), (3, 2) if n == 128 else (BIG, BIG), (1, 1)]
    partial = circuit.partial(r)
    assert sum(v is not None for v in partial[1]) == (6 + 4 + 4 + 5) * limbs
    for batch in (1, 3, 70):
        circuits = [_combinations(n, limbs, 23200 + 100 * batch + 4 * i) for i in range(batch)]
        assignments = [ci.native(r) for ci in circuits]
        A, B, Np, Nm, Dp, Dm = circuits[0].parts[0].cases[0]
        Z = PC.limbs_int(assignments[0][1][6 * limbs:7 * limbs], n)              # Z of the first part follows its six operands
        assert 0 <= Z < modulus and 2 * (Dp - Dm) * Z % modulus == 3 * (A * B + Np - Nm) % modulus
        _completes(s, assignments, partial)


# ---- 2. the width of one level: the workgroup edges of k_solve_modmuldiv, and grid y ----------------------------------------------------------------------
@pytest.mark.parametrize("curve", BOTH)
@pytest.mark.parametrize("count", [1, 63, 64, 65, 257])
def test_level_width(gpu_ctx, curve, count):
    r = CURVES[curve].r
    s = _declared(gpu_ctx, curve, ("width", count), _muldiv(16, 2, count, 23300, 3, 2, decompose=False), 23300 + count)
    partial = _muldiv(16, 2, count, 23300, 3, 2, decompose=False).partial(r)
    for batch in (1, 3, 70):
        circuits = [_muldiv(16, 2, count, 23400 + 100 * batch + i, 3, 2, decompose=False) for i in range(batch)]
        _completes(s, [ci.native(r) for ci in circuits], partial)


# ---- 3. two shapes in one level: the launch's trip counts are the larger ones ------------------------------------------------------------------------------
def _two_shapes(seed):
    return _Beside([_muldiv(64, 4, 1, seed, 3, 2, decompose=False), _muldiv(128, 4, 1, seed + 1, 3, 2, decompose=False)])


@pytest.mark.parametrize("curve", BOTH)
def test_mixed_trip_counts(gpu_ctx, curve):
    """(64, 4) asks for 448 reduction rounds and 2 * 448 for the product and the inversion, (128, 4) for 640 and 2 * 512; both hints are
    ready at once, so they share a launch, and the narrower one runs under the wider one's counts"""
    r = CURVES[curve].r
    circuit = _two_shapes(23500)
    s = _declared(gpu_ctx, curve, ("two shapes",), circuit, 23500)
    hints = circuit.hints(s["q"].m0)
    assert [h.get("op") for h in hints] == ["modmuldiv", None, "modmuldiv", None] and [h["n"] for h in hints] == [64, 64, 128, 128]
    circuits = [_two_shapes(23510 + 2 * i) for i in range(3)]
    _completes(s, [ci.native(r) for ci in circuits], circuits[0].partial(r))


# ---- 4. the stuck conditions, each on the device, under a plan in matrix order and under a reordered one ---------------------------------------------------
class _Columns:
    """Z with 3 (D+) Z = A B + N+ (mod P), every operand and the modulus in given witness columns, limbs of 128 bits: A of 8 limbs (so
    that an assignment can carry a sum of 2^1024), B, N+ and D+ of one, P of four (2^512), Z of ONE limb (so that Z >= 2^128 can
    happen).  Witnesses A[8], B, N+, D+, P[4], Z (hinted), y = 2 Z by an ordinary row that follows the hint, w = A_0 B by an ordinary
    row that precedes nothing; the public input is y.  Reversed, the plan is a reordered one."""
    A, B, N, D, P, Z = list(range(8)), 8, 9, 10, [11, 12, 13, 14], 15

    def __init__(self, values=None):
        self.values = values or dict(A=[7], B=5, N=3, D=4, P=[1000003])

    def value(self):
        v = self.values
        P = sum(x << (128 * j) for j, x in enumerate(v["P"]))
        return (sum(x << (128 * j) for j, x in enumerate(v["A"])) * v["B"] + v["N"]) * pow(3 * v["D"], -1, P) % P

    def generate_constraints(self, cs):
        from polymath_amd.polymath import ConstraintSystem
        one, v = ConstraintSystem.ONE, self.values
        for x in list(v["A"]) + [0] * (8 - len(v["A"])) + [v["B"], v["N"], v["D"]] + list(v["P"]) + [0] * (4 - len(v["P"])):
            cs.new_witness_variable(x)
        Z = cs.new_witness_variable(self.value())
        y = cs.new_witness_variable(2 * self.value())
        w = cs.new_witness_variable(v["A"][0] * v["B"])
        cs.enforce_constraint([(1, ("wit", self.A[0]))], [(1, ("wit", self.B))], [(1, w)])
        cs.enforce_constraint([(2, Z)], [(1, one)], [(1, y)])
        cs.enforce_constraint([(1, y)], [(1, one)], [(1, cs.new_input_variable(2 * self.value()))])

    def native(self, r):
        from polymath_amd import circuits as PC
        cs = PC._ValuesOnly(r)
        self.generate_constraints(cs)
        return cs.instance, cs.witness

    @classmethod
    def hints(cls, m0):
        at = lambda cols: [m0 + c for c in cols]
        return [{"op": "modmuldiv", "n": 128, "z": at([cls.Z]), "A": at(cls.A), "B": at([cls.B]), "Np": at([cls.N]), "Nm": [], "Dp": at([cls.D]), "Dm": [], "cN": 1, "cD": 3,
                 "P": at(cls.P)}]


@pytest.mark.parametrize("curve", BOTH)
@pytest.mark.parametrize("order", [None, "reverse"])
def test_stuck_conditions(gpu_ctx, curve, order):
    """the middle assignment of 3 carries, in turn, every stuck condition at its boundary; the one beside it completes"""
    r = CURVES[curve].r
    s = _declared(gpu_ctx, curve, ("columns",), _Columns(), 23600, order)
    q, f = s["q"], s["f"]
    assert (q.m0, q.mw, q.nr) == (2, 18, 3)
    goods = [_Columns(dict(A=[7 + i, 1], B=5, N=3, D=4 + i, P=[P])) for i, P in enumerate((1000003, 1000033, 1000037))]          # primes
    assignments = [g.native(r) for g in goods]
    partial = ([1, None], [0] * 15 + [None] * 3)
    want = _completes(s, assignments, partial)
    top = 1 << 128
    # (name, the middle assignment's values, stuck?)
    cases = [("P even", dict(P=[1000004]), True), ("P = 1", dict(P=[1]), True), ("P = 5, a small modulus", dict(P=[5], D=2), False),
             ("P = 2^512", dict(P=[0, 0, 0, top]), True), ("P = 2^512 - 3", dict(P=[top - 3, top - 1, top - 1, top - 1], D=7, A=[21], B=5, N=0), False),      # Z = 105 / 21 = 5
             ("A = 2^1024", dict(A=[0] * 7 + [top]), True), ("A = 2^1024 - 1", dict(A=[top - 1] * 8), False),
             ("D = 0", dict(D=0), True), ("D = P", dict(D=1000033), True), ("cD D = 0 mod P though D != 0 mod P", dict(P=[15], D=5), True),
             ("cD D invertible modulo a composite P", dict(P=[35], D=4), False),
             ("Z = 2^128", dict(P=[(1 << 130) + 1], A=[0, 1], B=3, N=0, D=1), True), ("Z = 2^128 - 1", dict(P=[(1 << 130) + 1], A=[top - 1], B=3, N=0, D=1), False)]
    for name, change, is_stuck in cases:
        values = dict(goods[1].values, **change)
        _, rows = _rows(s, assignments, partial)
        given = list(values["A"]) + [0] * (8 - len(values["A"])) + [values["B"], values["N"], values["D"]] + list(values["P"]) + [0] * (4 - len(values["P"]))
        rows[1, q.m0:q.m0 + 15] = f.fr_limbs(given).reshape(15, 4)
        n_bad, bad_rows, stuck, full = _solve(s, rows)
        assert np.array_equal(full[0], want[0]) and np.array_equal(full[2], want[2]), name
        if is_stuck:
            hint_word = q.nr + 0
            assert stuck == [NONE, hint_word, NONE] and n_bad == [0, NONE, 0] and int(bad_rows[1][0]) == hint_word, name
            assert not full[1, q.m0 + _Columns.Z].any(), name          # zero in the output
        else:
            Z = _Columns(values).value()
            assert stuck == [NONE] * 3 and n_bad == [0] * 3 and np.array_equal(full[1, q.m0 + _Columns.Z], f.fr_limbs([Z]).reshape(4)), name


# ---- 5. EcDoubleAddChain: four coordinates -> verified proofs, the same bytes as the same call on the Python-completed assignment ------------------------
def _chains(count, first, n=64, limbs=4):
    """R_0 = (first + i) G and Q = G: 2 (2 R_0 + Q) + Q = (4 (first + i) + 3) G, and no exceptional case on the way"""
    from polymath_amd import circuits as PC
    return [PC.EcDoubleAddChain(PC.affine_mul(SECP, first + i, G), G, SECP, n, limbs, 2) for i in range(count)]


_assignments = key_cache()


@pytest.mark.parametrize("curve", BOTH)
@pytest.mark.parametrize("n,limbs", [(64, 4), (86, 3)])
def test_ec_double_add_chain(gpu_ctx, curve, n, limbs):
    from polymath_amd import circuits as PC
    r = CURVES[curve].r
    circuits = _chains(70, 7, n, limbs)
    assignments = _assignments((curve, n), lambda: [ci.native(r) for ci in circuits])
    partial = circuits[0].partial(r)
    assert sum(v is not None for v in partial[1]) == 4 * limbs                  # four coordinates
    for i, ci in enumerate(circuits[:3]):
        assert ci.result() == PC.affine_mul(SECP, 4 * (7 + i) + 3, G)
        last = ci.hints(2)[-1]                                                  # the last reduction's remainder is Y of the last step
        assert PC.limbs_int([assignments[i][1][c - 2] for c in last["rem"]], n) == ci.result()[1]
    key = lambda order=None: _declared(gpu_ctx, curve, ("ecdouble", n, limbs), _chains(1, 5, n, limbs)[0], 23700, order)
    s = key()
    hints = circuits[0].hints(s["q"].m0)
    assert [h.get("op", "longdiv") for h in hints] == ["modmuldiv", "longdiv", "longdiv", "longdiv", "moddiv", "longdiv", "longdiv", "longdiv"] * 2
    _completes(s, assignments[:1], partial)
    want = _completes(s, assignments[:3], partial)
    _completes(s, assignments, partial)
    for order in ("reverse", 23701):
        assert np.array_equal(_completes(key(order), assignments[:3], partial), want)
    if (n, limbs) != (64, 4):
        return
    # inputs -> proofs
    count = 3
    pm, pk, q = s["pm"], s["pk"], s["q"]
    _, rows = _rows(s, assignments[:count], partial)
    part = [(np.ascontiguousarray(rows[i, :q.m0]), np.ascontiguousarray(rows[i, q.m0:])) for i in range(count)]
    full = [(np.ascontiguousarray(want[i, :q.m0]), np.ascontiguousarray(want[i, q.m0:])) for i in range(count)]
    r_as = [[51 + i, 61 + i] for i in range(count)]
    vk = pm.make_vk(pk, s["x"], s["z"])
    for glue in ("host", "device"):
        proofs, statuses, instances = pm.prove_batch(pk, part, r_as, solve=True, glue=glue)
        plain_proofs, plain_statuses = pm.prove_batch(pk, full, r_as, glue=glue)
        assert statuses == [0] * count and plain_statuses == [0] * count and instances == [inst for inst, _ in assignments[:count]], glue
        assert proofs == plain_proofs, glue
        assert all(pm.verify(vk, assignments[i][0][1:], proofs[i]) for i in range(count)), glue
        assert not pm.verify(vk, assignments[0][0][1:], proofs[1])
    assert pm.check_batch(pk, part, solve=True) == [(0, [])] * count


# ---- 6. through the C ABI: the refusals; redeclaration and clearing; a sharded key; opcodes 1, 3, 5 and 7 on one key -------------------------------------
def _four_opcodes(seed):
    """the wide long division first (LimbModMul lays its hints out from witness 0), then a modular division with its long division,
    then a multiply-divide"""
    from polymath_amd import circuits as PC
    return _Beside([PC.LimbModMul(PC.modmul_pairs(SECP, 1, seed), SECP, 64, 4, wide=True), PC.LimbModDiv(PC.moddiv_cases(SECP, 1, seed + 1), SECP, 64, 4),
                    _muldiv(64, 4, 1, seed + 2, 3, 2)])


@pytest.mark.parametrize("curve", BOTH)
def test_four_opcodes_on_one_key(gpu_ctx, curve):
    from polymath_amd import api
    r = CURVES[curve].r
    circuit = _four_opcodes(23800)
    s = _declared(gpu_ctx, curve, ("four opcodes",), circuit, 23800)
    hints = circuit.hints(s["q"].m0)
    assert [h.get("op", "longdiv") for h in hints] == ["longdiv_wide", "moddiv", "longdiv", "modmuldiv", "longdiv"]
    assert sorted({int(api.encode_hints([h])[0]) for h in hints}) == [1, 3, 5, 7]
    circuits = [_four_opcodes(23810 + 3 * i) for i in range(3)]
    _completes(s, [ci.native(r) for ci in circuits], circuits[0].partial(r))


@pytest.mark.parametrize("curve", BOTH)
def test_refusals_and_redeclaration(gpu_ctx, curve):
    from polymath_amd import api
    r = CURVES[curve].r
    circuit = _muldiv(86, 3, 2, 23900, 3, 2)
    s = _declared(gpu_ctx, curve, ("refusals",), circuit, 23900)
    pm, pk, q = s["pm"], s["pk"], s["q"]
    good = circuit.hints(q.m0)
    ncols = q.m0 + q.mw
    h = good[0]
    assert h["op"] == "modmuldiv" and "op" not in good[1]

    def refused(hints, text):
        rc = pk.set_hints(hints)
        message = pm.ctx.last_error()
        assert rc == PM_ERR_INVALID_ARG and text in message, (rc, message)

    variant = lambda **kw: [dict(h, **kw)]
    many = list(range(1, 34))
    words = api.encode_hints(good)
    assert int(words[0]) == 7
    for opcode in (2, 4, 6, 8):
        bad = words.copy(); bad[0] = opcode
        refused(bad, "pm_pk_set_hints: hint 0: unknown opcode %d" % opcode)
    bad = words.copy(); bad[10] = 2
    refused(bad, "pm_pk_set_hints: hint 0: unknown flags 2")
    refused(words[:-1], "pm_pk_set_hints: hint 3: the record is truncated")
    refused(words[:12], "pm_pk_set_hints: hint 0: the record is truncated")
    bad = words.copy(); bad[11] = 0
    refused(bad, "pm_pk_set_hints: hint 0: cN = 0 is outside 1..4294967295")
    bad = words.copy(); bad[12] = 1 << 32
    refused(bad, "pm_pk_set_hints: hint 0: cD = 4294967296 is outside 1..4294967295")
    refused(variant(n=0), "hint 0: n = 0 is outside 1..128")
    refused(variant(n=129), "hint 0: n = 129 is outside 1..128")
    refused(variant(z=[]), "hint 0: kz = 0 is outside 1..16")
    refused(variant(z=list(range(1, 18))), "hint 0: kz = 17 is outside 1..16")
    refused(variant(literal=[1] * 17), "hint 0: kP = 17 is outside 1..16")
    refused(variant(A=[]), "hint 0: kA = 0 is outside 1..32")
    refused(variant(A=many), "hint 0: kA = 33 is outside 1..32")
    refused(variant(B=[]), "hint 0: kB = 0 is outside 1..32")
    refused(variant(B=many), "hint 0: kB = 33 is outside 1..32")
    refused(variant(Np=many), "hint 0: kNp = 33 is outside 0..32")
    refused(variant(Nm=many), "hint 0: kNm = 33 is outside 0..32")
    refused(variant(Dp=many), "hint 0: kDp = 33 is outside 0..32")
    refused(variant(Dm=many), "hint 0: kDm = 33 is outside 0..32")
    refused(variant(Dp=[]), "hint 0: kDm = 3 with kDp = 0")
    refused(variant(n=128, A=many[:9]), "hint 0: n (kA - 1) = 1024 is 1024 or more")
    refused(variant(n=128, Dm=many[:9]), "hint 0: n (kDm - 1) = 1024 is 1024 or more")
    refused(variant(n=128, literal=[1] * 5), "hint 0: n (kP - 1) = 512 is 512 or more")
    refused(variant(B=[ncols]), "hint 0: column %d is not below m0 + mw = %d" % (ncols, ncols))
    refused(variant(z=[0]), "hint 0: an output is column 0 (the constant one)")
    refused(variant(z=[h["z"][0]] * 2), "hint 0: output column %d is named twice" % h["z"][0])
    refused(variant(A=[h["z"][1]]), "hint 0: output column %d is an input of the hint as well" % h["z"][1])
    refused([h, dict(good[1], q=[h["z"][2]])], "hint 1: output column %d is an output of hint 0 as well" % h["z"][2])
    refused([good[1], dict(h, z=[good[1]["rem"][0]])], "hint 1: output column %d is an output of hint 0 as well" % good[1]["rem"][0])
    refused(variant(literal=[3, r]), "hint 0: literal limb 1 is not below r")
    # a sharded key: refused whatever the declaration says, and freed here
    from polymath_amd import polymath as PM
    half = pm.setup((PM.R1CS(q.m0, q.mw, q.a, q.b, q.c), s["inst"], s["wit"]), 123, 456, 0, 2)
    assert half.set_hints(good) == PM_ERR_INVALID_ARG and "pm_pk_set_hints: hints on a sharded key are not supported" in pm.ctx.last_error()
    half.free()
    # the key is unchanged by all of them: the first declaration still completes the witness
    circuits = [_muldiv(86, 3, 2, 23910 + i, 3, 2) for i in range(3)]
    assignments, partial = [ci.native(r) for ci in circuits], circuit.partial(r)
    want = _completes(s, assignments, partial)
    # some outputs given and some marked; a special marker on an output
    _, rows = _rows(s, assignments, partial)
    mixed = rows.copy()
    mixed[:, h["z"][0]] = want[:, h["z"][0]]
    xs, ws = np.ascontiguousarray(mixed[:, :q.m0]), np.ascontiguousarray(mixed[:, q.m0:])
    assert pk.r1cs_check_batch(xs, ws, 2, solve=True)[0] == PM_ERR_INVALID_ARG and "pm solve: hint 0: some outputs are marked unknown and some are given" in pm.ctx.last_error()
    for marker in (api.QUOTIENT_LIMBS, api.INDICATOR_LIMBS, api.SQRT_LIMBS):
        mixed = rows.copy()
        mixed[:, good[2]["z"][1]] = marker
        xs, ws = np.ascontiguousarray(mixed[:, :q.m0]), np.ascontiguousarray(mixed[:, q.m0:])
        assert pk.r1cs_check_batch(xs, ws, 2, solve=True)[0] == PM_ERR_INVALID_ARG and "pm solve: hint 2: an output carries the quotient, indicator or square-root marker" in pm.ctx.last_error()
    # a caller that supplies Z itself: the multiply-divide hints inert, the long divisions still active
    supplied = rows.copy()
    for hint in good:
        if hint.get("op") == "modmuldiv":
            supplied[:, hint["z"]] = want[:, hint["z"]]
    n_bad, _, stuck, full = _solve(s, supplied)
    assert n_bad == [0] * 3 and stuck == [NONE] * 3 and np.array_equal(full, want)
    # cleared: nothing determines Z, and the plan made under the declaration is not reused ...
    assert pk.set_hints([]) == PM_OK
    xs, ws = np.ascontiguousarray(rows[:, :q.m0]), np.ascontiguousarray(rows[:, q.m0:])
    assert pk.r1cs_check_batch(xs, ws, 2, solve=True)[0] == PM_ERR_INVALID_ARG and "in any row order" in pm.ctx.last_error()
    # ... a hint whose factor is its own check's quotient never becomes ready, and the refusal names it and its input ...
    assert pk.set_hints([dict(h, A=[good[1]["q"][0]])] + good[1:]) == PM_OK
    assert pk.r1cs_check_batch(xs, ws, 2, solve=True)[0] == PM_ERR_INVALID_ARG
    assert "pm solve: hint 0: input column %d is never determined; column " % good[1]["q"][0] in pm.ctx.last_error(), pm.ctx.last_error()
    # ... and declared again it completes again
    pm.set_hints(pk, good)
    assert np.array_equal(_completes(s, assignments, partial), want)
