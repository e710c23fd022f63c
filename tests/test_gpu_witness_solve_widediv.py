"""GPU: PM_ASSIGNMENT_SOLVE on circuits that divide WIDE integers -- declared wide long-division hints (csrc/solve.hip:
k_solve_longdiv_wide, a wave per division; csrc/solve_steps.cuh: longdiv_wide_words, the recurrence it distributes; host/solve_plan.hpp:
decode_hints' opcode 5, KIND_LONGDIV_WIDE; the declaration: PM_KEY_HINTS of pm_pk_load_bytes, Polymath.set_hints).  The bar is equality,
word for word, with Python integers: the generators' own assignments (polymath_amd.circuits: LimbDivision, LimbModMul(wide=True),
RsaVerify, whose quotients and remainders are Python's divmod).

Shapes are the smallest at which each mechanism can differ.  (n, kD, kE) = (64, 33, 16) is one limb past opcode 1, (64, 63, 32) the
RSA-2048 reduction, (121, 33, 17) the zk-email limbs with word-crossing offsets, (128, 64, 32) the widest limbs and the whole 8192 /
4096 bits, (32, 128, 64) two limbs to every lane, (1, 2, 1) the narrowest.  The operand families (circuits.division_cases) are the
divisor's word counts at lane and half-wave edges, both normalising shifts, the family that makes algorithm D add the divisor back
and the one that saturates its estimate (random operands do neither), the orderings of D and E, and limbs of r - 1 that make every
word carry.  1, 3, 4, 5 and 257 hints in a level are the workgroup edges of four waves to a workgroup, batches of 1, 3 and 70 grid y.
On the code before this record every declaration here is refused with "hint 0: unknown opcode 5"."""
import numpy as np
import pytest
import torch        # noqa: F401  before libpolymath_hip.so is loaded: torch brings its own HIP runtime (tests/ntt_device_child.py)

from oracle.pyref.fields import CURVES
from witness_solve_helpers import BOTH, NONE, PM_ERR_INVALID_ARG, PM_OK, _completes, _rows, _setup, _solve, key_cache

pytestmark = pytest.mark.gpu

_cached = key_cache()
_made = []          # every key this module made: freed when its last test has run (_keys_freed)
SHAPES = [(64, 33, 16), (64, 63, 32), (121, 33, 17), (128, 64, 32), (32, 128, 64), (1, 2, 1)]
SECP = 2 ** 256 - 2 ** 32 - 977
G = (0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798, 0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8)


def _declared(gpu_ctx, curve, key, circuit, seed, order=None):
    """a key for `circuit` (its rows in `order`) with the circuit's hints declared"""
    from polymath_amd import circuits as PC

    def make():
        s = _setup(gpu_ctx, curve, circuit if order is None else PC.Reordered(circuit, order), seed)
        s["pm"].set_hints(s["pk"], circuit.hints(s["q"].m0))
        _made.append(s)
        return s
    return _cached((curve, order) + key, make)


@pytest.fixture(scope="module", autouse=True)
def _keys_freed():
    """The module's keys (bases and window tables in device memory) go when the module is done, not when the session is"""
    yield
    for s in _made:
        s["pk"].free()
    _made.clear()


def _families(curve, shape, seed, divisor="columns"):
    from polymath_amd import circuits as PC
    n, kD, kE = shape
    cases = PC.division_cases(n, kD, kE, CURVES[curve].r, seed)
    return PC.LimbDivision([(D, E) for _, D, E in cases], n, kD, kE, divisor=divisor), [name for name, _, _ in cases]


# ---- 1. LimbDivision, one level: the shapes and the operand families, the divisor in columns and as a literal -----------------------------------------------
@pytest.mark.parametrize("curve", BOTH)
@pytest.mark.parametrize("divisor", ["columns", "literal"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%d-%d-%d" % s)
def test_limb_division(gpu_ctx, curve, shape, divisor):
    r = CURVES[curve].r
    circuit, names = _families(curve, shape, 21000, divisor)
    for needle in ("random", "one significant word", "D < E", "D = 0", "D = E", "D = E - 1") + (("add-back m = 3 k = 1", "saturating m = 3", "shift 31") if shape[0] > 1 else ()):
        assert any(needle in name for name in names), needle
    if shape in ((64, 63, 32), (32, 128, 64), (128, 64, 32)):
        assert "add-back m = 64 k = 3" in names and "saturating m = 64" in names and "a divisor of 63 significant words" in names
    if shape == (128, 64, 32):
        assert "add-back m = 128 k = 3" in names and "saturating m = 65" in names and "E = 2^4096 - 1 under D = 2^8192 - 1" in names and "a divisor of 127 significant words" in names
    s = _declared(gpu_ctx, curve, ("families", shape, divisor), circuit, 21000 + shape[0])
    hints = circuit.hints(s["q"].m0)
    assert all(h["op"] == "longdiv_wide" for h in hints) and ("literal" in hints[0]) == (divisor == "literal")
    assignments = [circuit.native(r)]
    if divisor == "columns":          # a second assignment of other values under the same key: a literal divisor is the key's
        assignments.append(_families(curve, shape, 21001)[0].native(r))
        assert len(assignments[1][1]) == len(assignments[0][1])
    _completes(s, assignments, circuit.partial(r))


# ---- 2. the width of one level: four waves to a workgroup, and grid y ---------------------------------------------------------------------------------------
def _narrow(count, seed):
    """`count` divisions of the narrowest shape, limbs that are not normalised: D = d0 + 2 d1 below 2^10, E below 2^4"""
    from polymath_amd import circuits as PC
    g = PC.SplitMix64(seed)
    return PC.LimbDivision([([g.next_u64() % 256, g.next_u64() % 256], [1 + g.next_u64() % 15]) for _ in range(count)], 1, 10, 4)


@pytest.mark.parametrize("curve", BOTH)
@pytest.mark.parametrize("count", [1, 3, 4, 5, 257])
def test_level_width(gpu_ctx, curve, count):
    r = CURVES[curve].r
    circuit = _narrow(count, 21100)
    s = _declared(gpu_ctx, curve, ("width", count), circuit, 21100 + count)
    for batch in (1, 3, 70):
        _completes(s, [_narrow(count, 21200 + 100 * batch + i).native(r) for i in range(batch)], circuit.partial(r))


# ---- 3. stuck: one bad assignment in a batch of 3 is reported at nr + h, its neighbours are intact -------------------------------------------------------
def _stuck_runs(s, circuit_of, good, cases, r):
    """cases: [(D limbs, E limbs, stuck)] for the middle assignment; its neighbours carry `good`"""
    q = s["q"]
    for D, E, stuck_wanted in cases:
        circuits = [circuit_of(*good), circuit_of(D, E), circuit_of(*good)]
        assert circuits[1].stuck_cases() == [stuck_wanted], (D, E)
        assignments = [ci.native(r) for ci in circuits]
        want, rows = _rows(s, assignments, circuits[0].partial(r))
        n_bad, bad_rows, stuck, full = _solve(s, rows)
        if stuck_wanted:
            word = q.nr + 0
            assert stuck == [NONE, word, NONE] and n_bad == [0, NONE, 0] and int(bad_rows[1][0]) == word and int(bad_rows[1][1]) == NONE, (D, E, stuck)
            assert np.array_equal(full[0], want[0]) and np.array_equal(full[2], want[2])
        else:
            assert stuck == [NONE] * 3 and n_bad == [0] * 3 and np.array_equal(full, want), (D, E, stuck)


@pytest.mark.parametrize("curve", BOTH)
@pytest.mark.parametrize("order", [None, "reverse"])
def test_stuck_at_the_hint(gpu_ctx, curve, order):
    from polymath_amd import circuits as PC
    r = CURVES[curve].r
    full = (1 << 128) - 1
    # the operands' own limits, on the widest shape: limbs that are not normalised reach 2^8192 and 2^4096 exactly
    wide = lambda D, E: PC.LimbDivision([(D, E)], 128, 64, 32, stuck=True)
    good = ([5] * 64, [3] * 32)
    s = _declared(gpu_ctx, curve, ("stuck wide",), wide(*good), 21300, order)
    _stuck_runs(s, wide, good, [([7] * 64, [0] * 32, True),
                                ([7] * 64, [0] * 31 + [1 << 128], True), ([full] * 64, [full] * 32, False),
                                ([0] * 63 + [1 << 128], [9] * 32, True), ([full] * 64, [9] + [0] * 31, False)], r)
    # the outputs' limits: q = 2^(n kq) and rem = 2^(n kr) exactly, and one less
    small = lambda D, E: PC.LimbDivision([(D, E)], 64, 2, 1, stuck=True)
    good = ([5, 6, 7, 0], [9, 1])
    s = _declared(gpu_ctx, curve, ("stuck small",), small(*good), 21301, order)
    ones = (1 << 64) - 1
    _stuck_runs(s, small, good, [([0, 0, 1, 0], [1, 0], True), ([ones, ones, 0, 0], [1, 0], False),
                                 ([0, 1, 0, 0], [1, 1], True), ([ones, 0, 0, 0], [1, 1], False)], r)


# ---- 4. RSA ---------------------------------------------------------------------------------------------------------------------------------------------------
def _rsa(n, limbs, witness_modulus, seed):
    from polymath_amd import circuits as PC
    modulus, signature = PC.rsa_modulus(2048, seed)
    return PC.RsaVerify(signature, modulus, n, limbs, witness_modulus=witness_modulus)


@pytest.mark.parametrize("curve", BOTH)
def test_limb_modmul_at_rsa_size(gpu_ctx, curve):
    from polymath_amd import circuits as PC
    r = CURVES[curve].r
    modulus = PC.rsa_modulus(2048, 21400)[0]
    make = lambda seed: PC.LimbModMul(PC.modmul_pairs(modulus, 1, seed), modulus, 64, 32, decompose=True, wide=True)
    circuit = make(21401)
    s = _declared(gpu_ctx, curve, ("modmul rsa",), circuit, 21400)
    assert circuit.hints(s["q"].m0)[0]["op"] == "longdiv_wide"
    for batch in (1, 3):
        _completes(s, [make(21410 + 10 * batch + i).native(r) for i in range(batch)], circuit.partial(r))


@pytest.mark.parametrize("curve", BOTH)
@pytest.mark.parametrize("order", [None, "reverse", 21500])
@pytest.mark.parametrize("n,limbs,witness_modulus", [(64, 32, False), (64, 32, True), (121, 17, False), (121, 17, True)])
def test_rsa_verify(gpu_ctx, curve, n, limbs, witness_modulus, order):
    r = CURVES[curve].r
    # a literal modulus is the key's; in witness columns every assignment brings its own
    circuits = [_rsa(n, limbs, witness_modulus, 21510 + (i if witness_modulus else 0)) for i in range(2)]
    if not witness_modulus:
        from polymath_amd import circuits as PC
        circuits[1] = PC.RsaVerify(circuits[0].signature ^ 0x5555, circuits[0].modulus, n, limbs)
    s = _declared(gpu_ctx, curve, ("rsa", n, limbs, witness_modulus), circuits[0], 21500 + n, order)
    partial = circuits[0].partial(r)
    assert sum(v is not None for v in partial[1]) == limbs * (2 if witness_modulus else 1)          # the signature's limbs (and the modulus')
    _completes(s, [ci.native(r) for ci in circuits], partial)


@pytest.mark.parametrize("curve", BOTH)
def test_rsa_to_proofs(gpu_ctx, curve):
    """signature limbs -> proofs that verify, the bytes of the same call on the Python-completed assignment, under both glues"""
    r, count = CURVES[curve].r, 2
    from polymath_amd import circuits as PC
    first = _rsa(64, 32, False, 21510)
    circuits = [first, PC.RsaVerify(first.signature ^ 0x5555, first.modulus, 64, 32)]
    s = _declared(gpu_ctx, curve, ("rsa", 64, 32, False), first, 21500 + 64)
    pm, pk, q = s["pm"], s["pk"], s["q"]
    assignments, partial = [ci.native(r) for ci in circuits], first.partial(r)
    want, rows = _rows(s, assignments, partial)
    part = [(np.ascontiguousarray(rows[i, :q.m0]), np.ascontiguousarray(rows[i, q.m0:])) for i in range(count)]
    full = [(np.ascontiguousarray(want[i, :q.m0]), np.ascontiguousarray(want[i, q.m0:])) for i in range(count)]
    r_as = [[51 + i, 61 + i] for i in range(count)]
    vk = pm.make_vk(pk, s["x"], s["z"])
    for glue in ("host", "device"):
        proofs, statuses, instances = pm.prove_batch(pk, part, r_as, solve=True, glue=glue)
        plain_proofs, plain_statuses = pm.prove_batch(pk, full, r_as, glue=glue)
        assert statuses == [0] * count and plain_statuses == [0] * count and instances == [inst for inst, _ in assignments], glue
        assert proofs == plain_proofs, glue
        assert all(pm.verify(vk, assignments[i][0][1:], proofs[i]) for i in range(count)), glue
        assert not pm.verify(vk, assignments[0][0][1:], proofs[1])


# ---- 5. through the C ABI: the refusals, redeclaration and clearing, a sharded key, the three opcodes on one key -----------------------------------------
@pytest.mark.parametrize("curve", BOTH)
def test_refusals_and_redeclaration(gpu_ctx, curve):
    from polymath_amd import api, circuits as PC, polymath as PM
    r = CURVES[curve].r
    make = lambda seed: PC.LimbDivision([(D, E) for _, D, E in PC.division_cases(64, 5, 2, r, seed)[:3]], 64, 5, 2)
    circuit = make(21600)
    s = _declared(gpu_ctx, curve, ("refusals",), circuit, 21600)
    pm, pk, q = s["pm"], s["pk"], s["q"]
    good = circuit.hints(q.m0)
    ncols = q.m0 + q.mw
    h = good[0]
    cols = lambda k: list(range(1, 1 + k))

    def refused(hints, text):
        rc = pk.set_hints(hints)
        message = pm.ctx.last_error()
        assert rc == PM_ERR_INVALID_ARG and text in message, (rc, message)

    variant = lambda **kw: [dict(h, **kw)]
    words = api.encode_hints(good)
    assert int(words[0]) == 5
    for opcode in (2, 4, 6):
        bad = words.copy(); bad[0] = opcode
        refused(bad, "pm_pk_set_hints: hint 0: unknown opcode %d" % opcode)
    bad = words.copy(); bad[6] = 2
    refused(bad, "pm_pk_set_hints: hint 0: unknown flags 2")
    refused(words[:-1], "pm_pk_set_hints: hint 2: the record is truncated")
    refused(words[:6], "pm_pk_set_hints: hint 0: the record is truncated")
    refused(variant(n=0), "hint 0: n = 0 is outside 1..128")
    refused(variant(n=129), "hint 0: n = 129 is outside 1..128")
    refused(variant(q=[]), "hint 0: kq = 0 is outside 1..128")
    refused(variant(q=cols(129)), "hint 0: kq = 129 is outside 1..128")
    refused(variant(rem=[]), "hint 0: kr = 0 is outside 1..64")
    refused(variant(rem=cols(65)), "hint 0: kr = 65 is outside 1..64")
    refused(variant(D=[]), "hint 0: kD = 0 is outside 1..128")
    refused(variant(D=cols(129)), "hint 0: kD = 129 is outside 1..128")
    refused(variant(E=[]), "hint 0: kE = 0 is outside 1..64")
    refused(variant(E=cols(65)), "hint 0: kE = 65 is outside 1..64")
    refused(variant(n=128, D=cols(65)), "hint 0: n (kD - 1) = 8192 is 8192 or more")
    refused(variant(n=128, E=cols(33)), "hint 0: n (kE - 1) = 4096 is 4096 or more")
    # opcode 1 is not widened: today's text
    narrow = {k: v for k, v in h.items() if k != "op"}
    refused([dict(narrow, D=cols(33))], "hint 0: kD = 33 is outside 1..32")
    refused([dict(narrow, E=cols(17))], "hint 0: kE = 17 is outside 1..16")
    refused(variant(D=[ncols]), "hint 0: column %d is not below m0 + mw = %d" % (ncols, ncols))
    refused(variant(q=[0]), "hint 0: an output is column 0 (the constant one)")
    refused(variant(q=[h["q"][0]] * 2), "hint 0: output column %d is named twice" % h["q"][0])
    refused(variant(D=[h["rem"][1]]), "hint 0: output column %d is an input of the hint as well" % h["rem"][1])
    refused([h, dict(narrow, q=[good[2]["q"][0]], rem=[h["q"][2]], D=[1], E=[2])], "hint 1: output column %d is an output of hint 0 as well" % h["q"][2])
    refused([h, {"op": "moddiv", "n": 64, "z": [h["rem"][0]], "Dp": [1], "literal": [7]}], "hint 1: output column %d is an output of hint 0 as well" % h["rem"][0])
    refused([{k: v for k, v in dict(h, literal=[3, r]).items() if k != "E"}], "hint 0: literal limb 1 is not below r")
    # a sharded key: refused whatever the declaration says, and freed here
    half = pm.setup((PM.R1CS(q.m0, q.mw, q.a, q.b, q.c), s["inst"], s["wit"]), 123, 456, 0, 2)
    assert half.set_hints(good) == PM_ERR_INVALID_ARG and "pm_pk_set_hints: hints on a sharded key are not supported" in pm.ctx.last_error()
    half.free()
    # the key is unchanged by all of them: the first declaration still completes the witness
    assignments, partial = [make(21610 + i).native(r) for i in range(3)], circuit.partial(r)
    want = _completes(s, assignments, partial)
    _, rows = _rows(s, assignments, partial)
    mixed = rows.copy()
    mixed[:, h["q"][0]] = want[:, h["q"][0]]
    xs, ws = np.ascontiguousarray(mixed[:, :q.m0]), np.ascontiguousarray(mixed[:, q.m0:])
    assert pk.r1cs_check_batch(xs, ws, 2, solve=True)[0] == PM_ERR_INVALID_ARG and "pm solve: hint 0: some outputs are marked unknown and some are given" in pm.ctx.last_error()
    # a caller that supplies q and rem of hint 1 itself: that hint inert, the others active
    supplied = rows.copy()
    supplied[:, good[1]["q"] + good[1]["rem"]] = want[:, good[1]["q"] + good[1]["rem"]]
    n_bad, _, stuck, full = _solve(s, supplied)
    assert n_bad == [0] * 3 and stuck == [NONE] * 3 and np.array_equal(full, want)
    # cleared: nothing determines q and rem, and the plan made under the declaration is not reused ...
    assert pk.set_hints([]) == PM_OK
    xs, ws = np.ascontiguousarray(rows[:, :q.m0]), np.ascontiguousarray(rows[:, q.m0:])
    assert pk.r1cs_check_batch(xs, ws, 2, solve=True)[0] == PM_ERR_INVALID_ARG and "in any row order" in pm.ctx.last_error()
    # ... a hint whose dividend names another hint's output that waits for this one's never becomes ready ...
    assert pk.set_hints([dict(h, D=[good[1]["q"][0]]), dict(good[1], D=[h["q"][0]])] + good[2:]) == PM_OK
    assert pk.r1cs_check_batch(xs, ws, 2, solve=True)[0] == PM_ERR_INVALID_ARG
    assert "pm solve: hint 0: input column %d is never determined; column " % good[1]["q"][0] in pm.ctx.last_error(), pm.ctx.last_error()
    # ... and declared again it completes again
    pm.set_hints(pk, good)
    assert np.array_equal(_completes(s, assignments, partial), want)


class _Beside:
    """several generators in one system, one after the other: instance = 1, then each generator's public input.  A part's hints are
    asked for at the column where its own witnesses begin"""

    def __init__(self, parts):
        self.parts = parts

    def generate_constraints(self, cs):
        self.first = []
        for part in self.parts:
            self.first.append(len(cs.witness))
            part.generate_constraints(cs)

    def hints(self, m0):
        from polymath_amd import circuits as PC
        return [hint for part, first in zip(self.parts, self.first) for hint in part.hints(m0 if isinstance(part, PC._PartialModDiv) else m0 + first)]

    def _values(self, r):
        from polymath_amd import circuits as PC
        cs = PC._ValuesOnly(r)
        self.generate_constraints(cs)
        return cs

    def native(self, r):
        cs = self._values(r)
        return cs.instance, cs.witness

    def partial(self, r):
        cs = self._values(r)
        marks = [None] * len(cs.witness)          # a part's _chosen are witness indices of the system it was generated in
        for part in self.parts:
            for j in part._chosen:
                marks[j] = cs.witness[j]
        return [1] + [None] * (len(cs.instance) - 1), marks


def _multiple(k):
    point = G
    for _ in range(k - 1):
        (x1, y1), (x2, y2) = point, G
        lam = (3 * x1 * x1) * pow(2 * y1, -1, SECP) % SECP if point == G else (y2 - y1) * pow(x2 - x1, -1, SECP) % SECP
        x3 = (lam * lam - x1 - x2) % SECP
        point = (x3, (lam * (x1 - x3) - y1) % SECP)
    return point


def _three_opcodes(seed, r):
    from polymath_amd import circuits as PC
    x0, b = PC.modmul_pairs(SECP, 1, seed)[0]
    return _Beside([PC.ModMulChain(x0, b, SECP, 64, 4, 2, decompose=False), PC.EcAddChain(_multiple(5 + seed % 3), _multiple(2), SECP, 64, 4, 1, decompose=False),
                    PC.LimbDivision([(D, E) for _, D, E in PC.division_cases(64, 33, 16, r, seed)[:4]], 64, 33, 16)])


@pytest.mark.parametrize("curve", BOTH)
def test_three_opcodes_on_one_key(gpu_ctx, curve):
    r = CURVES[curve].r

    def make():
        circuit = _three_opcodes(21700, r)
        s = _setup(gpu_ctx, curve, circuit, 21700)
        hints = circuit.hints(s["q"].m0)
        assert {h.get("op", "longdiv") for h in hints} == {"longdiv", "moddiv", "longdiv_wide"}
        s["pm"].set_hints(s["pk"], hints)
        _made.append(s)
        return s
    s = _cached((curve, "three opcodes"), make)
    circuits = [_three_opcodes(21700 + i, r) for i in range(3)]
    _completes(s, [ci.native(r) for ci in circuits], circuits[0].partial(r))
