"""GPU: PM_ASSIGNMENT_SOLVE on circuits that DIVIDE in a foreign field -- declared modular-division hints (csrc/solve.hip:
k_solve_moddiv; csrc/solve_steps.cuh: modinv_odd, solve_moddiv; host/solve_plan.hpp: decode_hints' opcode 3, KIND_MODDIV; the
declaration: PM_KEY_HINTS of pm_pk_load_bytes, Polymath.set_hints).  The bar is equality, word for word, with Python integers: the
generators' own assignments (polymath_amd.circuits: LimbModDiv, EcAddChain, native(), whose quotients are Python's pow(D, -1, P)).

Shapes are the smallest at which each mechanism can differ.  k_solve_moddiv gives a lane to a (hint, assignment), 64 lanes to a
workgroup: 1, 63, 64, 65 and 257 hints in one level are the workgroup edges, batches of 1, 3 and 70 are grid y.  (n, l) = (64, 4) and
(86, 3) with secp256k1's prime are the word-aligned and the word-crossing limb offsets, (128, 4) the widest limb -- there with a
modulus whose limbs are 121 bits and operand limbs of 120, because a product of two full 128-bit limbs would pass r (circuits.py:
subtraction_pad) -- and (16, 2) the narrowest.  EcAddChain is modular hints, blocks, long divisions, decompositions and carry chains
alternating over 22 levels.  On the code before this record every declaration here is refused with "hint 0: unknown opcode 3"."""
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
G = (0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798, 0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8)


def _modulus(n, limbs):
    from polymath_amd import circuits as PC
    return {(64, 4): SECP, (86, 3): SECP, (16, 2): SMALL}.get((n, limbs)) or PC.narrow_modulus(n, limbs, 120)


def _moddiv(n, limbs, count, seed, decompose=True):
    """`count` cases, the last an inverse where there are two or more; at n = 128 operand limbs of 120 bits"""
    from polymath_amd import circuits as PC
    modulus, narrow = _modulus(n, limbs), (n, limbs, 120) if n == 128 else None
    cases = PC.moddiv_cases(modulus, count, seed, inverses=1 if count > 1 else 0, narrow=narrow)
    return PC.LimbModDiv(cases, modulus, n, limbs, decompose=decompose, operand_bits=120 if n == 128 else None)


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


def _div_key(gpu_ctx, curve, n, limbs, count, decompose=True):
    return _declared(gpu_ctx, curve, ("div", n, limbs, count, decompose), _moddiv(n, limbs, count, 19100, decompose), 19100 + n + count)


# ---- 1. LimbModDiv: the limb widths ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", BOTH)
@pytest.mark.parametrize("n,limbs", [(64, 4), (86, 3), (128, 4), (16, 2)])
def test_limb_moddiv(gpu_ctx, curve, n, limbs):
    from polymath_amd import circuits as PC
    r, count, modulus = CURVES[curve].r, 2, _modulus(n, limbs)
    s = _div_key(gpu_ctx, curve, n, limbs, count)
    partial = _moddiv(n, limbs, count, 19100).partial(r)
    assert sum(v is not None for v in partial[1]) == (4 + 2) * limbs          # a division's four operands, an inverse's two
    for batch in (1, 3, 70):
        circuits = [_moddiv(n, limbs, count, 19200 + 100 * batch + i) for i in range(batch)]
        assignments = [ci.native(r) for ci in circuits]
        Np, Nm, Dp, Dm = circuits[0].cases[0]
        Z = PC.limbs_int(assignments[0][1][4 * limbs:5 * limbs], n)              # Z of case 0 follows its four operands
        assert 0 <= Z < modulus and Z * (Dp - Dm) % modulus == (Np - Nm) % modulus
        _completes(s, assignments, partial)


# ---- 2. the width of one level: the workgroup edges of k_solve_moddiv, and grid y -------------------------------------------------------------------------
@pytest.mark.parametrize("curve", BOTH)
@pytest.mark.parametrize("count", [1, 63, 64, 65, 257])
def test_level_width(gpu_ctx, curve, count):
    r = CURVES[curve].r
    s = _div_key(gpu_ctx, curve, 16, 2, count, decompose=False)
    partial = _moddiv(16, 2, count, 19100, decompose=False).partial(r)
    for batch in (1, 3, 70):
        circuits = [_moddiv(16, 2, count, 19300 + 100 * batch + i, decompose=False) for i in range(batch)]
        _completes(s, [ci.native(r) for ci in circuits], partial)


# ---- 3. two shapes in one level: the launch's trip counts are the larger ones ------------------------------------------------------------------------------
class _Beside:
    """several generators in one system, one after the other: instance = 1, then each generator's public input"""

    def __init__(self, parts):
        self.parts = parts

    def generate_constraints(self, cs):
        for part in self.parts:
            part.generate_constraints(cs)

    def hints(self, m0):
        return [hint for part in self.parts for hint in part.hints(m0)]      # each part's columns in the system it was last generated in

    def assignment(self, r, values_only):
        from polymath_amd import circuits as PC
        from polymath_amd.polymath import ConstraintSystem
        cs = PC._ValuesOnly(r) if values_only else ConstraintSystem(r)
        self.generate_constraints(cs)
        return cs

    def native(self, r):
        cs = self.assignment(r, True)
        return cs.instance, cs.witness

    def partial(self, r):
        cs = self.assignment(r, True)
        chosen = {j for part in self.parts for j in part._chosen}
        return [1] + [None] * (len(cs.instance) - 1), [v if j in chosen else None for j, v in enumerate(cs.witness)]


def _two_shapes(seed):
    return _Beside([_moddiv(64, 4, 1, seed, decompose=False), _moddiv(128, 4, 1, seed + 1, decompose=False)])


@pytest.mark.parametrize("curve", BOTH)
def test_mixed_trip_counts(gpu_ctx, curve):
    """(64, 4) asks for 448 reduction rounds and 2 * 448 inversion rounds, (128, 4) for 640 and 2 * 512; both hints are ready at once, so
    they share a launch, and the narrower one runs under the wider one's counts"""
    r = CURVES[curve].r

    def make():
        circuit = _two_shapes(19400)
        s = _setup(gpu_ctx, curve, circuit, 19400)
        hints = circuit.hints(s["q"].m0)
        assert [h.get("op") for h in hints] == ["moddiv", None, "moddiv", None] and [h["n"] for h in hints] == [64, 64, 128, 128]
        s["pm"].set_hints(s["pk"], hints)
        _made.append(s)
        return s
    s = _cached((curve, "two shapes"), make)
    circuits = [_two_shapes(19410 + 2 * i) for i in range(3)]
    _completes(s, [ci.native(r) for ci in circuits], circuits[0].partial(r))


# ---- 4. EcAddChain: four coordinates -> verified proofs, the same bytes as the same call on the Python-completed assignment ------------------------------
def _ec_add(p1, p2):
    """affine addition or doubling on secp256k1 (y^2 = x^3 + 7), Python integers"""
    (x1, y1), (x2, y2) = p1, p2
    lam = (3 * x1 * x1) * pow(2 * y1, -1, SECP) % SECP if p1 == p2 else (y2 - y1) * pow(x2 - x1, -1, SECP) % SECP
    x3 = (lam * lam - x1 - x2) % SECP
    return x3, (lam * (x1 - x3) - y1) % SECP


def _multiple(k):
    point = G
    for _ in range(k - 1):
        point = _ec_add(point, G)
    return point


def _chains(count, first):
    """R_0 = (first + i) G and Q = 2 G: R_0 + 2 Q = (first + i + 4) G, and no x-coordinates meet on the way"""
    from polymath_amd import circuits as PC
    return [PC.EcAddChain(_multiple(first + i), _multiple(2), SECP, 64, 4, 2) for i in range(count)]


def _chain_key(gpu_ctx, curve, order=None):
    return _declared(gpu_ctx, curve, ("ecadd",), _chains(1, 5)[0], 19500, order)


@pytest.mark.parametrize("curve", BOTH)
def test_ec_add_chain(gpu_ctx, curve):
    from polymath_amd import circuits as PC
    r, count = CURVES[curve].r, 3
    circuits = _chains(count, 7)
    assignments, partial = [ci.native(r) for ci in circuits], circuits[0].partial(r)
    assert sum(v is not None for v in partial[1]) == 16                         # four coordinates of four limbs
    for i, ci in enumerate(circuits):
        assert ci.result() == _multiple(7 + i + 4) and (ci.result()[1] ** 2 - ci.result()[0] ** 3 - 7) % SECP == 0
        last = ci.hints(2)[-1]                                                  # the last reduction's remainder is Y3 of the last step
        assert PC.limbs_int([assignments[i][1][c - 2] for c in last["rem"]], 64) == ci.result()[1]
    s = _chain_key(gpu_ctx, curve)
    hints = circuits[0].hints(s["q"].m0)
    assert [h.get("op", "longdiv") for h in hints] == ["moddiv", "longdiv", "longdiv", "longdiv"] * 2
    want = _completes(s, assignments, partial)
    assert np.array_equal(_completes(_chain_key(gpu_ctx, curve, "reverse"), assignments, partial), want)
    # inputs -> proofs
    pm, pk, q = s["pm"], s["pk"], s["q"]
    _, rows = _rows(s, assignments, partial)
    part = [(np.ascontiguousarray(rows[i, :q.m0]), np.ascontiguousarray(rows[i, q.m0:])) for i in range(count)]
    full = [(np.ascontiguousarray(want[i, :q.m0]), np.ascontiguousarray(want[i, q.m0:])) for i in range(count)]
    r_as = [[51 + i, 61 + i] for i in range(count)]
    vk = pm.make_vk(pk, s["x"], s["z"])
    proofs = None
    for glue in ("host", "device"):
        proofs, statuses, instances = pm.prove_batch(pk, part, r_as, solve=True, glue=glue)
        plain_proofs, plain_statuses = pm.prove_batch(pk, full, r_as, glue=glue)
        assert statuses == [0] * count and plain_statuses == [0] * count and instances == [inst for inst, _ in assignments], glue
        assert proofs == plain_proofs, glue
        assert all(pm.verify(vk, assignments[i][0][1:], proofs[i]) for i in range(count)), glue
    assert not pm.verify(vk, assignments[0][0][1:], proofs[1])
    assert pm.check_batch(pk, part, solve=True) == [(0, [])] * count
    # several groups, host and device pointers: the same words and the same bytes, and the caller's rows are only read
    xs, ws = np.ascontiguousarray(rows[:, :q.m0]), np.ascontiguousarray(rows[:, q.m0:])
    dx, dw = torch.from_numpy(xs.view(np.int64)).cuda(), torch.from_numpy(ws.view(np.int64)).cuda()
    torch.cuda.synchronize()
    ncols = q.m0 + q.mw
    check_log = (2 * ncols - 1).bit_length()
    gpu_ctx.set_option("msm_max_piece_log", check_log)                     # the check solves in groups of 2 (restored by conftest)
    for device in (False, True):
        if device:
            rc, n_bad, _, _ = pk.r1cs_check_batch(dx.data_ptr(), dw.data_ptr(), 2, on_device=True, count=count, solve=True)
        else:
            rc, n_bad, _, _ = pk.r1cs_check_batch(xs, ws, 2, solve=True)
        assert rc == PM_OK and not n_bad.any(), pm.ctx.last_error()
        assert np.array_equal(pk.solved_assignments(count, q.mw), want), device
    prove_log = (10 * pk.n + 22 - 1).bit_length()
    gpu_ctx.set_option("msm_max_piece_log", prove_log)                     # the prover in groups of 1
    for glue in ("host", "device"):
        assert pm.prove_batch(pk, part, r_as, solve=True, glue=glue)[0] == proofs, glue
        got = pm.prove_batch(pk, part, r_as, device_ptrs=(dx.data_ptr(), dw.data_ptr()), solve=True, glue=glue)
        assert got[0] == proofs and got[2] == [inst for inst, _ in assignments], glue
    assert np.array_equal(dx.cpu().numpy().view(np.uint64).reshape(xs.shape), xs) and np.array_equal(dw.cpu().numpy().view(np.uint64).reshape(ws.shape), ws)


# ---- 5. stuck: one bad assignment in a batch of 3 is reported at nr + h, and its neighbours are intact ------------------------------------------------------
@pytest.mark.parametrize("curve", BOTH)
def test_stuck_at_the_hint(gpu_ctx, curve):
    """case 0 of the middle assignment gets D- = D+, so D = 0 (mod P): no inverse"""
    r = CURVES[curve].r
    s = _div_key(gpu_ctx, curve, 64, 4, 2)
    q = s["q"]
    circuits = [_moddiv(64, 4, 2, 19600 + i) for i in range(3)]
    assignments = [ci.native(r) for ci in circuits]
    want, rows = _rows(s, assignments, circuits[0].partial(r))
    rows[1, q.m0 + 12:q.m0 + 16] = rows[1, q.m0 + 8:q.m0 + 12]              # witnesses 0 .. 15 are N+, N-, D+, D- of case 0
    n_bad, bad_rows, stuck, full = _solve(s, rows)
    hint_word = q.nr + 0                                                     # hint 0 is case 0's modular division
    assert stuck == [NONE, hint_word, NONE] and n_bad == [0, NONE, 0] and int(bad_rows[1][0]) == hint_word and int(bad_rows[1][1]) == NONE
    assert np.array_equal(full[0], want[0]) and np.array_equal(full[2], want[2])
    part = [(np.ascontiguousarray(rows[i, :q.m0]), np.ascontiguousarray(rows[i, q.m0:])) for i in range(3)]
    proofs, statuses, instances = s["pm"].prove_batch(s["pk"], part, [[71, 72], [73, 74], [75, 76]], solve=True)
    assert statuses == [0, PM_ERR_INVALID_ARG, 0] and instances == [assignments[0][0], None, assignments[2][0]] and not proofs[1]


class _WitnessModulus:
    """y = 1 / D mod P with D and P given witnesses of one limb: the modulus of the hint is a column, so an assignment can carry an
    even one.  Witnesses D, P, Z (hinted), y = Z by an ordinary row; the public input is y"""

    def __init__(self, D, P):
        self.D, self.P = D, P

    def generate_constraints(self, cs):
        from polymath_amd.polymath import ConstraintSystem
        one = ConstraintSystem.ONE
        cs.new_witness_variable(self.D)
        cs.new_witness_variable(self.P)
        Z = cs.new_witness_variable(pow(self.D, -1, self.P))
        y = cs.new_witness_variable(pow(self.D, -1, self.P))
        cs.enforce_constraint([(1, Z)], [(1, one)], [(1, y)])
        cs.enforce_constraint([(1, y)], [(1, one)], [(1, cs.new_input_variable(pow(self.D, -1, self.P)))])

    @staticmethod
    def hints(m0):
        return [{"op": "moddiv", "n": 64, "z": [m0 + 2], "Np": [], "Nm": [], "Dp": [m0], "Dm": [], "P": [m0 + 1]}]


@pytest.mark.parametrize("curve", BOTH)
def test_stuck_at_an_even_modulus(gpu_ctx, curve):
    """the modulus in a witness column: the middle assignment of 3 carries an even one"""
    r = CURVES[curve].r
    s = _declared(gpu_ctx, curve, ("witness modulus",), _WitnessModulus(5, 2 ** 61 - 1), 19700)
    q, f = s["q"], s["f"]
    assert (q.m0, q.mw, q.nr) == (2, 4, 2)
    moduli = [2 ** 61 - 1, 1000003 * 15, 2 ** 64 - 59]                       # a prime, a composite, a prime of 64 bits
    assignments = [([1, pow(7 + i, -1, P)], [7 + i, P, pow(7 + i, -1, P), pow(7 + i, -1, P)]) for i, P in enumerate(moduli)]
    want, rows = _rows(s, assignments, ([1, None], [0, 0, None, None]))
    assert np.array_equal(_solve(s, rows)[3], want)
    rows[1, q.m0 + 1] = f.fr_limbs([1000003 * 16]).reshape(4)
    n_bad, bad_rows, stuck, full = _solve(s, rows)
    assert stuck == [NONE, q.nr + 0, NONE] and n_bad == [0, NONE, 0] and int(bad_rows[1][0]) == q.nr + 0
    assert np.array_equal(full[0], want[0]) and np.array_equal(full[2], want[2])
    part = [(np.ascontiguousarray(rows[i, :q.m0]), np.ascontiguousarray(rows[i, q.m0:])) for i in range(3)]
    _, statuses, _ = s["pm"].prove_batch(s["pk"], part, [[71, 72], [73, 74], [75, 76]], solve=True)
    assert statuses == [0, PM_ERR_INVALID_ARG, 0]


# ---- 6. the refusals through the C ABI; redeclaration, clearing, an inert hint, mixed markers ---------------------------------------------------------------
@pytest.mark.parametrize("curve", BOTH)
def test_refusals_and_redeclaration(gpu_ctx, curve):
    from polymath_amd import api
    r = CURVES[curve].r
    circuit = _moddiv(86, 3, 2, 19800)
    s = _declared(gpu_ctx, curve, ("refusals",), circuit, 19800)
    pm, pk, q = s["pm"], s["pk"], s["q"]
    good = circuit.hints(q.m0)
    ncols = q.m0 + q.mw
    h = good[0]
    assert h["op"] == "moddiv" and "op" not in good[1]

    def refused(hints, text):
        rc = pk.set_hints(hints)
        message = pm.ctx.last_error()
        assert rc == PM_ERR_INVALID_ARG and text in message, (rc, message)

    variant = lambda **kw: [dict(h, **kw)]
    words = api.encode_hints(good)
    assert int(words[0]) == 3
    bad = words.copy(); bad[0] = 2
    refused(bad, "pm_pk_set_hints: hint 0: unknown opcode 2")
    bad = words.copy(); bad[8] = 2
    refused(bad, "pm_pk_set_hints: hint 0: unknown flags 2")
    refused(words[:-1], "pm_pk_set_hints: hint 3: the record is truncated")
    refused(words[:8], "pm_pk_set_hints: hint 0: the record is truncated")
    refused(variant(n=0), "hint 0: n = 0 is outside 1..128")
    refused(variant(n=129), "hint 0: n = 129 is outside 1..128")
    refused(variant(z=[]), "hint 0: kz = 0 is outside 1..16")
    refused(variant(z=list(range(1, 18))), "hint 0: kz = 17 is outside 1..16")
    refused(variant(literal=[1] * 17), "hint 0: kP = 17 is outside 1..16")
    refused(variant(Dp=[]), "hint 0: kDp = 0 is outside 1..32")
    refused(variant(Dp=list(range(1, 34))), "hint 0: kDp = 33 is outside 1..32")
    refused(variant(Np=list(range(1, 34))), "hint 0: kNp = 33 is outside 0..32")
    refused(variant(Nm=list(range(1, 34))), "hint 0: kNm = 33 is outside 0..32")
    refused(variant(Dm=list(range(1, 34))), "hint 0: kDm = 33 is outside 0..32")
    refused(variant(n=128, Np=list(range(1, 10))), "hint 0: n (kNp - 1) = 1024 is 1024 or more")
    refused(variant(n=128, Dm=list(range(1, 10))), "hint 0: n (kDm - 1) = 1024 is 1024 or more")
    refused(variant(n=128, literal=[1] * 5), "hint 0: n (kP - 1) = 512 is 512 or more")
    refused(variant(Dp=[ncols]), "hint 0: column %d is not below m0 + mw = %d" % (ncols, ncols))
    refused(variant(z=[0]), "hint 0: an output is column 0 (the constant one)")
    refused(variant(z=[h["z"][0]] * 2), "hint 0: output column %d is named twice" % h["z"][0])
    refused(variant(Nm=[h["z"][1]]), "hint 0: output column %d is an input of the hint as well" % h["z"][1])
    refused([h, dict(good[1], q=[h["z"][2]])], "hint 1: output column %d is an output of hint 0 as well" % h["z"][2])
    refused([good[1], dict(h, z=[good[1]["rem"][0]])], "hint 1: output column %d is an output of hint 0 as well" % good[1]["rem"][0])
    refused(variant(literal=[3, r]), "hint 0: literal limb 1 is not below r")
    # a sharded key: refused whatever the declaration says, and freed here
    from polymath_amd import polymath as PM
    half = pm.setup((PM.R1CS(q.m0, q.mw, q.a, q.b, q.c), s["inst"], s["wit"]), 123, 456, 0, 2)
    assert half.set_hints(good) == PM_ERR_INVALID_ARG and "pm_pk_set_hints: hints on a sharded key are not supported" in pm.ctx.last_error()
    half.free()
    # the key is unchanged by all of them: the first declaration still completes the witness
    circuits = [_moddiv(86, 3, 2, 19810 + i) for i in range(3)]
    assignments, partial = [ci.native(r) for ci in circuits], circuit.partial(r)
    want = _completes(s, assignments, partial)
    # some outputs given and some marked; a special marker on an output
    _, rows = _rows(s, assignments, partial)
    mixed = rows.copy()
    mixed[:, h["z"][0]] = want[:, h["z"][0]]
    xs, ws = np.ascontiguousarray(mixed[:, :q.m0]), np.ascontiguousarray(mixed[:, q.m0:])
    assert pk.r1cs_check_batch(xs, ws, 2, solve=True)[0] == PM_ERR_INVALID_ARG and "pm solve: hint 0: some outputs are marked unknown and some are given" in pm.ctx.last_error()
    mixed = rows.copy()
    mixed[:, good[2]["z"][1]] = api.QUOTIENT_LIMBS
    xs, ws = np.ascontiguousarray(mixed[:, :q.m0]), np.ascontiguousarray(mixed[:, q.m0:])
    assert pk.r1cs_check_batch(xs, ws, 2, solve=True)[0] == PM_ERR_INVALID_ARG and "pm solve: hint 2: an output carries the quotient, indicator or square-root marker" in pm.ctx.last_error()
    # a caller that supplies Z itself: the modular hints inert, the long divisions still active
    supplied = rows.copy()
    for hint in good:
        if hint.get("op") == "moddiv":
            supplied[:, hint["z"]] = want[:, hint["z"]]
    n_bad, _, stuck, full = _solve(s, supplied)
    assert n_bad == [0] * 3 and stuck == [NONE] * 3 and np.array_equal(full, want)
    # cleared: nothing determines Z, and the plan made under the declaration is not reused ...
    assert pk.set_hints([]) == PM_OK
    xs, ws = np.ascontiguousarray(rows[:, :q.m0]), np.ascontiguousarray(rows[:, q.m0:])
    assert pk.r1cs_check_batch(xs, ws, 2, solve=True)[0] == PM_ERR_INVALID_ARG and "in any row order" in pm.ctx.last_error()
    # ... a modular hint whose denominator is its own check's quotient never becomes ready, and the refusal names it and its input ...
    assert pk.set_hints([dict(h, Dp=[good[1]["q"][0]])] + good[1:]) == PM_OK
    assert pk.r1cs_check_batch(xs, ws, 2, solve=True)[0] == PM_ERR_INVALID_ARG
    assert "pm solve: hint 0: input column %d is never determined; column " % good[1]["q"][0] in pm.ctx.last_error(), pm.ctx.last_error()
    # ... and declared again it completes again
    pm.set_hints(pk, good)
    assert np.array_equal(_completes(s, assignments, partial), want)
