"""The boundary of the witness solver's square-root hint, without a device: the fourth marker (PM_HINT_SQRT_MARKER) has the same words in
the header, in api.py (the ctypes stub's module) and in the Rust -sys crate, the wrapper re-exports it, it is 2^256 - 1 - 2^192 and
>= r on both curves; nothing was added to the pinned sets (70 entry points, 9 options, 2 assignment flags, 10 status values); the
header and the planner document the rule and what it does not handle; partial_limbs writes the marker; and the two circuits that take
square roots (circuits.SquareRoots, EdwardsDecompress) satisfy their own rows on Python integers, in order and reordered, with native()
equal to what generate_constraints writes, partial() marking exactly the root columns, and every marked value the smaller root of its
row's C side."""
import os
import re

import numpy as np
import pytest

from oracle.pyref.fields import CURVES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "polymath_hip.h")
U64 = (1 << 64) - 1
SQRT_WORDS = (U64, U64, U64, U64 - 1)


def test_the_marker_agrees_across_the_boundary():
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    define = re.search(r"#define PM_HINT_SQRT_MARKER \{([^}]*)\}", code).group(1)
    assert tuple(eval(w.replace("UINT64_MAX", str(U64))) for w in define.split(",")) == SQRT_WORDS
    assert code.index("#define PM_HINT_INDICATOR_WORDS") < code.index("#define PM_HINT_SQRT_MARKER") < code.index("pm_host_prove(")      # next to the other three
    from polymath_amd import api, polymath as PM
    assert api.SQRT_LIMBS == SQRT_WORDS and PM.SQRT is api.SQRT_LIMBS
    assert len({api.UNKNOWN_LIMBS, api.QUOTIENT_LIMBS, api.INDICATOR_LIMBS, api.SQRT_LIMBS}) == 4
    assert len({id(PM.UNKNOWN), id(PM.QUOTIENT), id(PM.INDICATOR), id(PM.SQRT)}) == 4
    sys_rs = open(os.path.join(ROOT, "rust", "polymath-hip-sys", "src", "lib.rs")).read()
    rust = re.search(r"pub const PM_HINT_SQRT_MARKER: \[u64; 4\] = \[([^\]]*)\];", sys_rs).group(1)
    assert tuple(eval(w.replace("u64::MAX", str(U64))) for w in rust.split(",")) == SQRT_WORDS
    wrapper = open(os.path.join(ROOT, "rust", "polymath-hip", "src", "lib.rs")).read()
    assert "pub const HINT_SQRT: [u64; 4] = sys::PM_HINT_SQRT_MARKER;" in wrapper
    value = sum(w << (64 * i) for i, w in enumerate(SQRT_WORDS))
    assert value == (1 << 256) - 1 - (1 << 192) and all(value >= c.r for c in CURVES.values())


def test_the_pinned_counts_still_hold():
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert len(set(re.findall(r"\b(pm_[a-z0-9_]+)\s*\(", code))) == 70
    assert re.search(r"\bPM_NUM_OPTIONS\s*=\s*9\b", code)
    assert dict(re.findall(r"\b(PM_ASSIGNMENT_[A-Z]+)\s*=\s*(\d+)", code)) == {"PM_ASSIGNMENT_DEVICE": "1", "PM_ASSIGNMENT_SOLVE": "2"}
    status = re.search(r"typedef enum pm_status \{(.*?)\} pm_status;", code, flags=re.S).group(1)
    assert [int(v) for v in re.findall(r"=\s*(\d+)", status)] == list(range(10))
    from polymath_amd import api
    assert len(api.EXPORTS) == 70 and (api.ASSIGNMENT_DEVICE, api.ASSIGNMENT_SOLVE) == (1, 2) and len(api.OPTIONS) == 9
    for name in ("solve.hip", "solve_steps.cuh", "divrem.cuh", "sqrt.cuh"):
        assert "getenv" not in open(os.path.join(ROOT, "polymath_amd", "csrc", name)).read()


def test_header_and_plan_document_the_rule():
    text = open(HEADER).read()
    doc = text[text.index("partial assignments: flags"):text.index("pm_assignment_flags;")]
    unhandled = ("a known rest beside u on either side", "u in C_r (a general quadratic)", "the larger root", "arkworks' unspecified choice of root",
                 "inferring a square root without the marker", "sharded keys", "per-assignment patterns")
    for needle in ("a square-root row", "PM_HINT_SQRT_MARKER", "the smaller of the", "<= (r - 1) / 2", "c a non-residue", "STUCK at row r", "nothing is inferred",
                   "any two of the four markers differ") + unhandled:
        assert needle in doc, needle
    plan = open(os.path.join(ROOT, "polymath_amd", "host", "solve_plan.hpp")).read()
    for needle in ("KIND_SQRT = 9", "KIND_INDICATOR = 8", "KIND_DIVREM = 7", "NUM_STEP_KINDS = 8", "NUM_KINDS = 7", "NUM_SORT_KINDS = 10", "PATTERN_SQRT = 4",
                   "square-root row", "c a non-residue") + unhandled:
        assert needle in plan, needle
    # the marker test is stated once (divrem.cuh) and knows the fourth byte
    assert "PATTERN_SQRT" in open(os.path.join(ROOT, "polymath_amd", "csrc", "divrem.cuh")).read()


@pytest.mark.parametrize("curve", sorted(CURVES))
def test_partial_limbs_writes_the_marker(curve):
    from polymath_amd import api, polymath as PM
    f = PM.Field(curve)

    class Host:      # partial_limbs reads self.field only
        field = f
    x, w = PM.Polymath.partial_limbs(Host(), [1, PM.SQRT], [5, PM.SQRT, None, PM.QUOTIENT, PM.INDICATOR, PM.UNKNOWN, 0])
    assert [tuple(int(v) for v in row) for row in w[1:6]] == [api.SQRT_LIMBS, api.UNKNOWN_LIMBS, api.QUOTIENT_LIMBS, api.INDICATOR_LIMBS, api.UNKNOWN_LIMBS]
    assert tuple(int(v) for v in x[1]) == api.SQRT_LIMBS
    assert np.array_equal(w[[0, 6]], f.fr_limbs([5, 0]).reshape(2, 4)) and np.array_equal(x[0], f.fr_limbs([1]).reshape(4))


@pytest.mark.parametrize("curve", sorted(CURVES))
def test_python_square_roots(curve):
    from polymath_amd import polymath as PM
    r = CURVES[curve].r
    assert PM.small_sqrt(r, 0) == 0 and PM.small_sqrt(r, 1) == 1 and PM.small_sqrt(r, 4) == 2 and PM.small_sqrt(r, 25) == 5
    assert PM.small_sqrt(r, {"bls12_381": 7, "bn254": 5}[curve]) is None              # the generator
    i = PM.small_sqrt(r, r - 1)                                                        # r = 1 mod 4
    assert i is not None and i * i % r == r - 1 and i <= (r - 1) // 2
    for v in range(2, 60):
        c = pow(v, 5, r)
        z = PM.small_sqrt(r, c)
        assert (z is None) == (pow(c, (r - 1) // 2, r) == r - 1)
        assert z is None or (z * z % r == c and z <= (r - 1) // 2 and PM.small_sqrt(r, (r - z) ** 2 % r) == z)
    # a prime that is 3 mod 4 goes through the same routine
    assert PM.tonelli_shanks(23, 2) in (5, 18) and PM.tonelli_shanks(23, 5) is None


def _rows_hold(r, q, instance, witness):
    z = list(instance) + list(witness)
    dot = lambda row: sum(v * z[j] for v, j in row) % r
    return [i for i in range(q.nr) if dot(q.a[i]) * dot(q.b[i]) % r != dot(q.c[i])]


def _synthesize(circuit, r):
    from polymath_amd.polymath import ConstraintSystem
    cs = ConstraintSystem(r)
    circuit.generate_constraints(cs)
    return cs.to_r1cs(), list(cs.instance), list(cs.witness)


@pytest.mark.parametrize("curve", sorted(CURVES))
def test_square_root_circuits_satisfy_their_own_rows(curve):
    from polymath_amd import circuits as PC, polymath as PM
    r = CURVES[curve].r
    ys = PC.edwards_ys(r, 3)
    squares = [0, 1, 4, r - 1] + [pow(v, 2, r) for v in (3, r - 3, 1 << 200, 12345678901234567890)]
    cases = [(PC.SquareRoots([9]), 1), (PC.SquareRoots(squares), len(squares)), (PC.EdwardsDecompress(ys[:1], [1]), 1), (PC.EdwardsDecompress(ys, [0, 1, 1]), 3)]
    for circuit, roots in cases:
        q, inst, wit = _synthesize(circuit, r)
        assert _rows_hold(r, q, inst, wit) == []
        assert circuit.native(r) == (inst, wit)
        p_inst, p_wit = circuit.partial(r)
        assert p_inst == [1, None] and sum(v is PM.SQRT for v in p_wit) == roots and len(p_wit) == len(wit)
        assert all(v is None or v is PM.SQRT or v == wit[j] for j, v in enumerate(p_wit))
        # a root's row: the column alone in A and alone in B with coefficient 1, one known column in C; its value is the smaller root of that
        z = inst + wit
        for j, v in enumerate(p_wit):
            if v is not PM.SQRT:
                continue
            col = q.m0 + j
            rows = [i for i in range(q.nr) if q.a[i] == [(1, col)] and q.b[i] == [(1, col)]]
            assert len(rows) == 1 and len(q.c[rows[0]]) == 1 and q.c[rows[0]][0][1] != col
            c_side = sum(c * z[k] for c, k in q.c[rows[0]]) % r
            assert z[col] <= (r - 1) // 2 and z[col] * z[col] % r == c_side and z[col] == PM.small_sqrt(r, c_side)
        for order in ("reverse", 5):
            q2, inst2, wit2 = _synthesize(PC.Reordered(circuit, order), r)
            assert (inst2, wit2) == (inst, wit) and _rows_hold(r, q2, inst2, wit2) == [] and PC.Reordered(circuit, order).partial(r) == (p_inst, p_wit)
    # SquareRoots: the layout is c_i, u_i per value and the public input is the sum of the roots
    assert PC.SquareRoots([9, 25, 0]).native(r) == ([1, 8], [9, 3, 25, 5, 0, 0]) and PC.SquareRoots([9, 25, 0]).partial(r) == ([1, None], [9, PM.SQRT, 25, PM.SQRT, 0, PM.SQRT])
    # EdwardsDecompress: (x, y) lies on the curve, x = x0 or r - x0 as the sign says, and the bits recompose x0
    _, a, d = PC.EDWARDS[r]
    inst, wit = PC.EdwardsDecompress(ys, [0, 1, 1]).native(r)
    per, nb, total = 6 + r.bit_length() - 1, r.bit_length() - 1, 0
    assert len(wit) == 3 * per
    for pt, sign in enumerate([0, 1, 1]):
        y, sg, y2, u, x0, x = wit[pt * per:pt * per + 6]
        assert (y, sg) == (ys[pt], sign) and (a * x * x + y * y - 1 - d * x * x * y * y) % r == 0 and x == ((r - x0) % r if sign else x0) and 0 < x0 <= (r - 1) // 2
        assert sum(b << i for i, b in enumerate(wit[pt * per + 6:(pt + 1) * per])) == x0 and x0 < 1 << nb
        total += x
    assert inst == [1, total % r]
