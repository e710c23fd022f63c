"""The quotient marker is a constant of the boundary and nothing else is new there: PM_UNKNOWN_QUOTIENT_WORDS has the same four words in
the header, in api.py (the ctypes stub's module) and in the Rust -sys crate, the wrapper re-exports it, and both markers are >= r on
both curves; the pinned counts (70 entry points, PM_NUM_OPTIONS = 9, two assignment flags, ten status values) hold; no getenv was
added; the header documents the rule.  Polymath.partial_limbs writes the marker for polymath.QUOTIENT; DivRem and ModChain satisfy
their own rows on Python integers, in order and under Reordered, native() is what generate_constraints writes, and partial() marks
exactly the quotients.  No device."""
import os
import re

import numpy as np
import pytest

from oracle.pyref.fields import CURVES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "polymath_hip.h")
U64 = (1 << 64) - 1
QUOTIENT_WORDS = (U64 - 1, U64, U64, U64)


def _c_words(text):
    return tuple(eval(w.replace("UINT64_MAX", str(U64))) for w in text.split(","))


def test_the_marker_agrees_across_the_boundary():
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    defines = dict(re.findall(r"#define (PM_UNKNOWN[A-Z_]*WORDS) \{([^}]*)\}", code))
    assert {k: _c_words(v) for k, v in defines.items()} == {"PM_UNKNOWN_WORDS": (U64,) * 4, "PM_UNKNOWN_QUOTIENT_WORDS": QUOTIENT_WORDS}
    assert code.index("pm_assignment_flags;") < code.index("#define PM_UNKNOWN_QUOTIENT_WORDS") < code.index("pm_host_prove(")      # next to the flags
    from polymath_amd import api, polymath as PM
    assert api.QUOTIENT_LIMBS == QUOTIENT_WORDS and api.UNKNOWN_LIMBS == (U64,) * 4
    assert PM.QUOTIENT is api.QUOTIENT_LIMBS and PM.UNKNOWN is api.UNKNOWN_LIMBS
    sys_rs = open(os.path.join(ROOT, "rust", "polymath-hip-sys", "src", "lib.rs")).read()
    rust = dict(re.findall(r"pub const (PM_UNKNOWN[A-Z_]*WORDS): \[u64; 4\] = \[([^\]]*)\];", sys_rs))
    to_words = lambda text: tuple(eval(w.replace("u64::MAX", str(U64))) for w in text.split(","))
    assert {k: to_words(v) for k, v in rust.items()} == {"PM_UNKNOWN_WORDS": (U64,) * 4, "PM_UNKNOWN_QUOTIENT_WORDS": QUOTIENT_WORDS}
    wrapper = open(os.path.join(ROOT, "rust", "polymath-hip", "src", "lib.rs")).read()
    assert "pub const UNKNOWN_QUOTIENT: [u64; 4] = sys::PM_UNKNOWN_QUOTIENT_WORDS;" in wrapper
    value = sum(w << (64 * i) for i, w in enumerate(QUOTIENT_WORDS))
    assert all(value >= c.r for c in CURVES.values())


def test_the_pinned_counts_still_hold():
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert len(set(re.findall(r"\b(pm_[a-z0-9_]+)\s*\(", code))) == 70
    assert re.search(r"\bPM_NUM_OPTIONS\s*=\s*9\b", code)
    assert dict(re.findall(r"\b(PM_ASSIGNMENT_[A-Z]+)\s*=\s*(\d+)", code)) == {"PM_ASSIGNMENT_DEVICE": "1", "PM_ASSIGNMENT_SOLVE": "2"}
    status = re.search(r"typedef enum pm_status \{(.*?)\} pm_status;", code, flags=re.S).group(1)
    assert [int(v) for v in re.findall(r"=\s*(\d+)", status)] == list(range(10))
    from polymath_amd import api
    assert len(api.EXPORTS) == 70 and (api.ASSIGNMENT_DEVICE, api.ASSIGNMENT_SOLVE) == (1, 2) and len(api.OPTIONS) == 9
    for name in ("solve.hip", "solve_steps.cuh", "divrem.cuh"):
        assert "getenv" not in open(os.path.join(ROOT, "polymath_amd", "csrc", name)).read()
    assert "getenv" not in open(os.path.join(ROOT, "polymath_amd", "host", "solve_plan.hpp")).read()


def test_header_and_plan_document_the_rule():
    text = open(HEADER).read()
    doc = text[text.index("partial assignments: flags"):text.index("pm_assignment_flags;")]
    for needle in ("a division row", "PM_UNKNOWN_QUOTIENT_WORDS", "q = floor(a / d),  rem = a mod d", "STUCK at row r", "nothing is inferred", "and no division row: ",
                   "cr != -cq; rem in A or B; rem named twice; the other side not known", "signed division", "marks one with the other marker"):
        assert needle in doc, needle
    plan = open(os.path.join(ROOT, "polymath_amd", "host", "solve_plan.hpp")).read()
    for needle in ("KIND_DIVREM = 7", "NUM_STEP_KINDS = 8", "division row", "never registered as an opener", "signed division", "a known rest beside q"):
        assert needle in plan, needle


@pytest.mark.parametrize("curve", sorted(CURVES))
def test_partial_limbs_writes_the_marker(curve):
    from polymath_amd import api, polymath as PM
    f = PM.Field(curve)

    class Host:      # partial_limbs reads self.field only
        field = f
    x, w = PM.Polymath.partial_limbs(Host(), [1, None], [5, PM.QUOTIENT, None, PM.UNKNOWN, 0])
    assert [tuple(int(v) for v in row) for row in w[1:4]] == [api.QUOTIENT_LIMBS, api.UNKNOWN_LIMBS, api.UNKNOWN_LIMBS]
    assert tuple(int(v) for v in x[1]) == api.UNKNOWN_LIMBS
    assert np.array_equal(w[[0, 4]], f.fr_limbs([5, 0]).reshape(2, 4)) and np.array_equal(x[0], f.fr_limbs([1]).reshape(4))


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
def test_division_circuits_satisfy_their_own_rows(curve):
    from polymath_amd import circuits as PC, polymath as PM
    r = CURVES[curve].r
    pairs = [(100, 7), (0, 1), (65535, 65535), (65534, 65535), (9, 9), (40000, 2)]
    cases = [(PC.DivRem(pairs, 16), len(pairs)), (PC.DivRem([((1 << 250) - 1, (1 << 192) + 1), (1 << 64, 1 << 64)], 250), 2), (PC.ModChain(3, 1103515245, 12345, 1 << 31, 6), 6),
             (PC.ModChain(3, 5, 7, 11, 5, bits=6), 5)]
    for circuit, quotients in cases:
        q, inst, wit = _synthesize(circuit, r)
        assert _rows_hold(r, q, inst, wit) == []
        assert circuit.native(r) == (inst, wit)
        p_inst, p_wit = circuit.partial(r)
        assert p_inst == [1, None] and sum(v is PM.QUOTIENT for v in p_wit) == quotients and len(p_wit) == len(wit)
        assert all(v is None or v is PM.QUOTIENT or v == wit[j] for j, v in enumerate(p_wit))
        # the quotient's row: q alone in A, a given divisor in B, the remainder in C with coefficient -1
        for j, v in enumerate(p_wit):
            if v is not PM.QUOTIENT:
                continue
            col = q.m0 + j
            rows = [i for i in range(q.nr) if q.a[i] == [(1, col)] and len(q.b[i]) == 1 and q.b[i][0][1] != 0]
            assert len(rows) == 1 and (r - 1) in [coef for coef, _ in q.c[rows[0]]]
        wrong = list(wit)
        wrong[p_wit.index(PM.QUOTIENT)] += 1
        assert _rows_hold(r, q, inst, wrong) != []
        for order in ("reverse", 5):
            q2, inst2, wit2 = _synthesize(PC.Reordered(circuit, order), r)
            assert (inst2, wit2) == (inst, wit) and _rows_hold(r, q2, inst2, wit2) == [] and PC.Reordered(circuit, order).partial(r) == (p_inst, p_wit)
    assert PC.DivRem(pairs, 16).native(r)[0][1] == sum(sum(divmod(a, b)) for a, b in pairs)
    chain = PC.ModChain(3, 1103515245, 12345, 1 << 31, 6)
    assert chain.native(r)[0][1] == PC.mod_chain_native(3, 1103515245, 12345, 1 << 31, 6)
    # b = 0 has no assignment: zeros are written, and the division row does not hold
    q, inst, wit = _synthesize(PC.DivRem([(5, 0)], 4), r)
    assert wit[2:4] == [0, 0] and (3 * 4) in _rows_hold(r, q, inst, wit)
