"""The indicator marker is a constant of the boundary and nothing else is new there: PM_HINT_INDICATOR_WORDS has the same four words in
the header, in api.py (the ctypes stub's module) and in the Rust -sys crate, the wrapper re-exports it, and it is >= r on both curves;
the pinned counts (70 entry points, PM_NUM_OPTIONS = 9, two assignment flags, ten status values) hold and the set of PM_UNKNOWN..WORDS
names is the two it was; the header and the planner document the rule.  Polymath.partial_limbs writes the marker for
polymath.INDICATOR; Decoder and TableWalk satisfy their own rows on Python integers, in order and under Reordered, native() is what
generate_constraints writes, partial() marks exactly the out columns, and an index out of range gives all zeros and success = 0.
No device."""
import os
import re

import numpy as np
import pytest

from oracle.pyref.fields import CURVES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "polymath_hip.h")
U64 = (1 << 64) - 1
INDICATOR_WORDS = (U64, U64 - 1, U64, U64)


def _c_words(text):
    return tuple(eval(w.replace("UINT64_MAX", str(U64))) for w in text.split(","))


def test_the_marker_agrees_across_the_boundary():
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    defines = dict(re.findall(r"#define (PM_[A-Z_]*WORDS) \{([^}]*)\}", code))
    assert {k: _c_words(v) for k, v in defines.items()} == {"PM_UNKNOWN_WORDS": (U64,) * 4, "PM_UNKNOWN_QUOTIENT_WORDS": (U64 - 1, U64, U64, U64),
                                                            "PM_HINT_INDICATOR_WORDS": INDICATOR_WORDS}
    assert sorted(set(re.findall(r"PM_UNKNOWN[A-Z_]*WORDS", code))) == ["PM_UNKNOWN_QUOTIENT_WORDS", "PM_UNKNOWN_WORDS"]
    assert code.index("#define PM_UNKNOWN_QUOTIENT_WORDS") < code.index("#define PM_HINT_INDICATOR_WORDS") < code.index("pm_host_prove(")      # next to the other two
    from polymath_amd import api, polymath as PM
    assert api.INDICATOR_LIMBS == INDICATOR_WORDS and PM.INDICATOR is api.INDICATOR_LIMBS
    assert len({api.UNKNOWN_LIMBS, api.QUOTIENT_LIMBS, api.INDICATOR_LIMBS}) == 3
    sys_rs = open(os.path.join(ROOT, "rust", "polymath-hip-sys", "src", "lib.rs")).read()
    rust = dict(re.findall(r"pub const (PM_[A-Z_]*WORDS): \[u64; 4\] = \[([^\]]*)\];", sys_rs))
    to_words = lambda text: tuple(eval(w.replace("u64::MAX", str(U64))) for w in text.split(","))
    assert to_words(rust["PM_HINT_INDICATOR_WORDS"]) == INDICATOR_WORDS and sorted(rust) == ["PM_HINT_INDICATOR_WORDS", "PM_UNKNOWN_QUOTIENT_WORDS", "PM_UNKNOWN_WORDS"]
    wrapper = open(os.path.join(ROOT, "rust", "polymath-hip", "src", "lib.rs")).read()
    assert "pub const HINT_INDICATOR: [u64; 4] = sys::PM_HINT_INDICATOR_WORDS;" in wrapper
    value = sum(w << (64 * i) for i, w in enumerate(INDICATOR_WORDS))
    assert value == (1 << 256) - 1 - (1 << 64) and all(value >= c.r for c in CURVES.values())


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
    for needle in ("an indicator row", "PM_HINT_INDICATOR_WORDS", "z_u = 1 where K z == 0, else 0", "never leaves an assignment stuck", "nothing is inferred",
                   "a hit value other than 1", "a non-empty C_r", "a known rest beside u", "inferring indicators without the marker", "sharded keys", "per-assignment patterns"):
        assert needle in doc, needle
    plan = open(os.path.join(ROOT, "polymath_amd", "host", "solve_plan.hpp")).read()
    for needle in ("KIND_INDICATOR = 8", "KIND_DIVREM = 7", "NUM_STEP_KINDS = 8", "NUM_KINDS = 7", "indicator row", "a hit value other than 1", "a known rest beside u"):
        assert needle in plan, needle
    # the marker test is stated once (divrem.cuh) and the two glue files ask it
    csrc = os.path.join(ROOT, "polymath_amd", "csrc")
    assert "marker_byte_limbs" in open(os.path.join(csrc, "host_prove.hip")).read() and "marker_byte<P>" in open(os.path.join(csrc, "prove_glue.hip")).read()


@pytest.mark.parametrize("curve", sorted(CURVES))
def test_partial_limbs_writes_the_marker(curve):
    from polymath_amd import api, polymath as PM
    f = PM.Field(curve)

    class Host:      # partial_limbs reads self.field only
        field = f
    x, w = PM.Polymath.partial_limbs(Host(), [1, PM.INDICATOR], [5, PM.INDICATOR, None, PM.QUOTIENT, PM.UNKNOWN, 0])
    assert [tuple(int(v) for v in row) for row in w[1:5]] == [api.INDICATOR_LIMBS, api.UNKNOWN_LIMBS, api.QUOTIENT_LIMBS, api.UNKNOWN_LIMBS]
    assert tuple(int(v) for v in x[1]) == api.INDICATOR_LIMBS
    assert np.array_equal(w[[0, 5]], f.fr_limbs([5, 0]).reshape(2, 4)) and np.array_equal(x[0], f.fr_limbs([1]).reshape(4))


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
def test_decoder_circuits_satisfy_their_own_rows(curve):
    from polymath_amd import circuits as PC, polymath as PM
    r = CURVES[curve].r
    table = [3, 0, 4, 1, 2]
    cases = [(PC.Decoder(1, 0), 1), (PC.Decoder(7, 0), 7), (PC.Decoder(7, 6), 7), (PC.Decoder(7, 3), 7), (PC.Decoder(7, 7), 7), (PC.Decoder(7, r - 1), 7),
             (PC.TableWalk(table, 2, 4), 20), (PC.TableWalk(table, 2, 4, signals=False), 20), (PC.TableWalk([1, 9, 0], 0, 4), 12)]
    for circuit, indicators in cases:
        q, inst, wit = _synthesize(circuit, r)
        assert _rows_hold(r, q, inst, wit) == []
        assert circuit.native(r) == (inst, wit)
        p_inst, p_wit = circuit.partial(r)
        assert p_inst == [1, None] and sum(v is PM.INDICATOR for v in p_wit) == indicators and len(p_wit) == len(wit)
        assert all(v is None or v is PM.INDICATOR or v == wit[j] for j, v in enumerate(p_wit))
        # an indicator's guard row: the column alone in A with coefficient 1, a known side in B, nothing in C; its value is 0 or 1, and
        # 1 exactly where the guard's known side is zero
        z = inst + wit
        for j, v in enumerate(p_wit):
            if v is not PM.INDICATOR:
                continue
            col = q.m0 + j
            rows = [i for i in range(q.nr) if q.a[i] == [(1, col)] and q.c[i] == [] and q.b[i]]
            assert len(rows) == 1 and all(p_wit[k - q.m0] is not PM.INDICATOR for _, k in q.b[rows[0]] if k >= q.m0)
            assert z[col] == int(sum(c * z[k] for c, k in q.b[rows[0]]) % r == 0)
        for order in ("reverse", 5):
            q2, inst2, wit2 = _synthesize(PC.Reordered(circuit, order), r)
            assert (inst2, wit2) == (inst, wit) and _rows_hold(r, q2, inst2, wit2) == [] and PC.Reordered(circuit, order).partial(r) == (p_inst, p_wit)
    # Decoder: partial() gives inp and marks exactly the out columns; the hit is where the index says
    inst, wit = PC.Decoder(7, 3).native(r)
    assert (inst, wit) == ([1, 1], [3, 0, 0, 0, 1, 0, 0, 0]) and PC.Decoder(7, 3).partial(r) == ([1, None], [3] + [PM.INDICATOR] * 7)
    # an index out of range: all zeros and success = 0 -- which satisfies the rows, so the value at a hit is a hint, not a consequence
    for index in (7, r - 1):
        assert PC.Decoder(7, index).native(r) == ([1, 0], [index] + [0] * 7)
    q, inst, wit = _synthesize(PC.Decoder(7, 3), r)
    assert _rows_hold(r, q, [1, 0], [3] + [0] * 7) == [] and _rows_hold(r, q, inst, [3, 0, 1, 0, 1, 0, 0, 0]) != []
    # TableWalk: the public output is the walk on plain integers; out of range reads 0
    assert PC.TableWalk(table, 2, 4).native(r)[0] == [1, PC.table_walk_native(table, 2, 4, r)] == [1, 2]
    assert PC.TableWalk(table, 2, 4, signals=False).native(r)[0] == [1, 2]
    assert PC.TableWalk([1, 9, 0], 0, 3).native(r)[0] == [1, 0] == [1, PC.table_walk_native([1, 9, 0], 0, 3, r)]      # 0 -> 1 -> 9 -> 0
    walk = PC.TableWalk(table, 2, 4)
    assert walk.partial(r)[1][:6] == [2] + table and PC.TableWalk(table, 2, 4, signals=False).partial(r)[1][:2] == [2, PM.INDICATOR]
