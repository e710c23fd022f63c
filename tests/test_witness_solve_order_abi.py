"""Rows in any order are new meaning under PM_ASSIGNMENT_SOLVE and nothing else: the pinned counts (70 entry points, PM_NUM_OPTIONS = 9,
two assignment flags, ten status values) hold in the header, in api.py and in the Rust -sys crate; the header documents the rule and
the root-cause stuck row where it documents the flag; and polymath_amd.circuits.Reordered emits a generator's rows in another order
with the generator's own variables and values, which satisfy the reordered rows on Python integers.  No device."""
import os
import re

import pytest

from oracle.pyref.fields import CURVES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "polymath_hip.h")


def test_the_pinned_counts_still_hold():
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert len(set(re.findall(r"\b(pm_[a-z0-9_]+)\s*\(", code))) == 70
    assert re.search(r"\bPM_NUM_OPTIONS\s*=\s*9\b", code)
    assert dict(re.findall(r"\b(PM_ASSIGNMENT_[A-Z]+)\s*=\s*(\d+)", code)) == {"PM_ASSIGNMENT_DEVICE": "1", "PM_ASSIGNMENT_SOLVE": "2"}
    status = re.search(r"typedef enum pm_status \{(.*?)\} pm_status;", code, flags=re.S).group(1)
    assert [int(v) for v in re.findall(r"=\s*(\d+)", status)] == list(range(10))
    from polymath_amd import api
    assert len(api.EXPORTS) == 70 and (api.ASSIGNMENT_DEVICE, api.ASSIGNMENT_SOLVE) == (1, 2) and len(api.OPTIONS) == 9
    sys_rs = open(os.path.join(ROOT, "rust", "polymath-hip-sys", "src", "lib.rs")).read()
    assert dict(re.findall(r"pub const (PM_ASSIGNMENT_[A-Z]+): i32 = (\d+);", sys_rs)) == {"PM_ASSIGNMENT_DEVICE": "1", "PM_ASSIGNMENT_SOLVE": "2"}
    block = re.sub(r"//[^\n]*", "", sys_rs)
    assert len(set(re.findall(r"pub fn (pm_[a-z0-9_]+)", block[block.index('extern "C" {'):]))) == 70


def test_header_documents_the_rule_and_the_root_cause():
    text = open(HEADER).read()
    doc = text[text.index("partial assignments: flags"):text.index("pm_assignment_flags;")]
    for needle in ("ANY ROW ORDER", "Rows in any order", "waiting-row scheduler", "DEPENDENCY order", "WAITS", "in any row order: ", "ROOT CAUSE",
                   "lowest dependency level, then smallest index", "a closer examined before its opener", "per-assignment patterns", "sharded keys"):
        assert needle in doc, needle
    assert "are not looked for: that decomposition row is refused" not in doc          # booleanity rows after the decomposition complete now
    wrapper = open(os.path.join(ROOT, "rust", "polymath-hip", "src", "lib.rs")).read()
    assert "waiting-row" in wrapper and "ROOT CAUSE" in wrapper
    plan = open(os.path.join(ROOT, "polymath_amd", "host", "solve_plan.hpp")).read()
    for needle in ("build_plan_any_order", "a closer examined BEFORE its opener", "K2 = lambda K1", "a known rest beside m", "over two matrices", "per-assignment patterns",
                   "sharded keys"):
        assert needle in plan, needle


def _rows_hold(r, q, instance, witness):
    z = list(instance) + list(witness)
    dot = lambda row: sum(v * z[j] for v, j in row) % r
    return [i for i in range(q.nr) if dot(q.a[i]) * dot(q.b[i]) % r != dot(q.c[i])]


def _synthesize(circuit, r):
    from polymath_amd.polymath import ConstraintSystem
    cs = ConstraintSystem(r)
    circuit.generate_constraints(cs)
    return cs.to_r1cs(), list(cs.instance), list(cs.witness)


def test_row_order():
    from polymath_amd import circuits as PC
    assert PC.row_order(5, "reverse") == [4, 3, 2, 1, 0]
    assert PC.row_order(7, "reverse", blocks=3) == [6, 3, 4, 5, 0, 1, 2]              # whole blocks move, the short last one too
    assert PC.row_order(6, [2, 0, 1], blocks=2) == [4, 5, 0, 1, 2, 3]
    for seed in (0, 1, 99):
        perm = PC.row_order(50, seed)
        assert sorted(perm) == list(range(50)) and perm != list(range(50)) and perm == PC.row_order(50, seed)
        blocks = PC.row_order(50, seed, blocks=4)
        assert sorted(blocks) == list(range(50)) and all(blocks[i + 1] == blocks[i] + 1 for i in range(49) if blocks[i] % 4 != 3 and blocks[i] != 49)
    assert PC.row_order(50, 1) != PC.row_order(50, 2)
    for bad in ("sorted", [0, 0, 1], [0, 1]):
        with pytest.raises(ValueError):
            PC.row_order(3, bad)


@pytest.mark.parametrize("curve", sorted(CURVES))
def test_reordered_circuits_satisfy_their_own_rows(curve):
    from polymath_amd import circuits as PC
    r = CURVES[curve].r
    g = PC.SplitMix64(77)
    hits = [True, False, True, True, False]
    cases = [(PC.MiMCDemo(g.fr(r), g.fr(r), [g.fr(r) for _ in range(6)]), 1),
             (PC.RangeCheck([5, 200, 0, 255], 8), 1),
             (PC.ArxDemo(0x1234, 0xBEEF, 16, 2, 5), 1),
             (PC.MatchCount([7, 9, 7, 0], 7, "ark"), 3),
             (PC.MatchCount([7, 9, 7, 0], 7, "circom"), 2),
             (PC.EqChain(3, PC.eq_chain_targets(3, hits, r), "ark", bits=6), 4 + 7),
             (PC.EqChain(3, PC.eq_chain_targets(3, hits, r), "circom"), 3)]
    for inner, blocks in cases:
        q0, inst0, wit0 = _synthesize(inner, r)
        assert _rows_hold(r, q0, inst0, wit0) == []
        for order in ("reverse", 3, 4):
            circuit = PC.Reordered(inner, order, blocks=blocks)
            q, inst, wit = _synthesize(circuit, r)
            perm = PC.row_order(q0.nr, order, blocks)
            assert (q.m0, q.mw, q.nr) == (q0.m0, q0.mw, q0.nr) and (inst, wit) == (inst0, wit0)          # variables in the inner order
            assert (q.a, q.b, q.c) == ([q0.a[i] for i in perm], [q0.b[i] for i in perm], [q0.c[i] for i in perm]) and perm != list(range(q0.nr))
            assert _rows_hold(r, q, inst, wit) == []
            wrong = list(wit)
            wrong[-1] = (wrong[-1] + 1) % r
            assert _rows_hold(r, q, inst, wrong) != []
            if hasattr(inner, "partial"):
                assert circuit.partial(r) == inner.partial(r)
        if hasattr(inner, "native"):
            args = () if isinstance(inner, PC.RangeCheck) else (r,)
            assert PC.Reordered(inner, "reverse").native(*args) == inner.native(*args)
    # generating into a system that already holds variables keeps them apart
    from polymath_amd.polymath import ConstraintSystem
    cs = ConstraintSystem(r)
    cs.new_witness_variable(42)
    cs.new_input_variable(43)
    PC.Reordered(PC.RangeCheck([5], 3), "reverse").generate_constraints(cs)
    q = cs.to_r1cs()
    assert (q.m0, q.mw, q.nr) == (2, 1 + 4, 4) and cs.witness == [42, 5, 1, 0, 1] and _rows_hold(r, q, cs.instance, cs.witness) == []
    assert q.c[0] == [(1, 4), (2, 5), (4, 6)]
