"""Is-zero pairs are new meaning under PM_ASSIGNMENT_SOLVE and nothing else: the pinned counts (70 entry points, PM_NUM_OPTIONS = 9,
two assignment flags, ten status values) hold in the header, in api.py and in the Rust -sys crate; the header documents the rule and
the m = 0 convention where it documents the flag; and the two circuits that carry the gadget (polymath_amd.circuits: MatchCount,
EqChain) exist, with assignments that satisfy their own rows on Python integers in both forms.  No device."""
import os
import re

import pytest

from oracle.pyref.fields import CURVES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "polymath_hip.h")
FORMS = ["ark", "circom"]


def _code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_the_pinned_counts_still_hold():
    code = _code()
    assert len(set(re.findall(r"\b(pm_[a-z0-9_]+)\s*\(", code))) == 70
    assert re.search(r"\bPM_NUM_OPTIONS\s*=\s*9\b", code)
    assert dict(re.findall(r"\b(PM_ASSIGNMENT_[A-Z]+)\s*=\s*(\d+)", code)) == {"PM_ASSIGNMENT_DEVICE": "1", "PM_ASSIGNMENT_SOLVE": "2"}
    status = re.search(r"typedef enum pm_status \{(.*?)\} pm_status;", code, flags=re.S).group(1)
    assert [int(v) for v in re.findall(r"=\s*(\d+)", status)] == list(range(10))
    from polymath_amd import api
    assert len(api.EXPORTS) == 70 and (api.ASSIGNMENT_DEVICE, api.ASSIGNMENT_SOLVE) == (1, 2)
    sys_rs = open(os.path.join(ROOT, "rust", "polymath-hip-sys", "src", "lib.rs")).read()
    assert dict(re.findall(r"pub const (PM_ASSIGNMENT_[A-Z]+): i32 = (\d+);", sys_rs)) == {"PM_ASSIGNMENT_DEVICE": "1", "PM_ASSIGNMENT_SOLVE": "2"}
    block = re.sub(r"//[^\n]*", "", sys_rs)
    assert len(set(re.findall(r"pub fn (pm_[a-z0-9_]+)", block[block.index('extern "C" {'):]))) == 70


def test_header_documents_the_pair_and_the_convention():
    text = open(HEADER).read()
    doc = text[text.index("partial assignments: flags"):text.index("pm_assignment_flags;")]
    for needle in ("is-zero pair", "opener", "closer", "K2 = K1 or -K1", "m = 0", "circom", "arkworks", "supplies m itself"):
        assert needle in doc, needle
    assert "Not solved: the is-zero" not in text
    wrapper = open(os.path.join(ROOT, "rust", "polymath-hip", "src", "lib.rs")).read()
    assert "is-zero" in wrapper and "m = 0" in wrapper


def _rows_hold(r, q, instance, witness):
    z = list(instance) + list(witness)
    dot = lambda row: sum(v * z[j] for v, j in row) % r
    return [i for i in range(q.nr) if dot(q.a[i]) * dot(q.b[i]) % r != dot(q.c[i])]


@pytest.mark.parametrize("curve", sorted(CURVES))
@pytest.mark.parametrize("form", FORMS)
def test_match_count_native_satisfies_its_rows(curve, form):
    from polymath_amd import circuits as PC
    from polymath_amd.polymath import ConstraintSystem
    r = CURVES[curve].r
    values = [7, r - 1, 7, 0, 8, 7 + r]
    for key, count in ((7, 3), (0, 1), (5, 0)):
        for free in (0, 1, 12345):
            circuit = PC.MatchCount(values, key, form, free=free)
            cs = ConstraintSystem(r)
            circuit.generate_constraints(cs)
            q = cs.to_r1cs()
            instance, witness = circuit.native(r)
            assert instance == [1, count] and (q.m0, q.mw) == (2, 1 + 3 * len(values))
            assert q.nr == {"ark": 3, "circom": 2}[form] * len(values) + 1
            assert _rows_hold(r, q, instance, witness) == []
            # per value: v, flag, multiplier; the free multiplier is `free` exactly where the value matches
            for i, v in enumerate(values):
                hit = (v - key) % r == 0
                flag, m = witness[2 + 3 * i], witness[3 + 3 * i]
                assert flag == int(hit if form == "circom" else not hit)
                assert m == (free if hit else pow((v - key) % r, r - 2, r))
            pi, pw = circuit.partial(r)
            assert pi == [1, None] and [j for j, v in enumerate(pw) if v is not None] == [0] + [1 + 3 * i for i in range(len(values))]
            assert [j for j, v in enumerate(circuit.partial(r, multipliers=True)[1]) if v is None] == [2 + 3 * i for i in range(len(values))]


@pytest.mark.parametrize("curve", sorted(CURVES))
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("bits", [0, 12])
def test_eq_chain_native_satisfies_its_rows(curve, form, bits):
    from polymath_amd import circuits as PC
    from polymath_amd.polymath import ConstraintSystem
    r = CURVES[curve].r
    hits = [True, False, False, True, True, False]
    targets = PC.eq_chain_targets(3, hits, r)
    assert targets == [3, 12, 13, 9, 19, 44]
    circuit = PC.EqChain(3, targets, form, bits=bits)
    cs = ConstraintSystem(r)
    circuit.generate_constraints(cs)
    q = cs.to_r1cs()
    instance, witness = circuit.native(r)
    assert instance == [1, 40] and _rows_hold(r, q, instance, witness) == []          # 3 -> 7 -> 8 -> 9 -> 19 -> 39 -> 40
    per_step = {"ark": 4, "circom": 3}[form] + (bits + 1 if bits else 0)
    assert q.nr == per_step * len(hits) and q.mw == 1 + (4 + bits) * len(hits) - 1
    pi, pw = circuit.partial(r)
    assert pi == [1, None] and sum(v is not None for v in pw) == 1 + len(hits)
    wrong = list(witness)
    wrong[2] ^= 1                                                                       # the first flag
    assert _rows_hold(r, q, instance, wrong) != []
