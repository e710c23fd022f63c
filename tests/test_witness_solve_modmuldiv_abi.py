"""The boundary of the witness solver's declared MODULAR MULTIPLY-DIVIDE hints, without a device.  The record travels in the
declaration that PM_KEY_HINTS of pm_pk_load_bytes carries, beside the three earlier records: its opcode and its limits have the same
values in the header, in api.py, in the Rust -sys crate and in host/solve_plan.hpp; nothing was added to the boundary's pinned counts
and the pinned lines of the earlier records stand; api.encode_hints / decode_hints round-trip the new dictionary form, mixed with the
others, and keep the words of opcodes 1, 3 and 5 byte for byte; the header and the planner document the rule, the refusals, the stuck
conditions and what is still not handled, and the sentences that were there before are intact.

Fails without the feature: the constant, the dictionary form and the sentences do not exist before this record."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "polymath_hip.h")
PLAN = os.path.join(ROOT, "polymath_amd", "host", "solve_plan.hpp")


def _code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_the_constants_agree_across_the_boundary():
    code = _code()
    assert "typedef enum pm_hint_op_muldiv { PM_HINT_MODMULDIV = 7 } pm_hint_op_muldiv;" in code
    # the pinned lines of the earlier records are as they were
    for line in ("typedef enum pm_hint_op { PM_HINT_LONGDIV = 1 } pm_hint_op;", "typedef enum pm_hint_flags { PM_HINT_DIVISOR_LITERAL = 1 } pm_hint_flags;",
                 "typedef enum pm_key_hints { PM_KEY_HINTS = 1024 } pm_key_hints;", "typedef enum pm_hint_op_modular { PM_HINT_MODDIV = 3 } pm_hint_op_modular;",
                 "typedef enum pm_hint_moddiv_flags { PM_HINT_MODULUS_LITERAL = 1 } pm_hint_moddiv_flags;", "typedef enum pm_hint_op_wide { PM_HINT_LONGDIV_WIDE = 5 } pm_hint_op_wide;"):
        assert line in code, line
    from polymath_amd import api
    assert api.HINT_MODMULDIV == 7 and (api.HINT_LONGDIV, api.HINT_MODDIV, api.HINT_LONGDIV_WIDE, api.HINT_MODULUS_LITERAL, api.PM_KEY_HINTS) == (1, 3, 5, 1, 1024)
    assert api.MODMULDIV_LIMITS == {"n": 128, "kz": 16, "kA": 32, "kB": 32, "kNp": 32, "kNm": 32, "kDp": 32, "kDm": 32, "kP": 16, "c": 2 ** 32 - 1}
    assert api.MODDIV_LIMITS == {"n": 128, "kz": 16, "kNp": 32, "kNm": 32, "kDp": 32, "kDm": 32, "kP": 16}
    sys_rs = open(os.path.join(ROOT, "rust", "polymath-hip-sys", "src", "lib.rs")).read()
    for line in ("pub const PM_HINT_MODMULDIV: u64 = 7;", "pub const PM_HINT_MODDIV: u64 = 3;", "pub const PM_HINT_LONGDIV_WIDE: u64 = 5;", "pub const PM_HINT_LONGDIV: u64 = 1;"):
        assert line in sys_rs, line
    # every constant of the -sys crate is an enumerator of the header with the same value, and the reverse
    enums = {k: int(v) for k, v in re.findall(r"\b(PM_HINT_[A-Z0-9_]+)\s*=\s*(\d+)", code)}
    consts = {k: int(v) for k, v in re.findall(r"pub const (PM_HINT_[A-Z0-9_]+): u64 = (\d+);", sys_rs)}
    assert consts == enums and enums["PM_HINT_MODMULDIV"] == 7
    plan = open(PLAN).read()
    for needle in ("KIND_LONGDIV = 11, KIND_MODDIV = 12, KIND_LONGDIV_WIDE = 13, KIND_MODMULDIV = 14", "NUM_PLAN_KINDS = 12", "NUM_HINT_KINDS = 13", "NUM_WIDE_KINDS = 14",
                   "NUM_MULDIV_KINDS = 15", "HINT_MODMULDIV = 7, MODMULDIV_MAX_C = 0xffffffffull", "MODMULDIV_LISTS = 6", "HINT_MODDIV = 3, HINT_MODULUS_LITERAL = 1",
                   "MODDIV_MAX_KZ = 16, MODDIV_MAX_KP = 16, MODDIV_MAX_K = 32, MODDIV_OPERAND_BITS = 1024, MODDIV_MODULUS_BITS = 512", "HINT_LONGDIV_WIDE = 5",
                   "LAUNCH_LONGDIV_WIDE, LAUNCH_MODMULDIV };", "{LAUNCH_MODMULDIV, 0, 0},  // KIND_MODMULDIV"):
        assert needle in plan, needle


def test_the_pinned_counts_hold():
    """70 entry points, nine options, ten status values, two assignment flags, four marker macros: the record added none"""
    code = _code()
    from polymath_amd import api
    assert len(api.EXPORTS) == 70 and len(set(api.EXPORTS)) == 70 and "pm_pk_set_hints" not in api.EXPORTS and len(api.OPTIONS) == 9
    assert len(set(re.findall(r"\b(pm_[a-z0-9_]+)\s*\(", code))) == 70
    assert re.search(r"\bPM_NUM_OPTIONS\s*=\s*9\b", code)
    assert dict(re.findall(r"\b(PM_ASSIGNMENT_[A-Z]+)\s*=\s*(\d+)", code)) == {"PM_ASSIGNMENT_DEVICE": "1", "PM_ASSIGNMENT_SOLVE": "2"}
    status = re.search(r"typedef enum pm_status \{(.*?)\} pm_status;", code, flags=re.S).group(1)
    assert [int(v) for v in re.findall(r"=\s*(\d+)", status)] == list(range(10))
    assert len(re.findall(r"#define PM_(?:UNKNOWN|HINT)_[A-Z_]*(?:WORDS|MARKER) ", code)) == 4
    for name in ("solve.hip", "solve_steps.cuh"):
        assert "getenv" not in open(os.path.join(ROOT, "polymath_amd", "csrc", name)).read()


def test_header_and_plan_document_the_rule():
    text = " ".join(open(HEADER).read().replace("\n *", " ").split())
    for needle in ("PM_HINT_MODMULDIV, n, kz, kA, kB, kNp, kNm, kDp, kDm, kP, flags, cN, cD,",
                   "kz output columns, kA + kB factor columns, kNp + kNm addend columns, kDp + kDm denominator columns, then kP modulus columns",
                   "with PM_HINT_MODULUS_LITERAL (flags bit 0, the literal flag of opcode 3), kP limb values of four words each",
                   "the unique Z in [0, P) with cD (D+ - D-) Z = cN (A B + N+ - N-) (mod P)", "one-word literals in 1 .. 2^32 - 1", "A = B = X, D+ = Y, cN = 3, cD = 2",
                   "A and B may name the same columns", "kDp = kDm = 0 means D = 1", "kNp = kNm = 0 means no addend", "opcodes 2, 4 and 6 are refused as unknown, and so is 8",
                   "kA or kB outside 1..32", "kNp, kNm, kDp or kDm above 32", "kDm > 0 with kDp = 0", "n (k - 1) >= 1024 for any of the six operand lists", "n (kP - 1) >= 512",
                   "cN or cD outside 1 .. 2^32 - 1", "Records of all four opcodes may be mixed in one declaration", "any of the six list sums is >= 2^1024",
                   "gcd(cD D mod P, P) != 1", "a cD that shares a factor with a composite P", "the literals scale residues, after the reductions",
                   "curves with a != 0", "the numerator 3 X^2 + a is N+ = a", "complete addition formulas", "windowed or GLV scalar multiplication",
                   "PM_HINT_MODDIV itself is not touched",
                   # the sentences that were there before
                   "PM_HINT_MODDIV, n, kz, kNp, kNm, kDp, kDm, kP, flags", "kNp = kNm = 0 means N = 1", "the unique Z in [0, P) with Z D = N (mod P)", "opcode 2 stays reserved",
                   "the slope of a doubling as one hint (its numerator is a product)", "PM_HINT_LONGDIV_WIDE, n, kq, kr, kD, kE, flags", "opcodes 2 and 4 are refused as unknown",
                   "Records of all three opcodes may be mixed", "other opcodes (modular inverse, gcd, sorting)", "ACTIVE / INERT / mixed-marker rule", "STUCK at the word nr + h"):
        assert needle in text, needle
    plan = " ".join(open(PLAN).read().replace("\n//", " ").split())
    for needle in ("multiply-divide hint", "KIND_MODMULDIV", "HINT_MODMULDIV = 7", "LAUNCH_MODMULDIV", "Launch::inv_rounds = 2 L", "min(512, n (kP - 1) + 256)",
                   "the trip count of the product's reduction as well", "gcd(cD D mod P, P) != 1", "cN and cD scale AFTER the reductions", "after its wide ones",
                   "km[6] = kA, kB, kNp, kNm, kDp, kDm", "k[4] stays zero: opcode 3 alone",
                   # the sentences that were there before
                   "the slope of a doubling as one hint (3 X^2 / 2 Y: the numerator is a product)", "P even or P < 3, P >= 2^512, N+, N-, D+ or D- >= 2^1024, gcd(D mod P, P) != 1",
                   "k[4] = kNp, kNm, kDp, kDm, the parts of D", "wide hint", "modular hint"):
        assert needle in plan, needle
    steps = open(os.path.join(ROOT, "polymath_amd", "csrc", "solve_steps.cuh")).read()
    assert "solve_modmuldiv" in steps and "NINE PHASES" in steps and "THE BOUND" in steps and "after 2 L rounds u = 0" in steps
    kernels = open(os.path.join(ROOT, "polymath_amd", "csrc", "solve.hip")).read()
    assert "k_solve_modmuldiv" in kernels and "case pmsolve::LAUNCH_MODMULDIV:" in kernels


def test_encoding_round_trip():
    from polymath_amd import api
    longdiv = [{"n": 64, "q": [10, 11, 12, 13], "rem": [14, 15, 16, 17], "D": [3, 4, 5, 6, 7, 8, 9], "literal": [2 ** 64 - 1, 5, 0, (1 << 255) + 12345]},
               {"op": "longdiv_wide", "n": 86, "q": [30], "rem": [31, 32], "D": [20, 21], "E": [22, 23, 24]}]
    moddiv = [{"op": "moddiv", "n": 64, "z": [40, 41], "Np": [1, 2], "Nm": [3], "Dp": [4, 5], "Dm": [6], "P": [7, 8]}]
    muldiv = [{"op": "modmuldiv", "n": 64, "z": [50, 51], "A": [1, 2], "B": [1, 2], "Np": [], "Nm": [], "Dp": [3, 4], "Dm": [], "cN": 3, "cD": 2, "P": [7, 8]},
              {"op": "modmuldiv", "n": 86, "z": [60], "A": [1], "B": [2, 3], "Np": [4], "Nm": [5, 6], "Dp": [], "Dm": [], "cN": 2 ** 32 - 1, "cD": 1, "literal": [3, (1 << 200) + 1]}]
    # the words of opcodes 1, 5 and 3 are what they were, byte for byte
    words = api.encode_hints(longdiv)
    assert [int(v) for v in words[:7]] == [1, 64, 4, 4, 7, 4, 1] and [int(v) for v in words[38:]] == [5, 86, 1, 2, 2, 3, 0, 30, 31, 32, 20, 21, 22, 23, 24]
    assert [int(v) for v in api.encode_hints(moddiv)] == [3, 64, 2, 2, 1, 2, 1, 2, 0, 40, 41, 1, 2, 3, 4, 5, 6, 7, 8]
    # the new record
    words = api.encode_hints(muldiv)
    assert words.dtype == np.uint64
    assert [int(v) for v in words[:23]] == [7, 64, 2, 2, 2, 0, 0, 2, 0, 2, 0, 3, 2, 50, 51, 1, 2, 1, 2, 3, 4, 7, 8]
    assert [int(v) for v in words[23:43]] == [7, 86, 1, 1, 2, 1, 2, 0, 0, 2, 1, 2 ** 32 - 1, 1, 60, 1, 2, 3, 4, 5, 6] and [int(v) for v in words[43:]] == [3, 0, 0, 0, 1, 0, 0, 1 << 8]
    assert api.decode_hints(words) == muldiv
    # the optional lists and literals: absent lists are empty, absent literals are 1
    assert np.array_equal(api.encode_hints([{"op": "modmuldiv", "n": 86, "z": [60], "A": [1], "B": [2, 3], "Np": [4], "Nm": [5, 6], "cN": 2 ** 32 - 1, "literal": [3, (1 << 200) + 1]}]), words[23:])
    # mixed, in both orders
    for mixed in ([longdiv[0], muldiv[0], moddiv[0], longdiv[1], muldiv[1]], [muldiv[1], longdiv[1], moddiv[0], longdiv[0], muldiv[0]]):
        assert api.decode_hints(api.encode_hints(mixed)) == mixed
    for bad in ({"op": "modmuldiv", "n": 8, "z": [1], "A": [2], "B": [3]}, {"op": "modmuldiv", "n": 8, "z": [1], "A": [2], "B": [3], "P": [4], "literal": [5]},
                {"op": "modmuldiv", "n": 8, "z": [1], "A": [2], "B": [3], "literal": [1 << 256]}, {"op": "modmuldiv", "n": 8, "z": [1], "A": [2], "B": [3], "P": [4], "cN": 0},
                {"op": "modmuldiv", "n": 8, "z": [1], "A": [2], "B": [3], "P": [4], "cD": 2 ** 32}, {"op": "gcd", "n": 8}):
        with pytest.raises(ValueError):
            api.encode_hints([bad])
    with pytest.raises(KeyError):
        api.encode_hints([{"op": "modmuldiv", "n": 8, "z": [1], "A": [2], "P": [3]}])          # a factor is not optional
    for opcode in (2, 4, 6, 8):
        with pytest.raises(ValueError):
            api.decode_hints(np.array([opcode, 64, 1, 1, 1, 1, 0, 1, 2, 3, 4], dtype=np.uint64))
