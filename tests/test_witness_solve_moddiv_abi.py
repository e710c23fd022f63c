"""The boundary of the witness solver's declared MODULAR-DIVISION hints, without a device.  The record travels in the declaration that
PM_KEY_HINTS of pm_pk_load_bytes carries, beside the long-division record: its opcode, its flag and its limits have the same values
in the header, in api.py, in the Rust -sys crate and in host/solve_plan.hpp; nothing was added to the boundary's pinned counts and the
pinned lines of the long-division record stand; api.encode_hints / decode_hints round-trip both dictionary forms, mixed, and keep
the long-division words byte for byte; the header and the planner document the rule, the refusals, the stuck conditions and what is
still not handled."""
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
    assert re.search(r"typedef enum pm_hint_op_modular \{ PM_HINT_MODDIV = 3 \} pm_hint_op_modular;", code)
    assert re.search(r"typedef enum pm_hint_moddiv_flags \{ PM_HINT_MODULUS_LITERAL = 1 \} pm_hint_moddiv_flags;", code)
    # the pinned lines of the long-division record are as they were
    for line in ("typedef enum pm_hint_op { PM_HINT_LONGDIV = 1 } pm_hint_op;", "typedef enum pm_hint_flags { PM_HINT_DIVISOR_LITERAL = 1 } pm_hint_flags;",
                 "typedef enum pm_key_hints { PM_KEY_HINTS = 1024 } pm_key_hints;"):
        assert line in code, line
    from polymath_amd import api
    assert (api.HINT_MODDIV, api.HINT_MODULUS_LITERAL) == (3, 1) and (api.HINT_LONGDIV, api.HINT_DIVISOR_LITERAL, api.PM_KEY_HINTS) == (1, 1, 1024)
    assert api.MODDIV_LIMITS == {"n": 128, "kz": 16, "kNp": 32, "kNm": 32, "kDp": 32, "kDm": 32, "kP": 16}
    assert api.HINT_LIMITS == {"n": 128, "kq": 32, "kr": 16, "kD": 32, "kE": 16}
    sys_rs = open(os.path.join(ROOT, "rust", "polymath-hip-sys", "src", "lib.rs")).read()
    for line in ("pub const PM_HINT_MODDIV: u64 = 3;", "pub const PM_HINT_MODULUS_LITERAL: u64 = 1;", "pub const PM_HINT_LONGDIV: u64 = 1;"):
        assert line in sys_rs, line
    wrapper = open(os.path.join(ROOT, "rust", "polymath-hip", "src", "lib.rs")).read()
    assert "ModDiv {" in wrapper and "LongDiv {" in wrapper and "sys::PM_HINT_MODDIV" in wrapper and "sys::PM_HINT_LONGDIV" in wrapper
    assert len(re.findall(r"sys::pm_pk_load_bytes\s*\(", wrapper)) == 1
    plan = open(PLAN).read()
    for needle in ("KIND_LONGDIV = 11, KIND_MODDIV = 12", "NUM_PLAN_KINDS = 12", "NUM_HINT_KINDS = 13", "HINT_MODDIV = 3, HINT_MODULUS_LITERAL = 1",
                   "MODDIV_MAX_KZ = 16, MODDIV_MAX_KP = 16, MODDIV_MAX_K = 32, MODDIV_OPERAND_BITS = 1024, MODDIV_MODULUS_BITS = 512",
                   "HINT_LONGDIV = 1, HINT_DIVISOR_LITERAL = 1", "HINT_MAX_N = 128, HINT_MAX_KD = 32, HINT_MAX_KE = 16, HINT_MAX_KQ = 32, HINT_MAX_KR = 16",
                   "HINT_D_BITS = 1024, HINT_E_BITS = 512", "NUM_SORT_KINDS = 10 + 1"):
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
    for needle in ("PM_HINT_MODDIV, n, kz, kNp, kNm, kDp, kDm, kP, flags", "kz output columns, kNp + kNm numerator columns, kDp + kDm denominator columns, then kP modulus columns",
                   "with PM_HINT_MODULUS_LITERAL (flags bit 0), kP limb values of four words each", "kNp = kNm = 0 means N = 1", "the unique Z in [0, P) with Z D = N (mod P)",
                   "P need not be prime", "opcode 2 stays reserved", "kz outside 1..16 or kP outside 1..16", "kDp outside 1..32", "kNp, kNm or kDm above 32",
                   "n (k - 1) >= 1024 for an operand list", "n (kP - 1) >= 512", "they share the index h", "P is even or P < 3", "P >= 2^512", ">= 2^1024",
                   "gcd(D mod P, P) != 1", "Z >= 2^(n kz)", "STUCK at the word nr + h", "other opcodes (modular inverse, gcd, sorting)", "even moduli",
                   "operands beyond 1024 bits", "the slope of a doubling as one hint", "ACTIVE / INERT / mixed-marker rule"):
        assert needle in text, needle
    plan = " ".join(open(PLAN).read().replace("\n//", " ").split())
    for needle in ("modular hint", "KIND_MODDIV", "HINT_MODDIV = 3", "LAUNCH_MODDIV", "Launch::inv_rounds = 2 L", "min(512, n (kP - 1) + 256)",
                   "P even or P < 3, P >= 2^512, N+, N-, D+ or D- >= 2^1024, gcd(D mod P, P) != 1", "Z >= 2^(n kz)", "Step::row = nr + h",
                   "other opcodes (modular inverse, gcd, sorting)", "even moduli", "gcd, sorting"):
        assert needle in plan, needle
    steps = open(os.path.join(ROOT, "polymath_amd", "csrc", "solve_steps.cuh")).read()
    assert "THE BOUND" in steps and "after 2 L rounds u = 0" in steps        # the trip count is stated and proved where the loop is


def test_encoding_round_trip():
    from polymath_amd import api
    longdiv = [{"n": 64, "q": [10, 11, 12, 13], "rem": [14, 15, 16, 17], "D": [3, 4, 5, 6, 7, 8, 9], "literal": [2 ** 64 - 1, 5, 0, (1 << 255) + 12345]},
               {"n": 86, "q": [30], "rem": [31, 32], "D": [20, 21], "E": [22, 23, 24]}]
    moddiv = [{"op": "moddiv", "n": 64, "z": [40, 41], "Np": [1, 2], "Nm": [3], "Dp": [4, 5], "Dm": [6], "P": [7, 8]},
              {"op": "moddiv", "n": 86, "z": [50], "Np": [], "Nm": [], "Dp": [9], "Dm": [], "literal": [3, (1 << 200) + 1]}]
    # the long-division words are what they were before the second opcode, byte for byte
    words = api.encode_hints(longdiv)
    assert [int(v) for v in words[:7]] == [1, 64, 4, 4, 7, 4, 1] and [int(v) for v in words[38:]] == [1, 86, 1, 2, 2, 3, 0, 30, 31, 32, 20, 21, 22, 23, 24]
    assert api.decode_hints(words) == longdiv and all("op" not in h for h in api.decode_hints(words))
    assert np.array_equal(api.encode_hints([dict(h, op="longdiv") for h in longdiv]), words)
    # the new record
    words = api.encode_hints(moddiv)
    assert words.dtype == np.uint64
    assert [int(v) for v in words[:17]] == [3, 64, 2, 2, 1, 2, 1, 2, 0, 40, 41, 1, 2, 3, 4, 5, 6] and [int(v) for v in words[17:19]] == [7, 8]
    assert [int(v) for v in words[19:30]] == [3, 86, 1, 0, 0, 1, 0, 2, 1, 50, 9] and [int(v) for v in words[30:]] == [3, 0, 0, 0, 1, 0, 0, 1 << 8] and len(words) == 38
    assert api.decode_hints(words) == moddiv
    # the optional lists: without "Np" and "Nm" the numerator is 1, without "Dm" nothing is subtracted
    assert np.array_equal(api.encode_hints([{"op": "moddiv", "n": 86, "z": [50], "Dp": [9], "literal": [3, (1 << 200) + 1]}]), words[19:])
    # mixed, in both orders
    for mixed in ([longdiv[0], moddiv[0], longdiv[1], moddiv[1]], [moddiv[1], longdiv[1], longdiv[0], moddiv[0]]):
        assert api.decode_hints(api.encode_hints(mixed)) == mixed
    # the long-division refusals stand; the new form has its own
    for bad in ({"n": 8, "q": [1], "rem": [2], "D": [3]}, {"n": 8, "q": [1], "rem": [2], "D": [3], "E": [4], "literal": [5]}, {"n": 8, "q": [1], "rem": [2], "D": [3], "literal": [1 << 256]},
                {"op": "moddiv", "n": 8, "z": [1], "Dp": [2]}, {"op": "moddiv", "n": 8, "z": [1], "Dp": [2], "P": [3], "literal": [5]},
                {"op": "moddiv", "n": 8, "z": [1], "Dp": [2], "literal": [1 << 256]}, {"op": "gcd", "n": 8}):
        with pytest.raises(ValueError):
            api.encode_hints([bad])
    with pytest.raises(KeyError):
        api.encode_hints([{"op": "moddiv", "n": 8, "z": [1], "P": [3]}])          # a denominator is not optional
    with pytest.raises(ValueError):
        api.decode_hints(np.array([2, 64, 1, 1, 1, 1, 0, 1, 2, 3, 4], dtype=np.uint64))      # opcode 2 is reserved
