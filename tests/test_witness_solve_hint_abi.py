"""The boundary of the witness solver's declared hints, without a device.  The declaration is the call pm_pk_set_hints(ctx, pk, desc,
n_words) of the header's comment, carried by PM_KEY_HINTS, a flag of pm_pk_load_bytes' `validate` argument, because the set of entry
points is pinned: the flag and the opcode constants have the same values in the header, in api.py and in the Rust -sys crate; the
wrapper has a set_hints that passes the flag; no entry point, option, status value or marker was added; api.encode_hints writes the
record format the header states and api.decode_hints reads it back; the header and the planner document the rule, the refusals, the
stuck conditions and what is not handled; and the refusals that need no device are refused."""
import ctypes as ct
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "polymath_hip.h")


def _code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_the_flag_and_the_opcode_agree_across_the_boundary():
    code = _code()
    assert re.search(r"typedef enum pm_key_hints \{ PM_KEY_HINTS = 1024 \} pm_key_hints;", code)
    assert re.search(r"typedef enum pm_hint_op \{ PM_HINT_LONGDIV = 1 \} pm_hint_op;", code)
    assert re.search(r"typedef enum pm_hint_flags \{ PM_HINT_DIVISOR_LITERAL = 1 \} pm_hint_flags;", code)
    from polymath_amd import api
    assert (api.PM_KEY_HINTS, api.HINT_LONGDIV, api.HINT_DIVISOR_LITERAL) == (1024, 1, 1)
    assert api.PM_KEY_HINTS & (api.PM_WIRE_UNCOMPRESSED | api.PM_KEY_CHECK_RELATIONS | 1) == 0          # a bit of its own in `validate`
    assert api.HINT_LIMITS == {"n": 128, "kq": 32, "kr": 16, "kD": 32, "kE": 16}
    sys_rs = open(os.path.join(ROOT, "rust", "polymath-hip-sys", "src", "lib.rs")).read()
    for line in ("pub const PM_KEY_HINTS: i32 = 1024;", "pub const PM_HINT_LONGDIV: u64 = 1;", "pub const PM_HINT_DIVISOR_LITERAL: u64 = 1;"):
        assert line in sys_rs, line
    wrapper = open(os.path.join(ROOT, "rust", "polymath-hip", "src", "lib.rs")).read()
    body = wrapper[wrapper.index("pub fn set_hints(&mut self"):]
    body = body[:body.index("\n    }\n")]
    assert "Self::load_bytes_raw(" in body and "sys::PM_KEY_HINTS" in body and "8 * desc.len()" in body          # the wrapper's one call of pm_pk_load_bytes
    assert len(re.findall(r"sys::pm_pk_load_bytes\s*\(", wrapper)) == 1
    plan = open(os.path.join(ROOT, "polymath_amd", "host", "solve_plan.hpp")).read()
    for needle in ("KIND_LONGDIV = 11", "NUM_PLAN_KINDS = 12", "HINT_LONGDIV = 1, HINT_DIVISOR_LITERAL = 1", "HINT_MAX_N = 128, HINT_MAX_KD = 32, HINT_MAX_KE = 16, HINT_MAX_KQ = 32, HINT_MAX_KR = 16",
                   "HINT_D_BITS = 1024, HINT_E_BITS = 512"):
        assert needle in plan, needle


def test_nothing_else_was_added_to_the_boundary():
    """no entry point of its own, no option, no status value, no assignment flag, no marker, no environment variable"""
    code = _code()
    assert "pm_pk_set_hints" not in re.findall(r"\b(pm_[a-z0-9_]+)\s*\(", code)
    assert re.search(r"\bPM_NUM_OPTIONS\s*=\s*9\b", code)
    assert dict(re.findall(r"\b(PM_ASSIGNMENT_[A-Z]+)\s*=\s*(\d+)", code)) == {"PM_ASSIGNMENT_DEVICE": "1", "PM_ASSIGNMENT_SOLVE": "2"}
    status = re.search(r"typedef enum pm_status \{(.*?)\} pm_status;", code, flags=re.S).group(1)
    assert [int(v) for v in re.findall(r"=\s*(\d+)", status)] == list(range(10))
    assert len(re.findall(r"#define PM_(?:UNKNOWN|HINT)_[A-Z_]*(?:WORDS|MARKER) ", code)) == 4
    from polymath_amd import api
    assert "pm_pk_set_hints" not in api.EXPORTS and len(api.OPTIONS) == 9
    for name in ("solve.hip", "solve_steps.cuh"):
        assert "getenv" not in open(os.path.join(ROOT, "polymath_amd", "csrc", name)).read()
    assert "getenv" not in open(os.path.join(ROOT, "polymath_amd", "host", "solve_plan.hpp")).read()


def test_header_and_plan_document_the_rule():
    text = " ".join(open(HEADER).read().replace("\n *", " ").split())
    unhandled = ("other opcodes (modular inverse, gcd, sorting)", "signed limbs", "dividends beyond 1024 bits (RSA-2048)", "hints on sharded keys",
                 "per-assignment declarations", "inferring a hint from rows")
    for needle in ("pm_pk_set_hints(ctx, pk, desc, n_words)", "PM_KEY_HINTS", "no entry point of its own", "PM_HINT_LONGDIV, n, kq, kr, kD, kE, flags",
                   "kE limb values of four words each", "0 is the constant one, then the instance, then the witness", "n outside 1..128",
                   "kD > 32, kE > 16, kq > 32, kr > 16, or any of them 0", "n (kD - 1) >= 1024 or n (kE - 1) >= 512", "a column >= m0 + mw", "an output that is column 0",
                   "an output named twice, or by two hints, or also an input of its own hint", "a literal limb >= r", "a sharded key", "n_words = 0 clears it",
                   "E = 0, D >= 2^1024, E >= 2^512, q >= 2^(n kq) or rem >= 2^(n kr)", "is nr + h, a value no row has", "rows[i][0]",
                   "hint h: input column c is never determined", "ACTIVE when all its outputs carry PM_UNKNOWN_WORDS", "INERT when all are given") + unhandled:
        assert needle in text, needle
    plan = " ".join(open(os.path.join(ROOT, "polymath_amd", "host", "solve_plan.hpp")).read().replace("\n//", " ").split())
    for needle in ("declared hint", "HINT-OWNED", "KIND_LONGDIV", "E = 0, D >= 2^1024, E >= 2^512, q >= 2^(n kq), rem >= 2^(n kr)", "nr + h",
                   "hint h: input column c is never determined") + unhandled:
        assert needle in plan, needle


def test_encoding_round_trip():
    from polymath_amd import api
    hints = [{"n": 64, "q": [10, 11, 12, 13], "rem": [14, 15, 16, 17], "D": [3, 4, 5, 6, 7, 8, 9], "literal": [2 ** 64 - 1, 5, 0, (1 << 255) + 12345]},
             {"n": 86, "q": [30], "rem": [31, 32], "D": [20, 21], "E": [22, 23, 24]}]
    words = api.encode_hints(hints)
    assert words.dtype == np.uint64
    assert [int(v) for v in words[:7]] == [1, 64, 4, 4, 7, 4, 1] and [int(v) for v in words[7:22]] == list(range(10, 18)) + list(range(3, 10))
    assert [int(v) for v in words[22:26]] == [2 ** 64 - 1, 0, 0, 0] and [int(v) for v in words[34:38]] == [12345, 0, 0, 1 << 63]
    second = 7 + 15 + 16
    assert [int(v) for v in words[second:]] == [1, 86, 1, 2, 2, 3, 0, 30, 31, 32, 20, 21, 22, 23, 24] and len(words) == second + 15
    assert api.decode_hints(words) == hints
    # tuples: (n, q, rem, D, E) and (n, q, rem, D, None, literal)
    assert np.array_equal(api.encode_hints([(64, [10, 11, 12, 13], [14, 15, 16, 17], [3, 4, 5, 6, 7, 8, 9], None, hints[0]["literal"]), (86, [30], [31, 32], [20, 21], [22, 23, 24])]), words)
    assert len(api.encode_hints([])) == 0
    for bad in ({"n": 8, "q": [1], "rem": [2], "D": [3]}, {"n": 8, "q": [1], "rem": [2], "D": [3], "E": [4], "literal": [5]}, {"n": 8, "q": [1], "rem": [2], "D": [3], "literal": [1 << 256]}):
        with pytest.raises(ValueError):
            api.encode_hints([bad])


def test_refusals_that_need_no_device():
    """PM_KEY_HINTS without a context, without a key behind `out`, without `out`: PM_ERR_INVALID_ARG before anything is touched"""
    from polymath_amd import api
    L = api.load_library()
    words = api.encode_hints([(64, [3], [4], [1], [2])])
    data, size = words.ctypes.data_as(ct.c_void_p), words.size * 8
    key = ct.c_void_p(None)
    fake = ct.c_void_p(8)
    assert L.pm_pk_load_bytes(None, 0, data, size, api.PM_KEY_HINTS, 0, 1, 0, ct.byref(key)) == 1
    assert L.pm_pk_load_bytes(fake, 0, data, size, api.PM_KEY_HINTS, 0, 1, 0, ct.byref(key)) == 1 and key.value is None      # no key to declare for
    assert L.pm_pk_load_bytes(fake, 0, data, size, api.PM_KEY_HINTS, 0, 1, 0, None) == 1
