"""The batch prover's glue mode is a flag of the boundary, not a new entry point: pm_prove_glue (0 / 256) is declared in the header,
quoted by the -sys crate and by api.PROVE_GLUE_DEVICE, OR-ed into the `transcript` argument of pm_host_prove_batch alone; the pinned
counts of the boundary (70 entry points, 9 options) hold; the argument checks need no device."""
import ctypes as ct
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUST_SYS = os.path.join(ROOT, "rust", "polymath-hip-sys", "src", "lib.rs")
RUST_WRAPPER = os.path.join(ROOT, "rust", "polymath-hip", "src", "lib.rs")
PM_ERR_INVALID_ARG = 1


def _header():
    return open(os.path.join(ROOT, "include", "polymath_hip.h")).read()


def test_enum_in_header_sys_crate_and_python():
    from polymath_amd import api
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"typedef\s+enum\s+pm_prove_glue\s*\{([^}]*)\}\s*pm_prove_glue\s*;", code)
    assert m, "pm_prove_glue is not declared in include/polymath_hip.h"
    values = {k: int(v) for k, v in re.findall(r"\b(PM_[A-Z0-9_]+)\s*=\s*(\d+)", m.group(1))}
    assert values == {"PM_PROVE_GLUE_HOST": 0, "PM_PROVE_GLUE_DEVICE": 256}
    consts = {k: int(v) for k, v in re.findall(r"pub const (PM_PROVE_GLUE_[A-Z]+): i32 = (\d+);", open(RUST_SYS).read())}
    assert consts == values
    assert api.PROVE_GLUE_DEVICE == 256 and api.PROVE_GLUE_HOST == 0 and api.PROVE_GLUE == {"host": 0, "device": 256}
    assert "sys::PM_PROVE_GLUE_DEVICE" in open(RUST_WRAPPER).read()


def test_documented_in_the_header():
    text = _header()
    assert "PM_PROVE_GLUE_DEVICE" in text and re.search(r"\*\s+11 \(no proof in flight needed\)", text), "flag and tap 11 are documented"
    before_single = text[:text.index("int pm_host_prove(")]
    assert "pm_prove_glue flag below belongs to pm_host_prove_batch alone" in before_single      # the other entry points keep refusing it


def test_pinned_counts_hold():
    from polymath_amd import api
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert len(set(re.findall(r"\b(pm_[a-z0-9_]+)\s*\(", code))) == 70 == len(api.EXPORTS)
    assert re.search(r"\bPM_NUM_OPTIONS\s*=\s*9\b", code)
    flags = re.search(r"typedef\s+enum\s+pm_assignment_flags\s*\{([^}]*)\}", code).group(1)
    assert sorted(int(v) for v in re.findall(r"=\s*(\d+)", flags)) == [1, 2]


def test_python_wrappers_take_the_mode():
    import inspect
    from polymath_amd import api
    from polymath_amd.polymath import Polymath
    assert inspect.signature(api.ProvingKey.host_prove_batch).parameters["glue"].default == "host"
    assert inspect.signature(Polymath.prove_batch).parameters["glue"].default == "host"
    assert hasattr(api.ProvingKey, "glue_challenges")


def _lib():
    from polymath_amd import api
    if not os.path.exists(api.LIB_PATH):
        pytest.skip("library not built")
    return api.load_library()


def test_transcript_word_is_validated_without_a_device():
    """bits outside 255 | 256, and a value of the low byte that is no pm_transcript, are refused before anything is read or written;
    the handles are zeroed memory that an implementation reading past the check would find to be no usable key"""
    L = _lib()
    zeros = (ct.c_uint64 * 8192)()
    fake = ct.c_void_p(ct.addressof(zeros))
    words = (ct.c_uint64 * 8)()
    buf, status = ct.create_string_buffer(176), (ct.c_int * 1)(-1)
    for transcript in (256 | 3, 256 | 7, 512, 256 | 1024):
        rc = L.pm_host_prove_batch(fake, fake, transcript, 1, words, ct.cast(words, ct.c_void_p), ct.cast(words, ct.c_void_p), 0, words, buf, 176, status)
        assert rc == PM_ERR_INVALID_ARG, transcript
    for ctx, pk in ((None, None), (None, fake), (fake, None)):     # a valid word and a NULL handle
        rc = L.pm_host_prove_batch(ctx, pk, 256 | 0, 1, words, ct.cast(words, ct.c_void_p), ct.cast(words, ct.c_void_p), 0, words, buf, 176, status)
        assert rc == PM_ERR_INVALID_ARG
    assert status[0] == -1 and buf.raw == bytes(176)


def test_single_prover_refuses_the_flag_without_a_device():
    L = _lib()
    words = (ct.c_uint64 * 8)()
    buf, n = ct.create_string_buffer(176), ct.c_size_t(77)
    rc = L.pm_host_prove(None, None, 256, words, ct.cast(words, ct.c_void_p), ct.cast(words, ct.c_void_p), 0, words, buf, 176, ct.byref(n))
    assert rc == PM_ERR_INVALID_ARG and n.value == 77 and buf.raw == bytes(176)
