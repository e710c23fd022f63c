"""PM_ASSIGNMENT_SOLVE is part of the boundary without widening it: two flags of an existing argument and two tap numbers.  The header
defines the flags and documents the taps, the pinned counts (70 entry points, PM_NUM_OPTIONS = 9, the pm_status values) still hold,
the -sys crate carries the same constants and the safe wrapper passes them; the flag check comes before any handle is read and
needs no device."""
import ctypes as ct
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PM_OK, PM_ERR_INVALID_ARG = 0, 1
HEADER = os.path.join(ROOT, "include", "polymath_hip.h")


def _code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_defines_the_flags_and_documents_the_taps():
    code, text = _code(), open(HEADER).read()
    flags = dict(re.findall(r"\b(PM_ASSIGNMENT_[A-Z]+)\s*=\s*(\d+)", code))
    assert flags == {"PM_ASSIGNMENT_DEVICE": "1", "PM_ASSIGNMENT_SOLVE": "2"}
    tap = text[text.index("Debug / parity taps"):text.index("int pm_prove_tap")]
    for needle in (" 9 ", "10 ", "PM_ASSIGNMENT_SOLVE", "stuck row", "1 + m0", "m0 + mw", "PM_ERR_STATE", "pm_ctx_destroy"):
        assert needle in tap, needle
    for needle in ("UINT64_MAX", "column 0", "assignment 0", "PM_ERR_INVALID_ARG", "pm_last_timings"):
        assert needle in text[text.index("partial assignments: flags"):text.index("pm_assignment_flags;")], needle


def test_the_pinned_counts_still_hold():
    code = _code()
    assert len(set(re.findall(r"\b(pm_[a-z0-9_]+)\s*\(", code))) == 70
    assert re.search(r"\bPM_NUM_OPTIONS\s*=\s*9\b", code)
    status = re.search(r"typedef enum pm_status \{(.*?)\} pm_status;", code, flags=re.S).group(1)
    assert [int(v) for v in re.findall(r"=\s*(\d+)", status)] == list(range(10))
    from polymath_amd import api
    assert len(api.EXPORTS) == 70 and (api.ASSIGNMENT_DEVICE, api.ASSIGNMENT_SOLVE) == (1, 2)
    assert api.UNKNOWN_LIMBS == (2 ** 64 - 1,) * 4
    from polymath_amd import polymath as PM
    from oracle.pyref.fields import CURVES
    assert all(sum(v << (64 * k) for k, v in enumerate(PM.UNKNOWN)) >= c.r for c in CURVES.values())     # never a field element
    for name in ("solve_batch", "partial_limbs"):
        assert hasattr(PM.Polymath, name)
    for name in ("solve_results", "solved_assignments"):
        assert hasattr(api.ProvingKey, name)


def test_rust_side_carries_the_same_constants():
    sys_rs = open(os.path.join(ROOT, "rust", "polymath-hip-sys", "src", "lib.rs")).read()
    consts = dict(re.findall(r"pub const (PM_ASSIGNMENT_[A-Z]+): i32 = (\d+);", sys_rs))
    assert consts == {"PM_ASSIGNMENT_DEVICE": "1", "PM_ASSIGNMENT_SOLVE": "2"}
    block = re.sub(r"//[^\n]*", "", sys_rs)
    assert len(set(re.findall(r"pub fn (pm_[a-z0-9_]+)", block[block.index('extern "C" {'):]))) == 70        # no new extern function
    wrapper = open(os.path.join(ROOT, "rust", "polymath-hip", "src", "lib.rs")).read()
    assert "pub fn prove_batch_from_partial" in wrapper and "pub fn solve" in wrapper
    assert "sys::PM_ASSIGNMENT_SOLVE" in wrapper and re.search(r"sys::pm_prove_tap\([^;]*\b9\b", wrapper)


def test_flag_check_needs_no_device():
    from polymath_amd import api
    L = api.load_library()
    words = (ct.c_uint64 * 12)(*([7] * 12))
    n_bad = (ct.c_uint64 * 1)(99)
    status = (ct.c_int * 1)(55)
    length = ct.c_size_t(66)
    buf = ct.create_string_buffer(b"M" * 176, 176)
    fake = ct.c_void_p(ct.addressof(words))           # never dereferenced: the flag word is refused first, or the other handle is NULL
    vp = ct.cast(words, ct.c_void_p)
    for flags in (4, 5, 6, 7, 8, 1 << 16, -1):
        assert L.pm_r1cs_check(fake, fake, vp, vp, flags, 1, n_bad, words, words) == PM_ERR_INVALID_ARG
        assert L.pm_r1cs_check_batch(fake, fake, 1, vp, vp, flags, 1, n_bad, words, words) == PM_ERR_INVALID_ARG
        assert L.pm_host_prove(fake, fake, 0, words, vp, vp, flags, words, buf, 176, ct.byref(length)) == PM_ERR_INVALID_ARG
        assert L.pm_host_prove_batch(fake, fake, 0, 1, words, vp, vp, flags, words, buf, 176, status) == PM_ERR_INVALID_ARG
    for flags in (2, 3):                               # the new modes with NULL handles
        for ctx, pk in ((None, None), (None, fake), (fake, None)):
            assert L.pm_r1cs_check(ctx, pk, vp, vp, flags, 1, n_bad, words, words) == PM_ERR_INVALID_ARG
            assert L.pm_r1cs_check_batch(ctx, pk, 1, vp, vp, flags, 1, n_bad, words, words) == PM_ERR_INVALID_ARG
            assert L.pm_host_prove_batch(ctx, pk, 0, 1, words, vp, vp, flags, words, buf, 176, status) == PM_ERR_INVALID_ARG
        assert L.pm_host_prove(None, None, 0, words, vp, vp, flags, words, buf, 176, ct.byref(length)) == PM_ERR_INVALID_ARG
        assert L.pm_host_prove(fake, None, 0, words, vp, vp, flags, words, buf, 176, ct.byref(length)) == PM_ERR_INVALID_ARG
    assert n_bad[0] == 99 and list(words) == [7] * 12 and status[0] == 55 and length.value == 66 and buf.raw == b"M" * 176
    out, n = (ct.c_uint64 * 8)(), ct.c_size_t(0)
    for which in (9, 10):
        assert L.pm_prove_tap(None, which, out, 2, ct.byref(n)) == PM_ERR_INVALID_ARG
