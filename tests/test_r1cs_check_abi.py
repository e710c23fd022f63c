"""pm_r1cs_check / pm_r1cs_check_batch are part of the boundary: declared in the header, exported by the built library, listed in
api.EXPORTS with ctypes stubs of the header's arity, declared by the -sys crate and wrapped above it; the argument checks that come
before any device work need no device."""
import ctypes as ct
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"pm_r1cs_check": 9, "pm_r1cs_check_batch": 10}
PM_OK, PM_ERR_INVALID_ARG = 0, 1


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "polymath_hip.h")).read(), flags=re.S)


def test_header_declares_both():
    header = _header()
    for name, arity in ARITY.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m, name + " is not declared in include/polymath_hip.h"
        args = [" ".join(a.split()) for a in m.group(1).split(",")]
        assert len(args) == arity, (name, args)
        assert args[0] == "pm_ctx *ctx" and args[1] == "const pm_pk *pk"
        assert args[-4:] == ["size_t max_rows", "uint64_t *n_bad", "uint64_t *rows", "uint64_t *abc"], (name, args)
    batch = re.search(r"\bint\s+pm_r1cs_check_batch\s*\(([^;]*)\)\s*;", header).group(1)
    assert " ".join(batch.split(",")[2].split()) == "size_t count"
    assert len(set(re.findall(r"\b(pm_[a-z0-9_]+)\s*\(", header))) == 70


def test_library_exports_both():
    from polymath_amd import api
    api.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ARITY:
        assert re.search(r"\bT\s+%s$" % name, out, flags=re.M), name + " is not exported by libpolymath_hip.so"
    assert len(re.findall(r"\bT\s+pm_[a-z0-9_]+$", out, flags=re.M)) == 70


def test_python_exports_with_the_headers_arity():
    from polymath_amd import api
    from polymath_amd.polymath import Polymath
    L = api.load_library()
    for name, arity in ARITY.items():
        assert name in api.EXPORTS
        assert len(getattr(L, name).argtypes) == arity, name
    assert len(api.EXPORTS) == len(set(api.EXPORTS)) == 70
    assert hasattr(api.ProvingKey, "r1cs_check") and hasattr(api.ProvingKey, "r1cs_check_batch")
    assert hasattr(Polymath, "check_assignment") and hasattr(Polymath, "check_batch")


def test_sys_crate_declares_both_and_the_wrapper_calls_one():
    sys_rs = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "rust", "polymath-hip-sys", "src", "lib.rs")).read())
    block = sys_rs[sys_rs.index('extern "C" {'):]
    for name, arity in ARITY.items():
        m = re.search(r"pub fn %s\s*\((.*?)\)\s*->\s*i32\s*;" % name, block, flags=re.S)
        assert m, name + " is not declared in rust/polymath-hip-sys/src/lib.rs"
        assert len(m.group(1).split(",")) == arity, name
    assert len(set(re.findall(r"pub fn (pm_[a-z0-9_]+)", block))) == 70
    wrapper = open(os.path.join(ROOT, "rust", "polymath-hip", "src", "lib.rs")).read()
    assert "pub fn check_assignment" in wrapper and "sys::pm_r1cs_check(" in wrapper


def test_argument_checks_need_no_device():
    from polymath_amd import api
    L = api.load_library()
    words = (ct.c_uint64 * 12)(*([7] * 12))
    n_bad = (ct.c_uint64 * 1)(99)
    fake = ct.c_void_p(ct.addressof(words))           # never dereferenced: the other handle is NULL
    vp = ct.cast(words, ct.c_void_p)
    for ctx, pk in ((None, None), (None, fake), (fake, None)):
        assert L.pm_r1cs_check(ctx, pk, vp, vp, 0, 1, n_bad, words, words) == PM_ERR_INVALID_ARG
        for count in (0, 1):
            assert L.pm_r1cs_check_batch(ctx, pk, count, vp, vp, 0, 1, n_bad, words, words) == PM_ERR_INVALID_ARG
    assert n_bad[0] == 99 and list(words) == [7] * 12
