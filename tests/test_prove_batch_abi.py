"""The batch prover is part of the boundary: declared in the header, listed in api.EXPORTS with a ctypes stub of the same arity,
exported by the built library, wrapped by ProvingKey.host_prove_batch / Polymath.prove_batch; its argument checks need no device."""
import ctypes as ct
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "pm_host_prove_batch"
PM_ERR_INVALID_ARG = 1


def test_declared_in_header_and_python_exports():
    from polymath_amd import api
    from polymath_amd.polymath import Polymath
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "polymath_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % SYMBOL, header)
    assert m, "not declared in include/polymath_hip.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 12 and args[3].startswith("size_t") and args[10].startswith("size_t") and args[11].startswith("int *")   # count, proof_len, status
    assert SYMBOL in api.EXPORTS
    assert hasattr(api.ProvingKey, "host_prove_batch") and hasattr(Polymath, "prove_batch")


def test_exported_with_a_stub_of_the_headers_arity():
    from polymath_amd import api
    if not os.path.exists(api.LIB_PATH):
        pytest.skip("library not built")
    out = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT\s+%s$" % SYMBOL, out, flags=re.M), "not exported by libpolymath_hip.so"
    L = api.load_library()
    assert len(L.pm_host_prove_batch.argtypes) == 12


def test_argument_validation_needs_no_device():
    from polymath_amd import api
    if not os.path.exists(api.LIB_PATH):
        pytest.skip("library not built")
    L = api.load_library()
    words = (ct.c_uint64 * 8)()
    buf, status = ct.create_string_buffer(176), (ct.c_int * 1)(-1)
    fake = ct.c_void_p(ct.addressof(words))           # never dereferenced: the other handle is NULL
    for ctx, pk, transcript in ((None, None, 0), (None, fake, 0), (fake, None, 0), (None, None, 7), (fake, None, 7)):
        rc = L.pm_host_prove_batch(ctx, pk, transcript, 1, words, ct.cast(words, ct.c_void_p), ct.cast(words, ct.c_void_p), 0, words, buf, 176, status)
        assert rc == PM_ERR_INVALID_ARG, (ctx, pk, transcript)
    assert status[0] == -1 and buf.raw == bytes(176)
