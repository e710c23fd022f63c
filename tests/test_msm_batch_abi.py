"""The batched resident MSM is part of the boundary: declared in the header, listed in api.EXPORTS, exported by the built library."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "pm_msm_g1_resident_batch"


def test_declared_in_header_and_python_exports():
    from polymath_amd import api
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "polymath_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % SYMBOL, header)
    assert m, "not declared in include/polymath_hip.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 9 and args[5].startswith("size_t") and args[6].startswith("size_t")      # len, batch
    assert SYMBOL in api.EXPORTS
    assert hasattr(api.Bases, "msm_batch")


def test_exported_by_the_built_library():
    from polymath_amd import api
    if not os.path.exists(api.LIB_PATH):
        pytest.skip("library not built")
    out = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT\s+%s$" % SYMBOL, out, flags=re.M), "not exported by libpolymath_hip.so"
