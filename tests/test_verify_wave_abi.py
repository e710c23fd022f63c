"""CPU: PM_VERIFY_PAIRING_DEVICE_WAVE at every layer of the boundary -- a value of pm_verify_batch2's `pairing` argument and nothing
else new there.  The header's enum, api.VERIFY_PAIRING, the -sys crate and the Rust wrapper carry the value 4; it is disjoint from
PM_VERIFY_CHALLENGES_DEVICE; api.verify_batch hands the library 4 and 4 | 256 (seen by a stand-in library); the leaf threshold
VERIFY_WAVE_LEAF_MAX is the same number in api.py, in the source and in the header's text; the header states the contract; the pinned
counts (70 entry points, PM_NUM_OPTIONS = 9) hold.  No GPU."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "polymath_hip.h")


def _code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_wave_mode_value_at_every_layer():
    from polymath_amd import api
    enums = {k: int(v) for k, v in re.findall(r"\b(PM_[A-Z0-9_]+)\s*=\s*(\d+)", _code())}
    assert enums["PM_VERIFY_PAIRING_HOST"] == 0 and enums["PM_VERIFY_PAIRING_DEVICE"] == 1 and enums["PM_VERIFY_PAIRING_DEVICE_WAVE"] == 4
    assert api.VERIFY_PAIRING == {"host": 0, "device": 1, "wave": 4}
    assert enums["PM_VERIFY_PAIRING_DEVICE_WAVE"] & enums["PM_VERIFY_CHALLENGES_DEVICE"] == 0
    assert all(v < 256 for v in api.VERIFY_PAIRING.values())                      # `pairing & 255` is the mode
    sys_rs = open(os.path.join(ROOT, "rust", "polymath-hip-sys", "src", "lib.rs")).read()
    consts = {k: int(v) for k, v in re.findall(r"pub const (PM_VERIFY_PAIRING_[A-Z_]+): i32 = (\d+);", sys_rs)}
    assert consts == {"PM_VERIFY_PAIRING_HOST": 0, "PM_VERIFY_PAIRING_DEVICE": 1, "PM_VERIFY_PAIRING_DEVICE_WAVE": 4}
    wrapper = open(os.path.join(ROOT, "rust", "polymath-hip", "src", "lib.rs")).read()
    body = re.search(r"pub fn verify_batch_wave_pairing\(.*?\n    \}\n", wrapper, flags=re.S).group(0)
    assert "sys::PM_VERIFY_PAIRING_DEVICE_WAVE" in body and "sys::PM_VERIFY_CHALLENGES_HOST" in body and "verify_batch_with" in body
    assert "pub fn verify_batch_device_pairing(" in wrapper                       # beside it, not instead of it


class _Lib:
    """stands in for the library: records the `pairing` argument (the 12th) of pm_verify_batch2"""

    def __init__(self):
        self.seen = []

    def pm_verify_batch2(self, *args):
        self.seen.append(args[11])
        return 0


class _Ctx:
    h = None

    def __init__(self):
        self.L = _Lib()

    def check(self, status):
        assert status == 0


def test_verify_batch_passes_wave_mode_in_the_pairing_argument():
    from polymath_amd import api
    ctx = _Ctx()
    proof = bytes(api.PROOF_BYTES[api.CURVE_IDS["bn254"]])
    pub = np.zeros((1, 1, 4), dtype=np.uint64)
    api.verify_batch(ctx, "bn254", "merlin", b"vk", pub, [proof], pairing="wave")
    api.verify_batch(ctx, "bn254", "merlin", b"vk", pub, [proof], pairing="wave", challenges="device")
    api.verify_batch(ctx, "bn254", "merlin", b"vk", pub, [proof])                  # the default stays the host mode
    assert ctx.L.seen == [4, 260, 0]
    with pytest.raises(KeyError):
        api.verify_batch(ctx, "bn254", "merlin", b"vk", pub, [proof], pairing="waves")
    import inspect
    from polymath_amd.polymath import Polymath
    assert inspect.signature(Polymath.verify_batch).parameters["pairing"].default == "host"


def test_leaf_threshold_is_one_constant():
    from polymath_amd import api
    csrc = os.path.join(ROOT, "polymath_amd", "csrc")
    defs = []
    for name in sorted(os.listdir(csrc)):
        defs += re.findall(r"constexpr\s+size_t\s+VERIFY_WAVE_LEAF_MAX\s*=\s*(\d+)\s*;", open(os.path.join(csrc, name)).read())
    assert defs == [str(api.VERIFY_WAVE_LEAF_MAX)], defs                          # defined once, mirrored in api.py
    text = open(HEADER).read()
    assert "VERIFY_WAVE_LEAF_MAX = %d" % api.VERIFY_WAVE_LEAF_MAX in text
    verify = open(os.path.join(csrc, "verify_batch.hip")).read()
    assert "live_total() <= VERIFY_WAVE_LEAF_MAX" in verify                       # the one place that takes the decision


def test_header_documents_the_contract():
    text = " ".join(open(HEADER).read().split())
    doc = text[text.index("PM_VERIFY_PAIRING_DEVICE_WAVE:"):text.index("typedef enum pm_verify_pairing")]
    for phrase in ("byte for byte", "*n_checks", "every refusal", "The root is always checked this way", "not a tuned one", "nothing written"):
        assert phrase in doc, phrase


def test_the_pinned_counts_still_hold():
    code = _code()
    assert len(set(re.findall(r"\b(pm_[a-z0-9_]+)\s*\(", code))) == 70
    assert re.search(r"\bPM_NUM_OPTIONS\s*=\s*9\b", code)
    from polymath_amd import api
    assert len(api.EXPORTS) == 70 and len(api.OPTIONS) == 9
