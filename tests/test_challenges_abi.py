"""CPU: PM_VERIFY_CHALLENGES_DEVICE at every layer of the boundary -- the header's enum, the ctypes side (api.py) and the -sys crate
carry the same values, the flag is disjoint from every pm_verify_pairing value it is OR-ed with, api.verify_batch hands the library
the OR of the two modes in pm_verify_batch2's `pairing` argument (seen by a stand-in library), and the timing slot has its name.
No GPU."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "polymath_hip.h")).read(), flags=re.S)


def test_challenge_mode_values():
    from polymath_amd import api
    enums = {k: int(v) for k, v in re.findall(r"\b(PM_[A-Z0-9_]+)\s*=\s*(\d+)", _header())}
    assert enums["PM_VERIFY_CHALLENGES_HOST"] == 0 and enums["PM_VERIFY_CHALLENGES_DEVICE"] == 256
    assert api.VERIFY_CHALLENGES == {"host": 0, "device": 256}
    for v in api.VERIFY_PAIRING.values():
        assert v & enums["PM_VERIFY_CHALLENGES_DEVICE"] == 0
    sys_rs = open(os.path.join(ROOT, "rust", "polymath-hip-sys", "src", "lib.rs")).read()
    consts = {k: int(v) for k, v in re.findall(r"pub const (PM_VERIFY_CHALLENGES_[A-Z]+): i32 = (\d+);", sys_rs)}
    assert consts == {"PM_VERIFY_CHALLENGES_HOST": 0, "PM_VERIFY_CHALLENGES_DEVICE": 256}
    assert api.VERIFY_TIMING_SLOTS["challenge_kernel"] == 6 and api.VERIFY_TIMING_SLOTS["host_glue"] == 3


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


def test_verify_batch_passes_both_modes_in_the_pairing_argument():
    from polymath_amd import api
    ctx = _Ctx()
    proof = bytes(api.PROOF_BYTES[api.CURVE_IDS["bn254"]])
    pub = np.zeros((1, 1, 4), dtype=np.uint64)
    api.verify_batch(ctx, "bn254", "merlin", b"vk", pub, [proof])                                  # the defaults: the parent's call
    api.verify_batch(ctx, "bn254", "merlin", b"vk", pub, [proof], pairing="device")
    api.verify_batch(ctx, "bn254", "merlin", b"vk", pub, [proof], challenges="device")
    api.verify_batch(ctx, "bn254", "merlin", b"vk", pub, [proof], pairing="device", challenges="device")
    assert ctx.L.seen == [0, 1, 256, 257]
    with pytest.raises(KeyError):
        api.verify_batch(ctx, "bn254", "merlin", b"vk", pub, [proof], challenges="gpu")
