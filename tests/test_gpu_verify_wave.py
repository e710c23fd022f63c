"""GPU: pm_verify_batch2 with PM_VERIFY_PAIRING_DEVICE_WAVE (api.verify_batch(..., pairing="wave")): every pairing check spread over a
group of lanes of one wave (csrc/pairing_wave.hip).  The contract is PM_VERIFY_PAIRING_DEVICE's, byte for byte, so device mode is the
reference for every verdict and count, and host mode and the host verifier (pm_host_verify) stand behind it: valid batches of 1, 2, 3
and 65 proofs; a mixed batch (tampered a_at_x1, a moved point, a_at_x1 = r, [d]_1 the canonical point at infinity so that the leaf
checks see -V = W = O) under two seeds and without verdicts; the leaf launch at live = 1, one wave's worth and one more; both sides of
VERIFY_WAVE_LEAF_MAX in one test; device challenges and the three transcripts; every refused `pairing` value with the outputs
untouched; and the same context in host and device mode afterwards.  The proofs are those of tests/verify_helpers.py (MiMC, 16
rounds), a handful of them tiled where a test needs many."""
import os
import re

import numpy as np
import pytest

from verify_helpers import CURVES2, G1N, _host_verdict, _key, _moved_point, _plus_one, _proofs, _run

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAVE_GROUP = int(re.search(r"constexpr int WAVE_GROUP = (\d+);", open(os.path.join(ROOT, "polymath_amd", "csrc", "pairing_wave.cuh")).read()).group(1))
PER_WAVE = 64 // WAVE_GROUP


def _tiled(curve, transcript, count, distinct=4):
    have = _proofs(curve, transcript, min(count, distinct))
    return [have[i % len(have)] for i in range(count)]


def _three_modes(curve, transcript, items, **kw):
    return {mode: _run(curve, transcript, items, pairing=mode, **kw) for mode in ("wave", "device", "host")}


@pytest.mark.parametrize("curve", CURVES2)
def test_wave_pairing_valid_batches(curve):
    api = _key(curve)["api"]
    seed = bytes(range(7, 39))
    for count in (1, 2, 3, 65):
        got = _three_modes(curve, "merlin", _tiled(curve, "merlin", count), seed=seed)
        v, ok, checks = got["wave"]
        assert v.dtype == np.uint8 and v.tolist() == [api.VERIFY_ACCEPTED] * count and ok is True and checks == 1, (count, v, checks)
        for mode in ("device", "host"):
            assert got[mode][0].tolist() == v.tolist() and got[mode][1:] == (ok, checks), (count, mode)
    _run(curve, "merlin", _tiled(curve, "merlin", 3), pairing="wave")
    tm = api.verify_batch_timings(_key(curve)["pm"]["merlin"].ctx)
    assert tm["pairing_kernels"] > 0 and tm["host_pairing"] > 0, tm                # slots 5 and 4 keep their meaning
    pm = _key(curve)["pm"]["merlin"]
    items = _proofs(curve, "merlin", 3)
    v, ok, checks = pm.verify_batch(_key(curve)["vk"], [x for x, _ in items], [p for _, p in items], pairing="wave")
    assert v.tolist() == [1, 1, 1] and ok and checks == 1
    v, ok, checks = _run(curve, "merlin", [], pairing="wave")
    assert len(v) == 0 and ok is True and checks == 0


def _mixed(curve):
    s = _key(curve)
    r, g1 = s["pm"]["merlin"].field.r, G1N[curve]
    items = list(_tiled(curve, "merlin", 9))
    items[1] = _plus_one(curve, items[1], r)                                        # a tampered a_at_x1
    items[3] = _moved_point(curve, items[3])                                        # a tampered point: no longer in the group
    x, p = items[5]
    items[5] = (x, p[:2 * g1] + r.to_bytes(32, "little") + p[2 * g1 + 32:])         # malformed: a_at_x1 = r is not canonical
    inf = bytes([0xC0]) + bytes(47) if curve == "bls12_381" else bytes(31) + b"\x40"
    x, p = items[6]
    items[6] = (x, p[:2 * g1 + 32] + inf)                                           # [d]_1 = O, canonical: the leaf's -V and W are O
    assert len(items[6][1]) == len(p)
    return items


@pytest.mark.parametrize("curve", CURVES2)
def test_wave_pairing_mixed_batch(curve):
    api = _key(curve)["api"]
    items = _mixed(curve)
    want = [_host_verdict(curve, "merlin", it) for it in items]
    assert want == [1, 0, 1, 2, 1, 2, 0, 1, 1], want
    live = len(items) - want.count(api.VERIFY_MALFORMED)
    for seed in (bytes(range(32)), bytes(range(100, 132))):
        vd, okd, nd = _run(curve, "merlin", items, pairing="device", seed=seed)
        vw, okw, nw = _run(curve, "merlin", items, pairing="wave", seed=seed)
        print(curve, "mixed batch: wave", vw.tolist(), nw, "device", vd.tolist(), nd, "live", live)
        assert vd.tolist() == want and okd is False and nd == 1 + live             # the reference itself
        assert vw.tolist() == vd.tolist() and okw is okd and nw == nd == 1 + live
    v, ok, n = _run(curve, "merlin", items, pairing="wave", seed=bytes(range(32)), verdicts=False)
    assert v is None and ok is False and n <= 1
    only_malformed = [items[k] for k in (0, 3, 4, 5)]                               # the root passes: nothing else is checked
    v, ok, n = _run(curve, "merlin", only_malformed, pairing="wave")
    assert v.tolist() == [1, 2, 1, 2] and ok is False and n == 1


@pytest.mark.parametrize("curve", CURVES2)
def test_wave_pairing_leaf_launch_group_edges(curve):
    """after a failing root every live leaf gets a check: one leaf, as many as fill the launch's last wave exactly, one more, and a
    few waves with a ragged end; one valid proof repeated and one rejected, at the end and in the middle"""
    r = _key(curve)["pm"]["merlin"].field.r
    good = _proofs(curve, "merlin", 2)
    bad = _plus_one(curve, good[1], r)
    for live in sorted({1, PER_WAVE, PER_WAVE + 1, 3 * PER_WAVE + 2}):
        for at in sorted({live - 1, live // 2}):
            items = [good[0]] * live
            items[at] = bad
            want = [1] * live
            want[at] = 0
            v, ok, n = _run(curve, "merlin", items, pairing="wave")
            assert v.tolist() == want and ok is False and n == 1 + live, (live, at, v.tolist(), n)


def test_wave_pairing_both_sides_of_the_leaf_threshold():
    """live = VERIFY_WAVE_LEAF_MAX takes the wave kernel for the leaves, one more takes the lane kernel: the same verdicts"""
    curve = "bn254"
    api, r = _key(curve)["api"], _key(curve)["pm"]["merlin"].field.r
    good = _proofs(curve, "merlin", 2)
    bad = _plus_one(curve, good[1], r)
    for live in (api.VERIFY_WAVE_LEAF_MAX, api.VERIFY_WAVE_LEAF_MAX + 1):
        items = [good[0]] * live
        items[live - 1] = bad
        items[live // 3] = bad
        want = [1] * live
        want[live - 1] = want[live // 3] = 0
        v, ok, n = _run(curve, "merlin", items, pairing="wave")
        assert v.tolist() == want and ok is False and n == 1 + live, (live, n, [i for i, x in enumerate(v.tolist()) if x != want[i]])
        tm = api.verify_batch_timings(_key(curve)["pm"]["merlin"].ctx)
        print("leaf launch, live = %d: pairing launches %.3f ms GPU, pairing stage %.3f ms wall" % (live, tm["pairing_kernels"], tm["host_pairing"]))


@pytest.mark.parametrize("curve", CURVES2)
def test_wave_pairing_with_device_challenges_and_transcripts(curve):
    r = _key(curve)["pm"]["merlin"].field.r
    items = list(_tiled(curve, "merlin", 5))
    w, d = (_run(curve, "merlin", items, pairing=mode, challenges="device") for mode in ("wave", "device"))
    assert w[0].tolist() == d[0].tolist() == [1] * 5 and w[1:] == d[1:] == (True, 1)
    items[2] = _plus_one(curve, items[2], r)
    v, ok, n = _run(curve, "merlin", items, pairing="wave", challenges="device")
    assert v.tolist() == [1, 1, 0, 1, 1] and ok is False and n == 6
    if curve == "bn254":
        for transcript in ("merlin", "keccak256", "blake3"):
            v, ok, n = _run(curve, transcript, _proofs(curve, transcript, 2), pairing="wave")
            assert v.tolist() == [1, 1] and ok is True and n == 1, transcript
        assert not _run(curve, "merlin", _proofs(curve, "blake3", 2), pairing="wave")[1]   # another transcript: other challenges


def _pairing_arg(curve, items, pairing):
    """pm_verify_batch2 itself with `pairing` as given -> (status, verdict bytes, all_accepted, n_checks), the outputs preset to 0x55 / 77 / 99"""
    s = _key(curve)
    api, pm = s["api"], s["pm"]["merlin"]
    pub = np.stack([pm.field.fr_limbs(list(x)) for x, _ in items])
    packed = b"".join(p for _, p in items)
    verdicts = np.full(len(items), 0x55, dtype=np.uint8)
    acc, n = api.ct.c_int(77), api.ct.c_size_t(99)
    st = pm.ctx.L.pm_verify_batch2(pm.ctx.h, api.CURVE_IDS[curve], 0, s["vk"], len(s["vk"]), api._p(pub), pub.shape[1], packed, len(items[0][1]),
                                   len(items), None, pairing, verdicts.ctypes.data_as(api.ct.c_void_p), api.ct.byref(acc), api.ct.byref(n))
    return st, verdicts.tolist(), acc.value, n.value


@pytest.mark.parametrize("curve", CURVES2)
def test_wave_pairing_refusals_and_the_other_modes_afterwards(curve):
    items = list(_proofs(curve, "merlin", 2))
    for pairing in (2, 3, 5, 6, 4 | 2, 4 | 8, 4 | 128, 4 | 512, 7, 128, 512, 256 | 2, 256 | 5):
        assert _pairing_arg(curve, items, pairing) == (1, [0x55, 0x55], 77, 99), pairing   # PM_ERR_INVALID_ARG, nothing written
    for pairing in (4, 4 | 256):
        assert _pairing_arg(curve, items, pairing) == (0, [1, 1], 1, 1), pairing
    r = _key(curve)["pm"]["merlin"].field.r
    items.append(_plus_one(curve, items[0], r))
    for mode in ("wave", "host", "device", "wave"):
        v, ok, n = _run(curve, "merlin", items, pairing=mode)
        assert v.tolist() == [1, 1, 0] and ok is False and (n == 4 or mode == "host"), (mode, v.tolist(), n)
        assert _run(curve, "merlin", items[:2], pairing=mode)[1:] == (True, 1), mode
