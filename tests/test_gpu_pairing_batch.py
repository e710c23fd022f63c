"""GPU: pairing checks on the device -- pm_pairing_check_batch (api.pairing_check_batch: one lane per check against k fixed G2
points) and pm_verify_batch2 with PM_VERIFY_PAIRING_DEVICE (api.verify_batch(..., pairing="device"): the root in a launch of one
lane, every live leaf in ONE more launch when it fails).

pm_pairing_check_batch: cases with known answers from oracle/pyref G1 / G2 arithmetic, e(aP, Q) e(-P, aQ) = 1 and the same with
a + 1 (!= 1), a pool of them tiled to count = 1, 2, 65, 300 (lane 64 and five waves); k = 1 with P = O; k = 3 with and without an
infinite point; a G2 point off the twist.

pm_verify_batch2, device mode: the proofs of test_gpu_verify_batch.py (tests/verify_helpers.py), the host verifier
api.verify (pm_host_verify) the reference for every verdict, n_checks == 1 for a valid batch and == 1 + live after a failing root;
then the same context in host mode.  One timed comparison in one process (32 BLS12-381 proofs, 3 tampered, spread apart): device
mode must be faster than host mode, no ratio asserted (the ratio is printed under -s; profiles/verify_batch_device_pairing.txt)."""
import os
import random
import time

import numpy as np
import pytest

import verify_helpers as VH
from verify_helpers import CURVES2, G1N, _bound, _ctx, _host_verdict, _key, _moved_point, _plus_one, _proofs

pytestmark = pytest.mark.gpu



# ------------------------------------------------------------------------------------------------ pm_pairing_check_batch
def _limbs(v, n):
    return [(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(n)]


def _g1_row(c, P):
    """x || y Montgomery limbs; None (infinity) is all-zero"""
    n = c.fq_limbs64
    if P is None:
        return [0] * (2 * n)
    return _limbs(c.fq_to_mont(P[0]), n) + _limbs(c.fq_to_mont(P[1]), n)


def _g2_row(c, Q):
    n = c.fq_limbs64
    (x0, x1), (y0, y1) = Q
    return sum((_limbs(c.fq_to_mont(v), n) for v in (x0, x1, y0, y1)), [])


@pytest.mark.parametrize("curve", CURVES2)
def test_pairing_check_batch_two_pairs(curve):
    from oracle.pyref import fields as F, pairing as PR
    from polymath_amd import api
    c, eng = F.CURVES[curve], PR.ENGINES[curve]
    rnd = random.Random(0x9A1 + len(curve))
    a = rnd.randrange(2, c.r)
    Q = eng.g2_mul(eng.g2_gen, rnd.randrange(2, c.r))
    aQ = eng.g2_mul(Q, a)
    assert eng.g2_is_on_curve(Q) and eng.g2_is_on_curve(aQ)
    g2 = np.array([_g2_row(c, Q), _g2_row(c, aQ)], dtype=np.uint64)
    pool = []                                                        # (rows of the two G1 points, expected byte)
    for t in range(16):
        s = rnd.randrange(2, c.r)
        P = F.g1_mul(c, c.g1, s)
        one = t % 2 == 0
        aP = F.g1_mul(c, c.g1, (a if one else a + 1) * s % c.r)     # e(aP, Q) e(-P, aQ) = 1;  with a + 1 it is e(P, Q) != 1
        pool.append(([_g1_row(c, aP), _g1_row(c, F.g1_neg(c, P))], 1 if one else 0))
    pool.append(([_g1_row(c, None), _g1_row(c, None)], 1))           # both points at infinity
    pool.append(([_g1_row(c, None), _g1_row(c, F.g1_neg(c, c.g1))], 0))
    ctx = _ctx(curve)
    for count in (1, 2, 65, 300):
        pick = [rnd.randrange(len(pool)) for _ in range(count)]
        g1 = np.array([pool[i][0] for i in pick], dtype=np.uint64)
        got = api.pairing_check_batch(ctx, curve, g2, g1)
        assert got.dtype == np.uint8 and got.tolist() == [pool[i][1] for i in pick], (curve, count)
    assert ctx.timings()["phase"] > 0                                # slot 7: the launch
    assert len(api.pairing_check_batch(ctx, curve, g2, np.zeros((0, 2, 2 * c.fq_limbs64), dtype=np.uint64))) == 0
    off = g2.copy()
    off[1, 2 * c.fq_limbs64] ^= 1                                    # y.c0 of the second point
    with pytest.raises(api.PolymathError) as e:
        api.pairing_check_batch(ctx, curve, off, np.array([pool[0][0]], dtype=np.uint64))
    assert e.value.status == 1                                       # PM_ERR_INVALID_ARG
    with pytest.raises(api.PolymathError):
        api.pairing_check_batch(ctx, curve, np.concatenate([g2, g2, g2[:1]]), np.zeros((1, 5, 2 * c.fq_limbs64), dtype=np.uint64))   # k = 5


@pytest.mark.parametrize("curve", CURVES2)
def test_pairing_check_batch_one_and_three_pairs(curve):
    from oracle.pyref import fields as F, pairing as PR
    from polymath_amd import api
    c, eng = F.CURVES[curve], PR.ENGINES[curve]
    rnd = random.Random(0x3B7 + len(curve))
    ctx = _ctx(curve)
    q1, q2 = rnd.randrange(2, c.r), rnd.randrange(2, c.r)
    Q1, Q2, H = eng.g2_mul(eng.g2_gen, q1), eng.g2_mul(eng.g2_gen, q2), eng.g2_gen
    # k = 1: only the point at infinity pairs to 1
    got = api.pairing_check_batch(ctx, curve, np.array([_g2_row(c, Q1)], dtype=np.uint64),
                                  np.array([[_g1_row(c, None)], [_g1_row(c, c.g1)], [_g1_row(c, None)]], dtype=np.uint64))
    assert got.tolist() == [1, 0, 1]
    # k = 3: p1 q1 + p2 q2 + p3 = 0
    g2 = np.array([_g2_row(c, Q1), _g2_row(c, Q2), _g2_row(c, H)], dtype=np.uint64)
    rows, want = [], []
    for t in range(6):
        p1, p2 = rnd.randrange(2, c.r), rnd.randrange(2, c.r)
        if t == 4:
            p2 = 0                                                   # the middle point at infinity
        p3 = -(p1 * q1 + p2 * q2) % c.r
        if t % 2:
            p3 = (p3 + 1) % c.r
        rows.append([_g1_row(c, F.g1_mul(c, c.g1, p) if p else None) for p in (p1, p2, p3)])
        want.append(0 if t % 2 else 1)
    rows.append([_g1_row(c, None)] * 3)
    want.append(1)
    got = api.pairing_check_batch(ctx, curve, g2, np.array(rows, dtype=np.uint64))
    assert got.tolist() == want, (curve, got.tolist())


# ------------------------------------------------------------------------------- pm_verify_batch2, PM_VERIFY_PAIRING_DEVICE
def _run(curve, transcript, items, pairing="device", **kw):
    return VH._run(curve, transcript, items, pairing=pairing, **kw)


@pytest.mark.parametrize("curve", CURVES2)
def test_device_pairing_valid_batches(curve):
    api = _key(curve)["api"]
    for count in (1, 2, 37, 64):
        v, ok, checks = _run(curve, "merlin", _proofs(curve, "merlin", count))
        assert v.dtype == np.uint8 and v.tolist() == [api.VERIFY_ACCEPTED] * count and ok is True and checks == 1, (count, v, checks)
    tm = api.verify_batch_timings(_ctx(curve))
    assert tm["pairing_kernels"] > 0 and tm["host_pairing"] > 0, tm                # slot 5: the launch's GPU ms; slot 4: the checks' wall ms
    for transcript in ("keccak256", "blake3"):
        v, ok, checks = _run(curve, transcript, _proofs(curve, transcript, 2))
        assert v.tolist() == [api.VERIFY_ACCEPTED] * 2 and ok and checks == 1, transcript
        assert not _run(curve, "merlin", _proofs(curve, transcript, 2))[1]          # another transcript: other challenges
    v, ok, checks = _run(curve, "merlin", [])
    assert len(v) == 0 and ok is True and checks == 0
    pm = _key(curve)["pm"]["merlin"]
    items = _proofs(curve, "merlin", 3)
    v, ok, checks = pm.verify_batch(_key(curve)["vk"], [x for x, _ in items], [p for _, p in items], pairing="device")
    assert v.tolist() == [1, 1, 1] and ok and checks == 1


@pytest.mark.parametrize("curve", CURVES2)
def test_device_pairing_mixed_batch(curve):
    s = _key(curve)
    api, r, g1 = s["api"], s["pm"]["merlin"].field.r, G1N[curve]
    items = list(_proofs(curve, "merlin", 21))
    items[7] = items[6]                                              # the same valid proof twice
    altered = {}
    altered[2] = _moved_point(curve, items[2])
    x, p = items[12]
    altered[12] = (x, p[:2 * g1] + r.to_bytes(32, "little") + p[2 * g1 + 32:])                      # a_at_x1 = r: not canonical
    altered[18] = _plus_one(curve, items[18], r)
    x, p = items[19]
    altered[19] = ([(x[0] + 1) % r] + list(x[1:]), p)                                                # a wrong public input
    x, p = items[20]
    inf = bytes([0xC0]) + bytes(47) if curve == "bls12_381" else bytes(31) + b"\x40"
    altered[20] = (x, inf + p[g1:])                                                                  # canonical infinity as a_g1
    for k, it in altered.items():
        items[k] = it
    want = [api.VERIFY_ACCEPTED] * 21
    for k in list(altered) + [0, 7, 13]:                             # every altered proof and three unaltered ones, by the host verifier
        want[k] = _host_verdict(curve, "merlin", items[k])
    assert [want[k] for k in (0, 7, 13)] == [1, 1, 1] and want[2] == want[12] == 2 and want[18] == want[19] == want[20] == 0, want
    f, live = want.count(api.VERIFY_REJECTED), 21 - want.count(api.VERIFY_MALFORMED)
    seed_a, seed_b = bytes(range(32)), bytes(range(100, 132))
    v1, ok1, n1 = _run(curve, "merlin", items, seed=seed_a)
    print(curve, "mixed batch, device pairing: verdicts", v1.tolist(), "n_checks", n1, "live", live)
    assert v1.tolist() == want and ok1 is False and n1 == 1 + live
    v2, ok2, n2 = _run(curve, "merlin", items, seed=seed_b)
    assert v2.tolist() == want and ok2 is False and n2 == 1 + live
    v3, ok3, n3 = _run(curve, "merlin", items, seed=seed_a, verdicts=False)
    assert v3 is None and ok3 is False and n3 <= 1
    # host mode afterwards in the same context: the bisection's verdicts and its bound
    v4, ok4, n4 = _run(curve, "merlin", items, pairing="host", seed=seed_a)
    assert v4.tolist() == want and ok4 is False and 1 < n4 <= _bound(21, f)
    # a batch whose only defects are malformed proofs: the root passes, nothing else is checked
    only_malformed = [items[k] for k in (0, 2, 6, 12)]
    v5, ok5, n5 = _run(curve, "merlin", only_malformed)
    assert v5.tolist() == [1, 2, 1, 2] and ok5 is False and n5 == 1
    st = _pairing_arg(curve, only_malformed[:1], 2)
    assert st == 1                                                   # another `pairing` value: PM_ERR_INVALID_ARG


def _pairing_arg(curve, items, pairing):
    s = _key(curve)
    api, pm = s["api"], s["pm"]["merlin"]
    pub = np.stack([pm.field.fr_limbs(list(x)) for x, _ in items])
    packed = b"".join(p for _, p in items)
    acc, n = api.ct.c_int(0), api.ct.c_size_t(0)
    return pm.ctx.L.pm_verify_batch2(pm.ctx.h, api.CURVE_IDS[curve], 0, s["vk"], len(s["vk"]), api._p(pub), pub.shape[1], packed, len(items[0][1]),
                                     len(items), None, pairing, None, api.ct.byref(acc), api.ct.byref(n))


def test_device_pairing_is_faster_on_a_failing_batch():
    """32 BLS12-381 proofs, 3 tampered and spread apart: host mode bisects (at most 31 checks of ~118 ms), device mode makes two
    launches.  Same process, same box, one call each after a warm-up of the device mode's code object; "faster" is all that is
    asserted, the ratio is printed."""
    curve = "bls12_381"
    s = _key(curve)
    api, r = s["api"], s["pm"]["merlin"].field.r
    items = list(_proofs(curve, "merlin", 32))
    for k in (3, 16, 29):
        items[k] = _plus_one(curve, items[k], r)
    want = [0 if k in (3, 16, 29) else 1 for k in range(32)]
    _run(curve, "merlin", items[:2])
    t0 = time.perf_counter()
    vh, okh, nh = _run(curve, "merlin", items, pairing="host")
    host_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    vd, okd, nd = _run(curve, "merlin", items, pairing="device")
    dev_s = time.perf_counter() - t0
    tm = api.verify_batch_timings(_ctx(curve))
    print("32 proofs, 3 rejected: host mode %.3f s (%d checks), device mode %.3f s (%d checks), host / device = %.1f; device mode slots %s"
          % (host_s, nh, dev_s, nd, host_s / dev_s, {k: round(x, 3) for k, x in tm.items()}))
    assert vh.tolist() == want and vd.tolist() == want and not okh and not okd
    assert nh <= _bound(32, 3) and nd == 33
    assert dev_s < host_s


def test_device_pairing_hygiene_and_flat_memory():
    """50 device-mode calls that take both launches: free device memory as the runtime reports it (hipMemGetInfo, the check of
    test_gpu_verify_batch.py) is where it was within 8 MiB, and so is the process's resident set within 32 MiB -- a call's host
    working set (line tables, 8 leaves) is a few hundred KiB, so a leak of it per call would still pass; what this catches is a
    leaked device buffer or staging area."""
    import ctypes as ct
    curve = "bn254"
    s = _key(curve)
    pm = s["pm"]["merlin"]
    items = list(_proofs(curve, "merlin", 8))
    items[5] = ([(items[5][0][0] + 1) % pm.field.r], items[5][1])
    want = [1, 1, 1, 1, 1, 0, 1, 1]
    hip = ct.CDLL("libamdhip64.so")

    def free_hbm():
        fr, tot = ct.c_size_t(), ct.c_size_t()
        assert hip.hipMemGetInfo(ct.byref(fr), ct.byref(tot)) == 0
        return fr.value

    def rss():
        with open("/proc/self/statm") as fh:
            return int(fh.read().split()[1]) * os.sysconf("SC_PAGE_SIZE")

    for _ in range(3):
        _run(curve, "merlin", items)
    free0, rss0 = free_hbm(), rss()
    for _ in range(50):
        v, ok, n = _run(curve, "merlin", items)
        assert v.tolist() == want and not ok and n == 9
    free1, rss1 = free_hbm(), rss()
    print("free device memory before / after 50 device-mode calls:", free0, free1, "resident set:", rss0, rss1)
    assert abs(free0 - free1) <= 8 << 20, (free0, free1)
    assert rss1 - rss0 <= 32 << 20, (rss0, rss1)
