"""GPU: the verifier's Fiat-Shamir challenges on the device -- pm_verify_batch2 with PM_VERIFY_CHALLENGES_DEVICE OR-ed into `pairing`
(api.verify_batch(..., challenges="device")): one lane per proof runs the transcript, x1, pi(x1), c(x1), x2 and the weighted scalars;
pm_prove_tap(8) hands back what the lanes derived (api.verifier_challenges_batch).

The challenges, row by row: the expected values are Python integers from oracle/pyref (make_transcripts, compute_x2, compute_pi_at_x1,
compute_c_at_x1, and compute_x1's two appends with the point records given as bytes: the lanes hash them as given, so they are random
bytes and every such proof is "malformed" to the verifier), independent of the host mirror and of the device code.  Per curve and
transcript one pool of rows per n_inputs in {0, 1, 3, 28, 60} (28 and 60 push BLAKE3 past one and two chunks and the batched inversion
past one chunk), computed once; the pools' prefixes of 1, 2, 63, 64, 65 rows and, for n_inputs = 3, 257 rows (one above the kernel's
workgroup of 256) are compared row by row as integers.  Three rows of a 65-row batch get a_at_x1 = r, r + 1, 2^256 - 1: ok = 0 and
zero outputs there, the oracle's values on both sides.  The Merlin rows are checked to include draws with 0, 1 and >= 2 rejections
on each curve (counted on the oracle's side).

The verifier: the proofs and the mixed 21-proof batch of test_gpu_pairing_batch.py (tests/verify_helpers.py), pm_host_verify the
reference for every verdict, all three transcripts and both curves, batches of 1, 2, 37 and 64; for one seed the verdicts,
all_accepted and n_checks equal the host-challenge mode's under both pairing modes; the argument's other bits refused; timing slot 6;
flat memory over 50 calls."""
import os
import random
import struct

import numpy as np
import pytest

import verify_helpers as VH
from verify_helpers import CURVES2, G1N, _bound, _ctx, _host_verdict, _key, _moved_point, _plus_one, _proofs

pytestmark = pytest.mark.gpu

TRANSCRIPTS3 = ("merlin", "keccak256", "blake3")
POOLS = {0: 65, 1: 65, 3: 257, 28: 65, 60: 65}          # n_inputs -> rows
_ORACLE = {}


# -------------------------------------------------------------------------------------------- api.verifier_challenges_batch
def _vk_scalars(vk):
    n, _m0, sigma = struct.unpack("<QQQ", vk[-56:-32])
    return n, sigma, int.from_bytes(vk[-32:], "little")


def _oracle_row(c, T, n, sigma, omega, inputs, a_rec, c_rec, a_at_x1):
    """verify_proof's lines :24-42 (oracle/pyref/protocol.py) -> (x1, x2, c_at_x1, number of rejected Merlin draws)"""
    from oracle.pyref import protocol as PR
    from oracle.pyref.serialize import ser_fr_slice
    r = c.r
    t = T(PR.B_POLYMATH)
    draws = [0]
    if hasattr(t, "m"):                                              # Merlin: count the 64-byte draws
        raw = t.m.challenge_bytes

        def counted(label, k):
            draws[0] += 1
            return raw(label, k)
        t.m.challenge_bytes = counted
    pub = [1] + list(inputs)
    t.append_message(b"public_inputs", ser_fr_slice(c, pub))         # compute_x1 with the two records as they arrived
    t.append_message(b"commitments", struct.pack("<Q", 2) + a_rec + c_rec)
    x1 = t.challenge(b"x1")
    y1_inv = pow(pow(x1, sigma, r), -1, r)
    y1_gamma, y1_alpha = pow(y1_inv, PR.MINUS_GAMMA, r), pow(y1_inv, PR.MINUS_ALPHA, r)
    pi_at_x1 = PR.compute_pi_at_x1(c, n, omega, pub, x1, y1_gamma)
    c_at_x1 = PR.compute_c_at_x1(c, y1_gamma, y1_alpha, a_at_x1, pi_at_x1)
    x2 = PR.compute_x2(c, t, x1, [a_at_x1, c_at_x1])
    return x1, x2, c_at_x1, max(0, draws[0] - 2)


def _pool(curve, transcript, n_inputs):
    """rows of one (curve, transcript, n_inputs): inputs, packed proofs with random point records, the oracle's values"""
    key = (curve, transcript, n_inputs)
    if key not in _ORACLE:
        from oracle.pyref import fields as F, transcripts as TR
        c = F.CURVES[curve]
        T = TR.make_transcripts(c)[transcript]
        n, sigma, omega = _vk_scalars(_key(curve)["vk"])
        rnd = random.Random("challenges %s %s %d" % key)
        g1 = G1N[curve]
        rows = []
        for i in range(POOLS[n_inputs]):
            inputs = [rnd.randrange(c.r) for _ in range(n_inputs)]
            if i == 5 and n_inputs:
                inputs[0], inputs[-1] = 0, c.r - 1
            a_rec, c_rec, d_rec = (bytes(rnd.getrandbits(8) for _ in range(g1)) for _ in range(3))
            a_at = rnd.randrange(c.r)
            proof = a_rec + c_rec + a_at.to_bytes(32, "little") + d_rec
            rows.append((inputs, proof, _oracle_row(c, T, n, sigma, omega, inputs, a_rec, c_rec, a_at)))
        _ORACLE[key] = rows
    return _ORACLE[key]


def _from_mont(field, row):
    v = sum(int(w) << (64 * k) for k, w in enumerate(row))
    return v * field.Rr_inv % field.r


def _challenges(curve, transcript, rows):
    s = _key(curve)
    pm = s["pm"]["merlin"]
    n_inputs = len(rows[0][0])
    pub = np.stack([pm.field.fr_limbs(list(x)) for x, _, _ in rows]) if n_inputs else np.zeros((len(rows), 0, 4), dtype=np.uint64)
    x1, x2, c_at, ok = s["api"].verifier_challenges_batch(pm.ctx, curve, transcript, s["vk"], pub, [p for _, p, _ in rows])
    f = pm.field
    return [(_from_mont(f, x1[i]), _from_mont(f, x2[i]), _from_mont(f, c_at[i])) for i in range(len(rows))], ok, (x1, x2, c_at)


@pytest.mark.parametrize("transcript", TRANSCRIPTS3)
@pytest.mark.parametrize("curve", CURVES2)
def test_challenges_batch_sweep(curve, transcript):
    for n_inputs, size in POOLS.items():
        pool = _pool(curve, transcript, n_inputs)
        for count in (1, 2, 63, 64, 65, 257):
            if count > size:
                continue
            got, ok, _ = _challenges(curve, transcript, pool[:count])
            assert ok.dtype == np.uint8 and ok.tolist() == [1] * count, (n_inputs, count)
            for i in range(count):
                assert got[i] == pool[i][2][:3], (curve, transcript, n_inputs, count, i)
    api = _key(curve)["api"]
    assert api.verify_batch_timings(_ctx(curve))["challenge_kernel"] > 0
    x1, x2, c_at, ok = api.verifier_challenges_batch(_ctx(curve), curve, transcript, _key(curve)["vk"], np.zeros((0, 0, 4), dtype=np.uint64), [])
    assert x1.shape == (0, 4) and len(ok) == 0                                      # count == 0: PM_OK


@pytest.mark.parametrize("transcript", TRANSCRIPTS3)
@pytest.mark.parametrize("curve", CURVES2)
def test_challenges_batch_bad_a_at_x1(curve, transcript):
    from oracle.pyref import fields as F
    r, g1 = F.CURVES[curve].r, G1N[curve]
    rows = list(_pool(curve, transcript, 1)[:65])
    bad = {20: r, 21: r + 1, 63: (1 << 256) - 1}
    for i, v in bad.items():
        x, p, want = rows[i]
        rows[i] = (x, p[:2 * g1] + v.to_bytes(32, "little") + p[2 * g1 + 32:], want)
    got, ok, raw = _challenges(curve, transcript, rows)
    for i in range(65):
        if i in bad:
            assert ok[i] == 0 and not any(a[i].any() for a in raw), i
        else:
            assert ok[i] == 1 and got[i] == rows[i][2][:3], i                       # 19, 22, 62 and 64 among them


@pytest.mark.parametrize("curve", CURVES2)
def test_merlin_rows_cover_the_rejection_loop(curve):
    """a condition on the fixed-seed inputs: the rows the sweep compares include draws that were rejected never, once and at
    least twice (the masked 32 bytes are >= r with probability ~0.55 on BLS12-381, ~0.24 on BN254; two challenges a row)"""
    seen = set()
    for n_inputs in POOLS:
        seen |= {min(row[2][3], 2) for row in _pool(curve, "merlin", n_inputs)}
    assert seen == {0, 1, 2}, seen


# ------------------------------------------------------------------------------ pm_verify_batch2, PM_VERIFY_CHALLENGES_DEVICE
def _run(curve, transcript, items, pairing="host", challenges="device", **kw):
    return VH._run(curve, transcript, items, pairing=pairing, challenges=challenges, **kw)


@pytest.mark.parametrize("curve", CURVES2)
def test_device_challenges_mixed_batch(curve):
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
    seed = bytes(range(32))
    for pairing in ("host", "device"):
        vd, okd, nd = _run(curve, "merlin", items, pairing=pairing, seed=seed)
        vh, okh, nh = _run(curve, "merlin", items, pairing=pairing, challenges="host", seed=seed)
        print(curve, "mixed batch, pairing", pairing, "device challenges: verdicts", vd.tolist(), "n_checks", nd, "host challenges:", nh)
        assert vd.tolist() == want and okd is False
        assert vh.tolist() == vd.tolist() and okh == okd and nh == nd
        assert nd == 1 + live if pairing == "device" else 1 < nd <= _bound(21, f)
    v3, ok3, n3 = _run(curve, "merlin", items, seed=seed, verdicts=False)
    assert v3 is None and ok3 is False and n3 <= 1
    only_malformed = [items[k] for k in (0, 2, 6, 12)]               # the root passes, nothing else is checked
    v5, ok5, n5 = _run(curve, "merlin", only_malformed)
    assert v5.tolist() == [1, 2, 1, 2] and ok5 is False and n5 == 1


def _pairing_arg(curve, items, pairing):
    s = _key(curve)
    api, pm = s["api"], s["pm"]["merlin"]
    pub = np.stack([pm.field.fr_limbs(list(x)) for x, _ in items])
    packed = b"".join(p for _, p in items)
    acc, n = api.ct.c_int(0), api.ct.c_size_t(0)
    st = pm.ctx.L.pm_verify_batch2(pm.ctx.h, api.CURVE_IDS[curve], 0, s["vk"], len(s["vk"]), api._p(pub), pub.shape[1], packed, len(items[0][1]),
                                   len(items), None, pairing, None, api.ct.byref(acc), api.ct.byref(n))
    return st, acc.value


@pytest.mark.parametrize("curve", CURVES2)
def test_device_challenges_valid_batches_and_arguments(curve):
    api = _key(curve)["api"]
    for transcript in TRANSCRIPTS3:
        for count in (1, 2, 37, 64):
            v, ok, checks = _run(curve, transcript, _proofs(curve, transcript, count))
            assert v.dtype == np.uint8 and v.tolist() == [api.VERIFY_ACCEPTED] * count and ok is True and checks == 1, (transcript, count, v, checks)
    for transcript in ("keccak256", "blake3"):
        assert not _run(curve, "merlin", _proofs(curve, transcript, 2))[1]          # another transcript: other challenges
        assert not _run(curve, transcript, _proofs(curve, "merlin", 2))[1]
    v, ok, checks = _run(curve, "merlin", _proofs(curve, "merlin", 3), pairing="device")
    assert v.tolist() == [1, 1, 1] and ok and checks == 1
    v, ok, checks = _run(curve, "merlin", [])
    assert len(v) == 0 and ok is True and checks == 0
    v, ok, checks = _run(curve, "merlin", _proofs(curve, "merlin", 5), verdicts=False)
    assert v is None and ok is True and checks == 1
    pm = _key(curve)["pm"]["merlin"]
    items = _proofs(curve, "merlin", 3)
    v, ok, checks = pm.verify_batch(_key(curve)["vk"], [x for x, _ in items], [p for _, p in items], challenges="device")
    assert v.tolist() == [1, 1, 1] and ok and checks == 1
    for pairing in (256, 257):                                                      # the flag alone and with PM_VERIFY_PAIRING_DEVICE
        assert _pairing_arg(curve, items[:2], pairing) == (0, 1), pairing
    for pairing in (2, 256 | 2, 512, 257 | 512, 128, -1):                           # any other bit or value: PM_ERR_INVALID_ARG
        assert _pairing_arg(curve, items[:1], pairing)[0] == 1, pairing
    v, ok, checks = _run(curve, "merlin", items, challenges="host")                 # pm_verify_batch2's path afterwards: unaffected
    assert v.tolist() == [1, 1, 1] and ok and checks == 1


def test_device_challenges_timing_slots():
    curve = "bn254"
    api = _key(curve)["api"]
    items = _proofs(curve, "merlin", 8)
    assert _run(curve, "merlin", items)[1]
    tm = api.verify_batch_timings(_ctx(curve))
    assert tm["challenge_kernel"] > 0 and tm["host_glue"] > 0, tm                   # slot 6: the launch's GPU ms
    assert _run(curve, "merlin", items, challenges="host")[1]
    tm = api.verify_batch_timings(_ctx(curve))
    assert tm["challenge_kernel"] == 0 and tm["host_glue"] > 0, tm


def test_device_challenges_flat_memory():
    """50 device-challenge calls: free device memory as the runtime reports it (hipMemGetInfo, the check of
    test_gpu_pairing_batch.py) is where it was within 8 MiB, the process's resident set within 32 MiB -- what this catches is a
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
        _run(curve, "merlin", items, pairing="device")
    free0, rss0 = free_hbm(), rss()
    for _ in range(50):
        v, ok, n = _run(curve, "merlin", items, pairing="device")
        assert v.tolist() == want and not ok and n == 9
    free1, rss1 = free_hbm(), rss()
    print("free device memory before / after 50 device-challenge calls:", free0, free1, "resident set:", rss0, rss1)
    assert abs(free0 - free1) <= 8 << 20, (free0, free1)
    assert rss1 - rss0 <= 32 << 20, (rss0, rss1)
