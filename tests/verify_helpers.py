"""Shared by the GPU tests of the batch verifier (test_gpu_verify_batch.py, test_gpu_pairing_batch.py, test_gpu_challenges.py,
test_gpu_verify_modes.py): ONE context, MiMC key (circuits.MiMCDemo, 16 rounds) and vk per curve and one growing list of proofs per
transcript for the whole session, and the helpers that run a batch and ask the host verifier (pm_host_verify) for a proof's verdict."""
import math

import numpy as np

CURVES2 = ("bls12_381", "bn254")
G1N = {"bls12_381": 48, "bn254": 32}
_STATE = {}


def _bound(count, f):
    """host pairing: with f REJECTED proofs, n_checks <= 1 + 2 f ceil(log2 count)"""
    return 1 + 2 * f * (math.ceil(math.log2(count)) if count > 1 else 0)


def _key(curve):
    """one context, key and vk per curve, and a growing list of (public inputs as ints, proof bytes) per transcript"""
    if curve not in _STATE:
        from polymath_amd import api, circuits as PC, rng as R
        from polymath_amd.polymath import Polymath
        rng = R.StdRng.seed_from_u64(0xB47C + len(curve))
        pm = Polymath(curve, "merlin", device=0)
        r = pm.field.r
        consts = [R.fr_rand(rng, r) for _ in range(16)]
        circuit = PC.MiMCDemo(R.fr_rand(rng, r), R.fr_rand(rng, r), consts)
        pk = pm.setup(circuit, rng)
        _STATE[curve] = dict(api=api, pm={"merlin": pm}, pk=pk, vk=pm.make_vk(pk, *pm.last_trapdoors), rng=rng, consts=consts, proofs={})
    return _STATE[curve]


def _ctx(curve):
    return _key(curve)["pm"]["merlin"].ctx


def _proofs(curve, transcript, count):
    from polymath_amd import circuits as PC, rng as R
    from polymath_amd.polymath import Polymath
    s = _key(curve)
    if transcript not in s["pm"]:
        s["pm"][transcript] = Polymath(curve, transcript, ctx=s["pm"]["merlin"].ctx)
    pm, have = s["pm"][transcript], s["proofs"].setdefault(transcript, [])
    while len(have) < count:
        circuit = PC.MiMCDemo(R.fr_rand(s["rng"], pm.field.r), R.fr_rand(s["rng"], pm.field.r), s["consts"])
        proof = pm.prove(s["pk"], circuit, s["rng"])
        have.append((pm._synthesize(circuit)[1][1:], proof.to_bytes()))
    return have[:count]


def _run(curve, transcript, items, pairing="host", challenges="host", **kw):
    s = _key(curve)
    pm = s["pm"]["merlin"]
    pub = np.stack([pm.field.fr_limbs(list(x)) for x, _ in items]) if items else np.zeros((0, 0, 4), dtype=np.uint64)
    return s["api"].verify_batch(pm.ctx, curve, transcript, s["vk"], pub, [p for _, p in items], pairing=pairing, challenges=challenges, **kw)


def _host_verdict(curve, transcript, item):
    s = _key(curve)
    api = s["api"]
    try:
        return api.VERIFY_ACCEPTED if api.verify(curve, transcript, s["vk"], s["pm"]["merlin"].field.fr_limbs(list(item[0])), item[1]) else api.VERIFY_REJECTED
    except api.PolymathError:
        return api.VERIFY_MALFORMED


def _moved_point(curve, item):
    """a_g1's x walked until the encoding no longer decodes into the group (off the curve, or on it and outside G1)"""
    for tweak in range(1, 40):
        bad = bytearray(item[1])
        k = G1N[curve] - 1 if curve == "bls12_381" else 0           # the low byte of x
        bad[k] = (bad[k] + tweak) & 0xFF
        cand = (item[0], bytes(bad))
        if _host_verdict(curve, "merlin", cand) == 2:
            return cand
    raise AssertionError("no tweak of x left the group")


def _plus_one(curve, item, r):
    """a_at_x1 + 1"""
    g1 = G1N[curve]
    x, p = item
    a_at = int.from_bytes(p[2 * g1:2 * g1 + 32], "little")
    return (x, p[:2 * g1] + ((a_at + 1) % r).to_bytes(32, "little") + p[2 * g1 + 32:])
