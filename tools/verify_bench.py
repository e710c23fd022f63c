"""Batch verification against single verification (DESIGN.md "Batch verification"; profiles/verify_batch.txt).

    python tools/verify_bench.py --count 1024 [--bad 8] [--curve bls12_381] [--distinct 64] [--pairing host|device|wave]
                                 [--challenges host|device] [--alternate ROUNDS] [--alternate-pairing ROUNDS]

Makes proofs of circuits.MiMCDemo (16 rounds) on one key -- `--distinct` of them with their own witness and r_a, tiled up to
`--count` -- and times (a) verify_batch, (b) the same with verdicts=False, (c) pm_host_verify on 4 of the proofs (mean) and,
with --bad F, (d) the batch with F proofs tampered (a_at_x1 + 1, spread evenly): the bisection (--pairing host) or the one launch
over all leaves (--pairing device; --pairing wave: the same launches, a check spread over 36 lanes of a wave).  --challenges picks where the per-proof Fiat-Shamir challenges run (PM_VERIFY_CHALLENGES_DEVICE); with
--alternate N the valid batch is also verified N more times in each mode, host and device taking turns in this one process, and
"alternate" lists per call the wall time, slot 3 (host glue, wall ms) and slot 6 (challenge kernel, GPU ms).  With --alternate-pairing N
the valid batch is verified N more times in each PAIRING mode, host, device and wave taking turns in this one process after one warm-up
call each (with --bad the tampered batch too, in the two device modes: the host's bisection is not what that batch is there to show), and "alternate_pairing" lists per call slot 4 (pairing stage, wall ms) and slot 5 (pairing
launches, GPU ms), with their medians and ranges per mode.  Prints ONE JSON line; the kernel times are pm_last_timings' (HIP events inside the call)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, required=True)
    ap.add_argument("--bad", type=int, default=0)
    ap.add_argument("--curve", default="bls12_381")
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--pairing", choices=("host", "device", "wave"), default="host")
    ap.add_argument("--challenges", choices=("host", "device"), default="host")
    ap.add_argument("--alternate", type=int, default=0)
    ap.add_argument("--alternate-pairing", type=int, default=0)
    a = ap.parse_args()
    from polymath_amd import api, circuits as PC, rng as R
    from polymath_amd.polymath import Polymath
    pm = Polymath(a.curve, "merlin", device=0)
    f, r = pm.field, pm.field.r
    rng = R.StdRng.seed_from_u64(7)
    consts = [R.fr_rand(rng, r) for _ in range(16)]
    shape = PC.MiMCDemo(R.fr_rand(rng, r), R.fr_rand(rng, r), consts)
    pk = pm.setup(shape, rng)
    vk = pm.make_vk(pk, *pm.last_trapdoors)
    made = []
    for _ in range(min(a.distinct, a.count)):
        circuit = PC.MiMCDemo(R.fr_rand(rng, r), R.fr_rand(rng, r), consts)
        made.append((f.fr_limbs(pm._synthesize(circuit)[1][1:]), pm.prove(pk, circuit, rng).to_bytes()))
    items = [made[i % len(made)] for i in range(a.count)]
    pub = np.stack([x for x, _ in items])
    proofs = [p for _, p in items]

    def timed(proofs, challenges=a.challenges, pairing=a.pairing, **kw):
        t0 = time.perf_counter()
        v, ok, checks = api.verify_batch(pm.ctx, a.curve, "merlin", vk, pub, b"".join(proofs), pairing=pairing, challenges=challenges, **kw)
        wall = (time.perf_counter() - t0) * 1e3
        return dict(wall_ms=round(wall, 3), all_accepted=ok, n_checks=checks, rejected=int((v == 0).sum()) if v is not None else None,
                    **{k + "_ms": round(x, 3) for k, x in api.verify_batch_timings(pm.ctx).items()})

    timed(proofs[:2])                                  # first launch: code objects
    if a.alternate and a.challenges != "device":
        timed(proofs[:2], challenges="device")       # the other mode's code object, only when that mode is timed
    out = dict(curve=a.curve, pairing=a.pairing, challenges=a.challenges, count=a.count, distinct=len(made), gates=pk.n)
    out["batch"] = timed(proofs)
    out["batch_no_verdicts"] = timed(proofs, verdicts=False)
    t0 = time.perf_counter()
    for x, p in items[:4]:
        assert api.verify(a.curve, "merlin", vk, x, p)
    out["host_verify_ms"] = round((time.perf_counter() - t0) * 1e3 / min(4, len(items)), 3)
    out["proofs_per_s"] = round(a.count / out["batch"]["wall_ms"] * 1e3, 1)
    out["ratio_to_count_singles"] = round(out["batch"]["wall_ms"] / (a.count * out["host_verify_ms"]), 6)
    if a.bad:
        g1 = api.G1_BYTES[api.CURVE_IDS[a.curve]]
        tampered = list(proofs)
        for k in range(a.bad):
            i = (2 * k + 1) * a.count // (2 * a.bad)
            p = tampered[i]
            v = (int.from_bytes(p[2 * g1:2 * g1 + 32], "little") + 1) % r
            tampered[i] = p[:2 * g1] + v.to_bytes(32, "little") + p[2 * g1 + 32:]
        out["descent"] = dict(bad=a.bad, **timed(tampered))
    if a.alternate_pairing:
        modes = ("host", "device", "wave")
        batches = [("valid", proofs)] + ([("bad", tampered)] if a.bad else [])
        for mode in modes:
            timed(proofs[:2], pairing=mode)          # every mode's code object
        calls, want = [], {}
        for _ in range(a.alternate_pairing):
            for what, batch in batches:
                for mode in modes if what == "valid" else modes[1:]:
                    t = timed(batch, pairing=mode)
                    assert want.setdefault(what, t["rejected"]) == t["rejected"] and t["all_accepted"] == (what == "valid")
                    calls.append(dict(batch=what, pairing=mode, n_checks=t["n_checks"], slot4_pairing_wall_ms=t["host_pairing_ms"],
                                      slot5_pairing_kernels_ms=t["pairing_kernels_ms"], wall_ms=t["wall_ms"]))
        summary = {}
        for what, _ in batches:
            for mode in modes if what == "valid" else modes[1:]:
                for slot in ("slot4_pairing_wall_ms", "slot5_pairing_kernels_ms"):
                    xs = sorted(c[slot] for c in calls if c["batch"] == what and c["pairing"] == mode)
                    summary["%s/%s/%s" % (what, mode, slot)] = dict(median=xs[len(xs) // 2], min=xs[0], max=xs[-1])
        out["alternate_pairing"] = dict(calls=calls, summary=summary)
    if a.alternate:
        out["alternate"] = []
        for _ in range(a.alternate):
            for mode in ("host", "device"):
                t = timed(proofs, challenges=mode)
                assert t["all_accepted"] and t["n_checks"] == 1
                out["alternate"].append(dict(challenges=mode, wall_ms=t["wall_ms"], slot3_host_glue_ms=t["host_glue_ms"],
                                             slot6_challenge_kernel_ms=t["challenge_kernel_ms"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
