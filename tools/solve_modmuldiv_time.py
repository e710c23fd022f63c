"""Times the solving call on one level of declared modular multiply-divides beside one level of declared modular divisions
(profiles/witness_solve.txt, section 9), in ONE process, alternating: LimbModMulDiv (all six lists, cN = 3, cD = 2) and LimbModDiv,
COUNT hints each modulo secp256k1's prime on 4 limbs of 64 bits without the decompositions -- one level of COUNT hints of the kind,
then block launches, ordinary rows, one level of COUNT long divisions and chain launches -- BATCH assignments a call, through
Polymath.check_batch's native call (pm_r1cs_check_batch, max_rows = 0) with PM_ASSIGNMENT_SOLVE on host limbs: per circuit one call
that plans, then REPS timed ones.  The completed assignment of one row is compared with native().

    python tools/solve_modmuldiv_time.py [--curve bls12_381] [--count 256] [--batch 256] [--reps 7]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/solve_modmuldiv_time.py
                                                  (k_solve_modmuldiv and k_solve_moddiv alone, side by side: a run of its own)
"""
import argparse
import os
import sys
import time

import numpy as np
import torch        # noqa: F401  before the library: torch brings its own HIP runtime

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from polymath_amd import circuits as PC  # noqa: E402
from polymath_amd.polymath import Polymath  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--curve", default="bls12_381")
ap.add_argument("--count", type=int, default=256)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--reps", type=int, default=7)
a = ap.parse_args()
SECP = 2 ** 256 - 2 ** 32 - 977
pm = Polymath(a.curve, "merlin", device=0)
r = pm.field.r
makers = {"modmuldiv": lambda seed: PC.LimbModMulDiv(PC.modmuldiv_cases(SECP, a.count, seed, cD=2), SECP, 64, 4, 3, 2, decompose=False),
          "moddiv": lambda seed: PC.LimbModDiv(PC.moddiv_cases(SECP, a.count, seed), SECP, 64, 4, decompose=False)}
runs = {}
for name, make in makers.items():
    distinct = [make(25000 + i) for i in range(min(a.batch, 8))]
    pk = pm.setup(distinct[0], 123, 456)
    pm.set_hints(pk, distinct[0].hints(2))
    partial = distinct[0].partial(r)
    marks = np.array([v is None for v in partial[0] + partial[1]], dtype=bool)
    full = [np.concatenate([pm.field.fr_limbs(inst), pm.field.fr_limbs(wit)]).reshape(-1, 4) for inst, wit in (c.native(r) for c in distinct)]
    want = np.stack([full[i % len(full)] for i in range(a.batch)])
    rows = want.copy()
    rows[:, marks] = 0xFFFFFFFFFFFFFFFF
    runs[name] = dict(pk=pk, xs=np.ascontiguousarray(rows[:, :2]), ws=np.ascontiguousarray(rows[:, 2:]), want=want, wall=[], kernels=[])
for rep in range(a.reps + 1):
    for name, run in runs.items():          # alternating: both circuits see the same box in the same minutes
        t0 = time.perf_counter()
        rc, n_bad, _, _ = run["pk"].r1cs_check_batch(run["xs"], run["ws"], 0, solve=True)
        dt = time.perf_counter() - t0
        assert rc == 0 and not n_bad.any(), pm.ctx.last_error()
        if rep == 0:
            print("%s: first call (plan): %.1f ms" % (name, 1e3 * dt))
            assert np.array_equal(run["pk"].solved_assignments(a.batch, run["ws"].shape[1])[a.batch // 2], run["want"][a.batch // 2])
        else:
            run["wall"].append(1e3 * dt)
            run["kernels"].append(pm.ctx.timings()["ntt"])      # slot 1: the solve kernels of the call
spread = lambda v: "%.3f [%.3f .. %.3f]" % (sorted(v)[len(v) // 2], min(v), max(v))
for name, run in runs.items():
    print("%s %s, %d hints x %d assignments, %d calls: call, wall ms %s; solve kernels, slot 1 ms %s" % (a.curve, name, a.count, a.batch, a.reps, spread(run["wall"]), spread(run["kernels"])))
    run["pk"].free()
