"""Times the solving call on one level of declared long divisions (profiles/witness_solve.txt, section 8): LimbDivision, COUNT
divisions of KD by KE limbs of N bits, random operands, the divisor in columns -- one level of COUNT hints, then the sums' chain --
BATCH assignments a call, through Polymath.check_batch's native call (pm_r1cs_check_batch, max_rows = 0) with PM_ASSIGNMENT_SOLVE on
host limbs: one call that plans, then REPS timed ones in one process.  --narrow declares opcode 1 (k_solve_longdiv, a lane per
division) in place of opcode 5 (k_solve_longdiv_wide, a wave per division), for the shapes both accept.  The completed assignment of
one row is compared with native().

    python tools/solve_widediv_time.py [--curve bls12_381] [--count 256] [--batch 256] [--shape 64:63:32] [--narrow] [--reps 7]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/solve_widediv_time.py     (the kernel alone: a run of its own)
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
ap.add_argument("--shape", default="64:63:32", help="N:KD:KE")
ap.add_argument("--narrow", action="store_true")
ap.add_argument("--reps", type=int, default=7)
a = ap.parse_args()
n, kD, kE = (int(v) for v in a.shape.split(":"))
pm = Polymath(a.curve, "merlin", device=0)
r = pm.field.r


def make(seed):
    g = PC.SplitMix64(seed)
    draw = lambda bits: sum(g.next_u64() << (64 * i) for i in range(-(-bits // 64))) & ((1 << bits) - 1)
    return PC.LimbDivision([(PC.int_limbs(draw(n * kD), n, kD), PC.int_limbs(draw(n * kE) | 1 << (n * kE - 1), n, kE)) for _ in range(a.count)], n, kD, kE, wide=not a.narrow)


distinct = [make(22000 + i) for i in range(min(a.batch, 8))]
pk = pm.setup(distinct[0], 123, 456)
pm.set_hints(pk, distinct[0].hints(2))
partial = distinct[0].partial(r)
marks = np.array([v is None for v in partial[0] + partial[1]], dtype=bool)
full = [np.concatenate([pm.field.fr_limbs(inst), pm.field.fr_limbs(wit)]).reshape(-1, 4) for inst, wit in (c.native(r) for c in distinct)]
want = np.stack([full[i % len(full)] for i in range(a.batch)])
rows = want.copy()
rows[:, marks] = 0xFFFFFFFFFFFFFFFF
xs, ws = np.ascontiguousarray(rows[:, :2]), np.ascontiguousarray(rows[:, 2:])
wall, kernels = [], []
for rep in range(a.reps + 1):
    t0 = time.perf_counter()
    rc, n_bad, _, _ = pk.r1cs_check_batch(xs, ws, 0, solve=True)
    dt = time.perf_counter() - t0
    assert rc == 0 and not n_bad.any(), pm.ctx.last_error()
    if rep == 0:
        print("first call (plan): %.1f ms" % (1e3 * dt))
        assert np.array_equal(pk.solved_assignments(a.batch, ws.shape[1])[a.batch // 2], want[a.batch // 2])
    else:
        wall.append(1e3 * dt)
        kernels.append(pm.ctx.timings()["ntt"])      # slot 1: the solve kernels of the call
spread = lambda v: "%.3f [%.3f .. %.3f]" % (sorted(v)[len(v) // 2], min(v), max(v))
print("%s, opcode %d, (%d, %d, %d), %d hints x %d assignments, %d calls: cached call, wall ms %s; solve kernels, slot 1 ms %s"
      % (a.curve, 1 if a.narrow else 5, n, kD, kE, a.count, a.batch, a.reps, spread(wall), spread(kernels)))
pk.free()
