#!/usr/bin/env python3
"""MSM micro-benchmark (SURVEY.md §8d MSM micro-inputs): bases P_i = (i+1)G generated on the device,
uniform scalars, both resident in HBM; prints pairs/s and the HIP-event stage times.
  python tools/msm_bench.py --log-len 22 --reps 3 [--curve bn254]
  python tools/msm_bench.py --batch 256 --log-len 14 --reps 5     B rows of 2^14 pairs: one pm_msm_g1_resident_batch call (a)
      against a loop of B pm_msm_g1_resident calls (b) on the same un-precomputed bases, alternating, in this process"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from polymath_amd import api

ap = argparse.ArgumentParser()
ap.add_argument("--log-len", type=int, default=22)
ap.add_argument("--len", type=int, default=0)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--curve", default="bls12_381")
ap.add_argument("--tables", action="store_true", help="pm_bases_precompute: window tables")
ap.add_argument("--batch", type=int, default=0, help="rows of --len pairs: batch call against a loop of single MSMs")
ap.add_argument("--opt", action="append", default=[], metavar="NAME=VALUE", help="pm_ctx_set_option, e.g. --opt table_window_bits=24 --opt msm_task_len=256")
a = ap.parse_args()
n = a.len or (1 << a.log_len)
ctx = api.Context(0)
for kv in a.opt:
    ctx.set_option(kv.split("=", 1)[0], int(kv.split("=", 1)[1]))
t0 = time.time()
bases = api.Bases.multiples(ctx, a.curve, n)
gen_s = time.time() - t0
t0 = time.time()
if a.tables:
    bases.precompute()
tbl_s = time.time() - t0
g = torch.Generator(device="cuda").manual_seed(1234)
sc = torch.randint(0, 2**62, (n, 4), dtype=torch.int64, device="cuda", generator=g) * 4 + torch.randint(0, 4, (n, 4), dtype=torch.int64, device="cuda", generator=g)
sc[:, 3] &= (1 << 61) - 1          # < 2^253: a valid residue for both scalar fields
torch.cuda.synchronize()
if a.batch:
    B = a.batch
    rows = torch.randint(0, 2**62, (B * n, 4), dtype=torch.int64, device="cuda", generator=g) * 4 + torch.randint(0, 4, (B * n, 4), dtype=torch.int64, device="cuda", generator=g)
    rows[:, 3] &= (1 << 61) - 1
    torch.cuda.synchronize()
    ptr = rows.data_ptr()

    def run_batch():
        t0 = time.perf_counter()
        out, inf = bases.msm_batch(None, 0, n, device_ptr=ptr, batch=B)
        return time.perf_counter() - t0, out, ctx.timings()

    def run_loop():
        t0 = time.perf_counter()
        outs = [bases.msm(None, 0, n, device_ptr=ptr + 32 * n * b)[0] for b in range(B)]
        return time.perf_counter() - t0, np.stack(outs), None

    _, ob, _ = run_batch()                  # warm-up of both (allocations, first launches) and the equality check
    _, ol, _ = run_loop()
    same = bool(np.array_equal(ob, ol))
    ta, tb, tm = [], [], None
    for rep in range(a.reps):               # alternating
        dt, _, tm = run_batch()
        ta.append(dt)
        tb.append(run_loop()[0])
    med = lambda v: sorted(v)[len(v) // 2]
    print(json.dumps({"curve": a.curve, "len": n, "batch": B, "pairs": B * n, "rows_equal": same,
                      "batch_ms": [round(t * 1e3, 3) for t in ta], "loop_ms": [round(t * 1e3, 3) for t in tb],
                      "batch_median_ms": round(med(ta) * 1e3, 3), "loop_median_ms": round(med(tb) * 1e3, 3),
                      "batch_mpairs_per_s": round(B * n / med(ta) / 1e6, 2), "loop_mpairs_per_s": round(B * n / med(tb) / 1e6, 2),
                      "loop_spread_ms": round((max(tb) - min(tb)) * 1e3, 3), "batch_spread_ms": round((max(ta) - min(ta)) * 1e3, 3),
                      "batch_stage_ms": {k: round(v, 3) for k, v in tm.items() if k.startswith("msm")}}))
    sys.exit(0 if same else 1)
out = None
res = []
for rep in range(a.reps + 1):
    t0 = time.perf_counter()
    out, inf = bases.msm(None, 0, n, device_ptr=sc.data_ptr())
    dt = time.perf_counter() - t0
    tm = ctx.timings()
    if rep:
        res.append((dt, tm))
best = min(r[0] for r in res)
tm = res[-1][1]
print(json.dumps({"curve": a.curve, "len": n, "best_ms": best * 1e3, "pairs_per_sec": n / best, "gen_s": gen_s, "tables": a.tables, "tables_s": tbl_s,
                  "options": {k: ctx.get_option(k) for k in api.OPTIONS},
                  "stage_ms": {k: round(v, 3) for k, v in tm.items() if k.startswith("msm")}}))
