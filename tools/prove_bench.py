#!/usr/bin/env python3
"""Batch prover against a loop of single proofs: one key, B device-resident assignments of one circuit, alternating in this process
  (a) one pm_host_prove_batch call of B proofs            (b) a loop of B pm_host_prove calls (device pointers)
and printing proofs/s for both plus the stage split of pm_last_timings (summed over the batch for (a); one proof for (b)).
  python tools/prove_bench.py --circuit mimc322 --batch 256 --reps 5
  python tools/prove_bench.py --circuit bench:32000 --batch 16 --reps 3        BenchCircuit with 32000 constraints: n = 2^16
The B rows cycle through min(B, 32) distinct seeded assignments with distinct r_a (a proof's cost does not depend on its values).
  python tools/prove_bench.py --circuit mimc322 --batch 256 --reps 5 --solve
compares inputs -> proofs instead (mimcK and arx only), host limbs in both routes, alternating in this process:
  (a) the B assignments synthesised on the host (generate_constraints, Python integers), then one pm_host_prove_batch call
  (b) B partial assignments (the inputs given, everything else the unknown marker), one pm_host_prove_batch call with PM_ASSIGNMENT_SOLVE
Every rep of (a) synthesises all B assignments again: that is the step (b) moves to the GPU.
  python tools/prove_bench.py --circuit arx --batch 256 --reps 5 --solve        ArxDemo, 32-bit words, 8 rounds; arx:W:R for others
is the same comparison on a boolean circuit (bit decompositions, XOR rows), and
  python tools/prove_bench.py --circuit matchcount --batch 256 --reps 5 --solve  MatchCount, 1024 values, arkworks' form;
                                                                                 matchcount:N:FORM (FORM = ark or circom) for others
on one that tests equality (one dependency level of N is-zero pairs; about half of the values match), and
  python tools/prove_bench.py --circuit divrem --batch 256 --reps 5 --solve      DivRem, 256 divisions of 32-bit operands;
                                                                                 divrem:N:BITS for others
on one that divides integers (one dependency level of N Euclidean division rows, then 3 N range checks; route (b) marks the
quotients with the quotient marker), and
  python tools/prove_bench.py --circuit tablewalk --batch 256 --reps 5 --solve   TableWalk, a table of 64 signals walked for 32 steps;
                                                                                 tablewalk:WIDTH:STEPS for others
on one that reads a table at a signal (per step one level of WIDTH indicator rows, the decoder's sum and WIDTH products, the next
index; route (b) marks the decoders' outputs with the indicator marker), and
  python tools/prove_bench.py --circuit decompress --batch 256 --reps 5 --solve  EdwardsDecompress, 32 points of Jubjub / Baby Jubjub;
                                                                                 decompress:POINTS for others
on one that decompresses curve points (per point a division, one square-root row, a product and a decomposition of the root into
bitlength(r) - 1 bits; route (b) marks the roots with the square-root marker), and
  python tools/prove_bench.py --circuit limbproduct --batch 256 --reps 5 --solve LimbProduct, 64 products of 8-limb numbers;
                                                                                 limbproduct:COUNT:LIMBS for others
on one that multiplies non-native numbers (one dependency level of COUNT linear blocks of 2 LIMBS - 1 unknowns through one shared
inverse, then the sums; no marker: the rows determine the product's limbs), and
  python tools/prove_bench.py --circuit modmul --batch 256 --reps 5 --solve      LimbModMul, 16 multiplications modulo a 256-bit prime on
                                                                                 4 limbs of 64 bits; modmul:COUNT:N:LIMBS for others
on one that multiplies in a foreign field (per multiplication a linear block, one declared long division -- the key's hints are set
from the circuit's hints() -- 2 LIMBS decompositions of N bits, the limbs of q p and a chain of carries; route (a) synthesises q and
rem with Python's divmod).  UNMEASURED: no run of it is recorded.
  python tools/prove_bench.py --circuit moddiv --batch 256 --reps 5 --solve      LimbModDiv, 16 divisions modulo secp256k1's prime on
                                                                                 4 limbs of 64 bits; moddiv:COUNT:N:LIMBS for others
  python tools/prove_bench.py --circuit ecadd --batch 256 --reps 5 --solve       EcAddChain, 4 affine additions on secp256k1 from
                                                                                 (k + 5) G and 2 G; ecadd:STEPS for others
on circuits that divide in a foreign field (a declared modular division per quotient or slope, then the product's block and a
declared long division per reduction, with their decompositions and carries; route (a) synthesises with Python's pow and divmod).
  python tools/prove_bench.py --circuit modmuldiv --batch 256 --reps 5 --solve   LimbModMulDiv, 16 multiply-divides (all six lists, cN = 3,
                                                                                 cD = 2) modulo secp256k1's prime on 4 limbs of 64 bits;
                                                                                 modmuldiv:COUNT:N:LIMBS for others
  python tools/prove_bench.py --circuit ecdouble --batch 256 --reps 5 --solve    EcDoubleAddChain, 4 times R <- 2 R + G on secp256k1 from
                                                                                 (k + 5) G; ecdouble:STEPS for others
  python tools/prove_bench.py --circuit ecdsa:toy --batch 16 --reps 3 --solve    EcdsaVerify on the tests' toy curve (p = 2^22 - 3, 22 scalar
                                                                                 bits, a key of 2^15); --circuit ecdsa is secp256k1 on 4 limbs of
                                                                                 64 bits: about 1.7 M rows, a key of 2^21, minutes of Python
                                                                                 synthesis per assignment
on circuits whose slopes have a product for their numerator (a declared modular multiply-divide per tangent; ECDSA verification is
every hint opcode but the wide one, decompositions, selections and blocks in one system).  UNMEASURED: no run of them is recorded.
  python tools/prove_bench.py --circuit rsa --batch 64 --reps 5 --solve          RsaVerify, s^65537 mod a 2048-bit modulus on 32 limbs
                                                                                 of 64 bits; rsa:BITS:N:LIMBS for others (rsa:2048:121:17)
  python tools/prove_bench.py --circuit widediv --batch 256 --reps 5 --solve     LimbDivision, 16 wide divisions of 63 by 32 limbs of
                                                                                 64 bits; widediv:COUNT:N:KD:KE for others
on circuits that divide wide integers (RSA: per modular multiplication a linear block of 2 LIMBS - 1 unknowns, one declared WIDE long
division, the limbs of q N and a chain of carries, 17 multiplications deep; route (a) synthesises with Python's divmod).
  python tools/prove_bench.py --circuit mimc322 --batch 256 --reps 5 --solve --reorder reverse     or --reorder SEED
runs either --solve comparison on the same circuit with its constraint rows stored in another order (circuits.Reordered: reversed, or
shuffled by SEED; a matchcount gadget moves as a block so that every opener stays before its closer).  Route (b) then goes through the
solver's any-order planner and the reordered plan's stuck key; route (a) is unchanged work.  UNMEASURED: no run of it is recorded.
  python tools/prove_bench.py --circuit mimc322 --batch 256 --reps 5 --glue device
compares the two glue modes of the batch call itself, alternating in this process, same key, same device-resident assignments:
  (a) pm_host_prove_batch, host glue (about six synchronisations a group)   (b) the same call with PM_PROVE_GLUE_DEVICE (one a group)
and prints proofs/s, the spread over the reps, the stage split of both and whether the two outputs are the same bytes."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from polymath_amd import circuits as PC
from polymath_amd.polymath import Polymath

ap = argparse.ArgumentParser()
ap.add_argument("--circuit", default="mimc322", help="mimcK (K round constants), bench:NC (BenchCircuit, NC constraints), arx[:WIDTH:ROUNDS] (ArxDemo), matchcount[:N:FORM] (MatchCount), divrem[:N:BITS] (DivRem), tablewalk[:WIDTH:STEPS] (TableWalk), decompress[:POINTS] (EdwardsDecompress), limbproduct[:COUNT:LIMBS] (LimbProduct), modmul[:COUNT:N:LIMBS] (LimbModMul), moddiv[:COUNT:N:LIMBS] (LimbModDiv), ecadd[:STEPS] (EcAddChain), rsa[:BITS:N:LIMBS] (RsaVerify), widediv[:COUNT:N:KD:KE] (LimbDivision), modmuldiv[:COUNT:N:LIMBS] (LimbModMulDiv), ecdouble[:STEPS] (EcDoubleAddChain) or ecdsa[:toy] (EcdsaVerify)")
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--curve", default="bls12_381")
ap.add_argument("--transcript", default="merlin")
ap.add_argument("--opt", action="append", default=[], metavar="NAME=VALUE", help="pm_ctx_set_option before the key is made, e.g. --opt tables=0")
ap.add_argument("--glue", choices=("host", "device"), default="host", help="device: host glue against device glue of the batch call")
ap.add_argument("--solve", action="store_true", help="host-synthesised assignments against partial assignments solved on the GPU")
ap.add_argument("--reorder", default=None, metavar="reverse|SEED", help="with --solve: the circuit's rows stored reversed or shuffled by SEED (unmeasured)")
a = ap.parse_args()
if a.solve and not a.circuit.startswith(("mimc", "arx", "matchcount", "divrem", "tablewalk", "decompress", "limbproduct", "modmul", "moddiv", "ecadd", "rsa", "widediv", "ecdouble", "ecdsa")):
    ap.error("--solve needs a mimcK, an arx, a matchcount, a divrem, a tablewalk, a decompress, a limbproduct, a modmul, a moddiv, a modmuldiv, an ecadd, an ecdouble, an ecdsa, an rsa or a widediv circuit")
if a.reorder is not None and not a.solve:
    ap.error("--reorder goes with --solve")
pm = Polymath(a.curve, a.transcript, device=0)
for kv in a.opt:
    pm.ctx.set_option(kv.split("=", 1)[0], int(kv.split("=", 1)[1]))
r = pm.field.r
g = PC.SplitMix64(20260117)
if a.circuit.startswith("mimc"):
    consts = [g.fr(r) for _ in range(int(a.circuit[4:]))]
    make = lambda: PC.MiMCDemo(g.fr(r), g.fr(r), consts)
    again = lambda c: PC.MiMCDemo(c.xl, c.xr, consts)
    partial_of = lambda c: ([1, None], [c.xl, c.xr] + [None] * (mw - 2))
elif a.circuit.startswith("arx"):
    width, rounds = (int(v) for v in a.circuit.split(":")[1:3]) if ":" in a.circuit else (32, 8)
    make = lambda: PC.ArxDemo(g.next_u64() % (1 << width), g.next_u64() % (1 << width), width, rounds, 7 % width or 1)
    again = lambda c: PC.ArxDemo(c.a, c.b, c.width, c.rounds, c.rot)
    partial_of = lambda c: c.partial(r)
elif a.circuit.startswith("matchcount"):
    n_values, form = (int(a.circuit.split(":")[1]), a.circuit.split(":")[2]) if ":" in a.circuit else (1024, "ark")

    def make():
        key = g.fr(r)
        return PC.MatchCount([key if g.next_u64() & 1 else g.fr(r) for _ in range(n_values)], key, form)
    again = lambda c: PC.MatchCount(c.values, c.key, c.form)
    partial_of = lambda c: c.partial(r)
elif a.circuit.startswith("divrem"):
    n_div, bits = (int(v) for v in a.circuit.split(":")[1:3]) if ":" in a.circuit else (256, 32)
    make = lambda: PC.DivRem([(g.next_u64() % (1 << bits), 1 + g.next_u64() % ((1 << bits) - 1)) for _ in range(n_div)], bits)
    again = lambda c: PC.DivRem(c.pairs, c.bits)
    partial_of = lambda c: c.partial(r)
elif a.circuit.startswith("tablewalk"):
    width, walk_steps = (int(v) for v in a.circuit.split(":")[1:3]) if ":" in a.circuit else (64, 32)
    make = lambda: PC.TableWalk([g.next_u64() % width for _ in range(width)], g.next_u64() % width, walk_steps)
    again = lambda c: PC.TableWalk(c.table, c.start, c.steps, c.signals)
    partial_of = lambda c: c.partial(r)
elif a.circuit.startswith("decompress"):
    n_points = int(a.circuit.split(":")[1]) if ":" in a.circuit else 32
    make = lambda: PC.EdwardsDecompress(PC.edwards_ys(r, n_points, g.next_u64()), [g.next_u64() & 1 for _ in range(n_points)])
    again = lambda c: PC.EdwardsDecompress(c.ys, c.signs)
    partial_of = lambda c: c.partial(r)
elif a.circuit.startswith("limbproduct"):
    n_products, n_limbs = (int(v) for v in a.circuit.split(":")[1:3]) if ":" in a.circuit else (64, 8)
    make = lambda: PC.LimbProduct(PC.limb_products(r, n_products, n_limbs, g.next_u64()))
    again = lambda c: PC.LimbProduct(c.products, c.first)
    partial_of = lambda c: c.partial(r)
elif a.circuit.startswith("modmuldiv"):
    n_divs, limb_bits, n_limbs = (int(v) for v in a.circuit.split(":")[1:4]) if ":" in a.circuit else (16, 64, 4)
    foreign = (1 << (limb_bits * n_limbs)) - 2 ** 32 - 977 if limb_bits * n_limbs == 256 else (1 << (limb_bits * n_limbs - 3)) - 1     # as for modmul; need not be a prime
    make = lambda: PC.LimbModMulDiv(PC.modmuldiv_cases(foreign, n_divs, g.next_u64(), cD=2), foreign, limb_bits, n_limbs, 3, 2)
    again = lambda c: PC.LimbModMulDiv(c.cases, c.modulus, c.n, c.limbs, c.cN, c.cD, c.decompose, c.operand_bits)
    partial_of = lambda c: c.partial(r)
elif a.circuit.startswith("ecdouble"):
    ec_steps = int(a.circuit.split(":")[1]) if ":" in a.circuit else 4
    secp, _, _, G1 = PC.SECP256K1
    make = lambda: PC.EcDoubleAddChain(PC.affine_mul(secp, 5 + g.next_u64() % 32, G1), G1, secp, 64, 4, ec_steps)      # the generator asserts that no step is exceptional
    again = lambda c: PC.EcDoubleAddChain(c.point, c.addend, c.modulus, c.n, c.limbs, c.steps, c.decompose)
    partial_of = lambda c: c.partial(r)
elif a.circuit.startswith("ecdsa"):
    ec_curve, (limb_bits, n_limbs) = (PC.TOY_CURVE, (11, 2)) if a.circuit.endswith(":toy") else (PC.SECP256K1, (64, 4))
    signatures = iter(PC.ecdsa_cases(ec_curve, min(a.batch, 32), g.next_u64()))
    make = lambda: PC.EcdsaVerify(ec_curve, *next(signatures), limb_bits, n_limbs)
    again = lambda c: PC.EcdsaVerify(c.curve, c.Q, c.h, c.r_sig, c.s, c.n, c.limbs, c.start, c.decompose)
    partial_of = lambda c: c.partial(r)
elif a.circuit.startswith("modmul"):
    n_muls, limb_bits, n_limbs = (int(v) for v in a.circuit.split(":")[1:4]) if ":" in a.circuit else (16, 64, 4)
    foreign = (1 << (limb_bits * n_limbs)) - 2 ** 32 - 977 if limb_bits * n_limbs == 256 else (1 << (limb_bits * n_limbs - 3)) - 1     # secp256k1's prime at 256 bits, else a modulus of the limbs' size
    make = lambda: PC.LimbModMul(PC.modmul_pairs(foreign, n_muls, g.next_u64()), foreign, limb_bits, n_limbs)
    again = lambda c: PC.LimbModMul(c.pairs, c.modulus, c.n, c.limbs, c.decompose)
    partial_of = lambda c: c.partial(r)
elif a.circuit.startswith("moddiv"):
    n_divs, limb_bits, n_limbs = (int(v) for v in a.circuit.split(":")[1:4]) if ":" in a.circuit else (16, 64, 4)
    foreign = (1 << (limb_bits * n_limbs)) - 2 ** 32 - 977 if limb_bits * n_limbs == 256 else (1 << (limb_bits * n_limbs - 3)) - 1     # as for modmul; need not be a prime
    make = lambda: PC.LimbModDiv(PC.moddiv_cases(foreign, n_divs, g.next_u64()), foreign, limb_bits, n_limbs)
    again = lambda c: PC.LimbModDiv(c.cases, c.modulus, c.n, c.limbs, c.decompose, c.operand_bits)
    partial_of = lambda c: c.partial(r)
elif a.circuit.startswith("ecadd"):
    ec_steps = int(a.circuit.split(":")[1]) if ":" in a.circuit else 4
    secp = 2 ** 256 - 2 ** 32 - 977
    G1 = (0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798, 0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8)

    def ec_add(p1, p2):      # affine addition or doubling on y^2 = x^3 + 7
        (x1, y1), (x2, y2) = p1, p2
        lam = (3 * x1 * x1) * pow(2 * y1, -1, secp) % secp if p1 == p2 else (y2 - y1) * pow(x2 - x1, -1, secp) % secp
        x3 = (lam * lam - x1 - x2) % secp
        return x3, (lam * (x1 - x3) - y1) % secp
    ec_points = [G1]
    for _ in range(40):
        ec_points.append(ec_add(ec_points[-1], G1))
    make = lambda: PC.EcAddChain(ec_points[4 + g.next_u64() % 32], ec_points[1], secp, 64, 4, ec_steps)      # R_t = (k + 5 + 2 t) G, k < 32, is never +-2 G: no chord without a slope
    again = lambda c: PC.EcAddChain(c.point, c.addend, c.modulus, c.n, c.limbs, c.steps, c.decompose)
    partial_of = lambda c: c.partial(r)
elif a.circuit.startswith("rsa"):
    rsa_bits, limb_bits, n_limbs = (int(v) for v in a.circuit.split(":")[1:4]) if ":" in a.circuit else (2048, 64, 32)
    rsa_n = PC.rsa_modulus(rsa_bits, g.next_u64())[0]          # one key, one literal modulus: the assignments differ in the signature
    make = lambda: PC.RsaVerify(PC.rsa_modulus(rsa_bits, g.next_u64())[1] % rsa_n, rsa_n, limb_bits, n_limbs)
    again = lambda c: PC.RsaVerify(c.signature, c.modulus, c.n, c.limbs, c.squarings, c.witness_modulus, c.decompose)
    partial_of = lambda c: c.partial(r)
elif a.circuit.startswith("widediv"):
    n_divs, limb_bits, k_d, k_e = (int(v) for v in a.circuit.split(":")[1:5]) if ":" in a.circuit else (16, 64, 63, 32)
    draw = lambda bits: sum(g.next_u64() << (64 * i) for i in range(-(-bits // 64))) & ((1 << bits) - 1)
    make = lambda: PC.LimbDivision([(PC.int_limbs(draw(limb_bits * k_d), limb_bits, k_d), PC.int_limbs(draw(limb_bits * k_e) | 1 << (limb_bits * k_e - 1), limb_bits, k_e))
                                    for _ in range(n_divs)], limb_bits, k_d, k_e)
    again = lambda c: PC.LimbDivision(c.cases, c.n, c.kq, c.kr, c.divisor, c.wide, c.stuck)
    partial_of = lambda c: c.partial(r)
else:
    nc = int(a.circuit.split(":", 1)[1])
    make = lambda: PC.BenchCircuit(g.fr(r), g.fr(r), 10, nc)
if a.reorder is None:
    stored = lambda c: c
else:       # the same variables and values, the rows in another order; `circuits` keeps the inner generators (partial_of, again)
    order = "reverse" if a.reorder == "reverse" else int(a.reorder)
    blocks = {"ark": 3, "circom": 2}[form] if a.circuit.startswith("matchcount") else 1
    stored = lambda c: PC.Reordered(c, order, blocks=blocks)
B, distinct = a.batch, min(a.batch, 32)
circuits = [make() for _ in range(distinct)]
t0 = time.time()
pk = pm.setup(stored(circuits[0]), g.fr(r), g.fr(r))
setup_s = time.time() - t0
if a.circuit.startswith(("modmul", "moddiv", "ecadd", "rsa", "widediv", "ecdouble", "ecdsa")):
    pm.set_hints(pk, circuits[0].hints(2))       # the long and the modular divisions are part of the circuit: declared once, with the key
rows = []
for c in circuits:
    _, inst, wit = pm._synthesize(stored(c))
    rows.append((pm.field.fr_limbs(inst), pm.field.fr_limbs(wit), [g.fr(r), g.fr(r)]))
pick = [i % distinct for i in range(B)]
xs = np.ascontiguousarray(np.stack([rows[i][0] for i in pick]))
ws = np.ascontiguousarray(np.stack([rows[i][1] for i in pick]))
ras = np.ascontiguousarray(np.stack([pm.field.fr_limbs(rows[i][2]) for i in pick]))
dx = torch.from_numpy(xs.view(np.int64)).cuda()
dw = torch.from_numpy(ws.view(np.int64)).cuda()
torch.cuda.synchronize()
m0, mw = xs.shape[1], ws.shape[1]


def solve_comparison():
    inputs = [circuits[i] for i in pick]
    ra_all = [rows[i][2] for i in pick]
    partial = [pm.partial_limbs(*partial_of(c)) for c in inputs]

    def run_host():
        t0 = time.perf_counter()
        t_syn = 0.0
        full = []
        for c in inputs:
            _, inst, wit = pm._synthesize(stored(again(c)))
            full.append((pm.field.fr_limbs(inst), pm.field.fr_limbs(wit)))
        t_syn = time.perf_counter() - t0
        proofs, status = pm.prove_batch(pk, full, ra_all)
        assert not any(status)
        return time.perf_counter() - t0, t_syn, proofs, pm.ctx.timings()

    def run_solve():
        t0 = time.perf_counter()
        proofs, status, _ = pm.prove_batch(pk, partial, ra_all, solve=True)
        assert not any(status)
        return time.perf_counter() - t0, proofs, pm.ctx.timings()

    _, _, ph, _ = run_host()
    _, ps, _ = run_solve()
    th, tsyn, tsv = [], [], []
    for _ in range(a.reps):
        dt, syn, _, tm_host = run_host()
        th.append(dt)
        tsyn.append(syn)
        dt, _, tm_solve = run_solve()
        tsv.append(dt)
    print(json.dumps({"curve": a.curve, "circuit": a.circuit, "reorder": a.reorder, "n": pk.n, "batch": B, "bytes_equal": ph == ps, "setup_s": round(setup_s, 3),
                      "host_synthesis_ms": [round(t * 1e3, 3) for t in th], "of_which_synthesis_ms": [round(t * 1e3, 3) for t in tsyn],
                      "solve_ms": [round(t * 1e3, 3) for t in tsv],
                      "host_proofs_per_s": round(B / med(th), 1), "solve_proofs_per_s": round(B / med(tsv), 1),
                      "solve_over_host": round(med(th) / med(tsv), 3),
                      "host_stage_ms_sum_over_batch": {k: round(v, 3) for k, v in tm_host.items()},
                      "solve_stage_ms_sum_over_batch": {k: round(v, 3) for k, v in tm_solve.items()}}))


med = lambda v: sorted(v)[len(v) // 2]
if a.solve:
    solve_comparison()
    sys.exit(0)


def run_batch(glue="host"):
    t0 = time.perf_counter()
    rc, data, status = pk.host_prove_batch(a.transcript, xs, dx.data_ptr(), dw.data_ptr(), ras, on_device=True, glue=glue)
    dt = time.perf_counter() - t0
    assert rc == 0 and not status.any(), (rc, status)
    return dt, data, pm.ctx.timings()


def glue_comparison():
    _, dh, _ = run_batch("host")        # warm-up of both modes and the equality check
    _, dd, _ = run_batch("device")
    th, td = [], []
    for _ in range(a.reps):
        dt, _, tm_host = run_batch("host")
        th.append(dt)
        dt, _, tm_dev = run_batch("device")
        td.append(dt)
    spread = lambda v: round((max(v) - min(v)) / med(v), 4)
    print(json.dumps({"curve": a.curve, "circuit": a.circuit, "transcript": a.transcript, "n": pk.n, "batch": B, "bytes_equal": dh == dd,
                      "setup_s": round(setup_s, 3),
                      "host_glue_ms": [round(t * 1e3, 3) for t in th], "device_glue_ms": [round(t * 1e3, 3) for t in td],
                      "host_glue_proofs_per_s": round(B / med(th), 1), "device_glue_proofs_per_s": round(B / med(td), 1),
                      "host_glue_spread": spread(th), "device_glue_spread": spread(td),
                      "device_over_host": round(med(th) / med(td), 3),
                      "host_glue_stage_ms_sum_over_batch": {k: round(v, 3) for k, v in tm_host.items()},
                      "device_glue_stage_ms_sum_over_batch": {k: round(v, 3) for k, v in tm_dev.items()}}))


if a.glue == "device":
    glue_comparison()
    sys.exit(0)


def run_loop():
    out = []
    t0 = time.perf_counter()
    for i in range(B):
        rc, proof = pk.host_prove(a.transcript, xs[i], dx.data_ptr() + 32 * m0 * i, dw.data_ptr() + 32 * mw * i, ras[i], on_device=True)
        assert rc == 0
        out.append(proof)
    dt = time.perf_counter() - t0
    return dt, b"".join(out), pm.ctx.timings()


_, db, _ = run_batch()                  # warm-up of both routes (allocations, twiddles, first launches) and the equality check
_, dl, _ = run_loop()
ta, tb = [], []
for _ in range(a.reps):
    dt, _, tm_batch = run_batch()
    ta.append(dt)
    dt, _, tm_one = run_loop()
    tb.append(dt)
print(json.dumps({"curve": a.curve, "circuit": a.circuit, "n": pk.n, "batch": B, "bytes_equal": db == dl, "setup_s": round(setup_s, 3),
                  "batch_ms": [round(t * 1e3, 3) for t in ta], "loop_ms": [round(t * 1e3, 3) for t in tb],
                  "batch_proofs_per_s": round(B / med(ta), 1), "loop_proofs_per_s": round(B / med(tb), 1),
                  "batch_over_loop": round(med(tb) / med(ta), 3),
                  "batch_stage_ms_sum_over_batch": {k: round(v, 3) for k, v in tm_batch.items()},
                  "loop_stage_ms_last_proof": {k: round(v, 3) for k, v in tm_one.items()}}))
