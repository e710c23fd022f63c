"""Time pm_pk_load_bytes: a ProvingKey::serialize_compressed byte string -> resident key, points decoded on the GPU.

    python tools/pk_load_time.py [--log-gates 20] [--form compressed|uncompressed|both] [--out FILE]

BLS12-381, 2^k - 100 synthetic gates (k = 20: 27.3 M points).  The key is generated on the device and serialised with
Polymath.pk_serialize; after one warm-up, pm_pk_load_bytes is timed three times each with validate 1 and 0 (each run ends
with a stream synchronisation on the loading context), once more with the window tables off (tables = load - that), and
pm_pk_load from already-decoded arrays is timed as today's path without its decoding cost.  The host baseline is
tools/host_deser_time.cpp (the host mirror's deser_g1, one thread) on 10 000 of the key's records, scaled to the key.
The decode kernel's own time comes from a separate `rocprofv3 --kernel-trace --stats` run of this script (--profile-only).
--form uncompressed times the same key as ProvingKey::serialize_uncompressed bytes (pm_pk_load_bytes with PM_WIRE_UNCOMPRESSED:
96-byte records, no square root); --form both times the two byte strings in one process, form by form within every setting, and
--loads-only leaves out the decoded-array and host baselines.  --relations times validate = 1 against validate = 1 | 512
(PM_KEY_CHECK_RELATIONS), alternating, three times per form, and nothing else; PM_PROFILE_HOST=1 prints the check's stage split (each
stage synchronised, so the flagged loads of such a run are not the ones to quote)."""
import argparse
import os
import struct
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--log-gates", type=int, default=20)
ap.add_argument("--out", default=None)
ap.add_argument("--chunk-logs", default="", help="comma list of wire_chunk_log values to time once each (validate 1)")
ap.add_argument("--profile-only", action="store_true", help="one validated load and nothing else (under rocprofv3)")
ap.add_argument("--form", choices=("compressed", "uncompressed", "both"), default="compressed")
ap.add_argument("--loads-only", action="store_true", help="no pm_pk_load-from-arrays and no host baseline")
ap.add_argument("--relations", action="store_true", help="validate 1 against 1 | 512, alternating, and nothing else")
args = ap.parse_args()

from polymath_amd import api, circuits as PC            # noqa: E402
from polymath_amd.polymath import Polymath              # noqa: E402

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


curve = "bls12_381"
nr = (1 << args.log_gates) - 100
pm = Polymath(curve, "merlin", device=0)
c_r = pm.field.r
lc = PC.synthetic_r1cs_native(curve, nr)
g = PC.SplitMix64(0x10AD)
x, z = g.fr(c_r), g.fr(c_r)
t = time.perf_counter()
pk = pm.setup(lc, x, z)
say("key: %d gates, n = %d, %d points; generated in %.2f s" % (nr, pk.n, sum(pk.base_lens), time.perf_counter() - t))
forms = ("compressed", "uncompressed") if args.form == "both" else (args.form,)
vk = pm.make_vk(pk, x, z)
blobs = {}
for form in forms:
    t = time.perf_counter()
    blobs[form] = pm.pk_serialize(pk, lc, vk if form == "compressed" else pm.vk_transcode(vk, "compressed", form), form=form)
    say("pk_serialize %s: %d bytes in %.2f s (matrices serialised in Python)" % (form, len(blobs[form]), time.perf_counter() - t))
data = blobs.get("compressed")
decoded = None if args.profile_only or args.loads_only else [pk.export_bases(v) for v in range(6)]
pk.free()


def sync(k):
    k.export_bases(1, 0, 1)          # a stream synchronisation on the loading context


def load(validate, form=forms[0], relations=False):
    t0 = time.perf_counter()
    k = api.ProvingKey.load_bytes(pm.ctx, curve, blobs[form], validate, form=form, **({"relations": True} if relations else {}))
    sync(k)
    dt = time.perf_counter() - t0
    k.free()
    return dt


if args.profile_only:
    for form in forms:
        say("validated load, %s: %.3f s" % (form, load(True, form)))
        say("unvalidated load, %s: %.3f s" % (form, load(False, form)))
    sys.exit(0)

for form in forms:
    load(True, form)                  # warm-up
if args.relations:
    for form in forms:
        load(True, form, True)
        plain, flagged = [], []
        for _ in range(3):
            plain.append(load(True, form))
            flagged.append(load(True, form, True))
        say("pm_pk_load_bytes %s validate=1:       %s s (best %.3f)" % (form, " ".join("%.3f" % v for v in plain), min(plain)))
        say("pm_pk_load_bytes %s validate=1|512:   %s s (best %.3f)" % (form, " ".join("%.3f" % v for v in flagged), min(flagged)))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0)
for validate in (1, 0):
    for form in forms:
        ts = [load(bool(validate), form) for _ in range(3)]
        say("pm_pk_load_bytes %s validate=%d: %s s (best %.3f)" % (form, validate, " ".join("%.3f" % v for v in ts), min(ts)))
tables = pm.ctx.get_option("tables")
pm.ctx.set_option("tables", "off")
for validate in (1, 0):
    for form in forms:
        ts = [load(bool(validate), form) for _ in range(3)]
        say("pm_pk_load_bytes %s validate=%d, tables off: %s s" % (form, validate, " ".join("%.3f" % v for v in ts)))
pm.ctx.set_option("tables", tables)
for cl in [int(v) for v in args.chunk_logs.split(",") if v]:
    old = pm.ctx.get_option("wire_chunk_log")
    pm.ctx.set_option("wire_chunk_log", cl)
    for form in forms:
        say("pm_pk_load_bytes %s validate=1, wire_chunk_log=%d: %.3f s" % (form, cl, load(True, form)))
    pm.ctx.set_option("wire_chunk_log", old)
if args.loads_only or data is None:   # the baselines below are the compressed form's
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0)
A, B, C = lc.csrs
for _ in range(2):
    t0 = time.perf_counter()
    k = api.ProvingKey.load(pm.ctx, curve, pk.n, lc.m0, lc.mw, lc.nr, pk.sigma, A, B, C, decoded)
    sync(k)
    say("pm_pk_load from decoded arrays (no decoding): %.3f s" % (time.perf_counter() - t0))
    k.free()
# host baseline: deser_g1 of the host mirror on 10 000 of the key's x_powers records
exe = os.path.join(ROOT, "tools", "host_deser_time")
subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tools", "host_deser_time.cpp")])
off = 392 + 24
for _ in range(3):
    rows = struct.unpack_from("<Q", data, off)[0]
    off += 8
    for _ in range(rows):
        off += 8 + 40 * struct.unpack_from("<Q", data, off)[0]
with tempfile.NamedTemporaryFile(suffix=".bin") as f:
    f.write(data[off + 8:off + 8 + 48 * 10000])
    f.flush()
    out = subprocess.run([exe, f.name], capture_output=True, text=True, check=True).stdout
total = sum(len(d) for d in decoded)
for line in out.strip().splitlines():
    us = float(line.split(",")[1].split()[0])
    say("%s -> x %d points = %.0f s on one thread" % (line, total, us * 1e-6 * total))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
