"""GPU: pm_host_prove_batch (Polymath.prove_batch) -- many assignments of one circuit against one resident key in one call.
The bar is equality of bytes: every row of a batch equals pm_host_prove (prove_native) of that row and the CPU oracle's proof of
that row.  Shapes are the smallest at which each mechanism can differ: n = 2^7 (dense transforms; the division scan is two chunked
levels of 82 and 6 values under its one-lane top), 2^10 (the last dense domain), 2^11 (the first reduced-radix tile domain: two
passes of 6 + 5 stages), 2^13 (two tile passes of 7 + 6 stages); counts that are one group, several groups (msm_max_piece_log) and
the per-proof fallback."""
import ctypes as ct

import numpy as np
import pytest

from helpers import I, load_golden, r1cs_from_json
from oracle import driver as DR
from oracle.pyref import circuits as CI, serialize as SE, transcripts as T
from oracle.pyref.fields import CURVES

pytestmark = pytest.mark.gpu

PM_OK, PM_ERR_INVALID_ARG, PM_ERR_REMAINDER_NONZERO = 0, 1, 4
PROOF_LEN = {"bls12_381": 176, "bn254": 128}
_KEYS = {}


def _assignment(curve, shape, g):
    c = CURVES[curve]
    if shape[0] == "mimc":
        return CI.mimc_circuit(c, g.fr(c.r), g.fr(c.r), _consts(curve, shape[1]))
    return CI.bench_circuit(c, g.fr(c.r), g.fr(c.r), 10, shape[1])


def _consts(curve, count):
    g = CI.SplitMix64(4000 + count)
    return [g.fr(CURVES[curve].r) for _ in range(count)]


SHAPES = {"mimc16": (("mimc", 16), 1 << 7), "mimc322": (("mimc", 322), 1 << 11), "bench2p10": (("bench", 500), 1 << 10),
          "bench2p13": (("bench", 4000), 1 << 13)}


def _key(gpu_ctx, oracle, curve, shape_name, rows, tables="auto"):
    """one GPU key and one oracle key per (curve, shape); `rows` seeded assignments with their r_a, limbs, single-prover bytes (per
    transcript, on demand) -- computed once and shared by the tests"""
    from polymath_amd import polymath as PM
    k = (curve, shape_name, tables)
    if k not in _KEYS:
        shape, n = SHAPES[shape_name]
        g = CI.SplitMix64(77 + len(shape_name))
        c = CURVES[curve]
        x, z = g.fr(c.r), g.fr(c.r)
        q, inst, wit = _assignment(curve, shape, g)
        pm = PM.Polymath(curve, "merlin", ctx=gpu_ctx)
        gpu_ctx.set_option("tables", tables)                     # restored by conftest; read at key generation
        pk = pm.setup((PM.R1CS(q.m0, q.mw, q.a, q.b, q.c), inst, wit), x, z)
        assert pk.n == n, (shape_name, pk.n)
        _KEYS[k] = dict(pk=pk, q=q, x=x, z=z, g=g, shape=shape, rows=[], pm={"merlin": pm}, opk=None, single={}, oracle={})
    s = _KEYS[k]
    c = CURVES[curve]
    while len(s["rows"]) < rows:
        q, inst, wit = _assignment(curve, s["shape"], s["g"])
        f = s["pm"]["merlin"].field
        s["rows"].append(dict(inst=inst, wit=wit, r_a=[s["g"].fr(c.r), s["g"].fr(c.r)], xl=f.fr_limbs(inst), wl=f.fr_limbs(wit)))
    return s


def _pm(s, gpu_ctx, curve, transcript):
    from polymath_amd import polymath as PM
    if transcript not in s["pm"]:
        s["pm"][transcript] = PM.Polymath(curve, transcript, ctx=gpu_ctx)
    return s["pm"][transcript]


def _single(s, gpu_ctx, curve, transcript, i):
    if (transcript, i) not in s["single"]:
        row = s["rows"][i]
        s["single"][(transcript, i)] = _pm(s, gpu_ctx, curve, transcript).prove_native(s["pk"], row["xl"], row["wl"], row["r_a"])
    return s["single"][(transcript, i)]


def _oracle_bytes(s, oracle, curve, transcript, i):
    if (transcript, i) not in s["oracle"]:
        c = CURVES[curve]
        if s["opk"] is None:
            s["opk"] = oracle.OraclePk(curve, s["q"], s["x"], s["z"], 8)
        opk, row = s["opk"], s["rows"][i]
        omega = oracle.fr_from_mont_limbs(curve, opk.omega_limbs)[0]
        proof = DR.prove(opk, opk.n, opk.sigma, omega, row["inst"], row["wit"], row["r_a"], T.make_transcripts(c)[transcript])
        s["oracle"][(transcript, i)] = SE.ser_proof(c, proof)
    return s["oracle"][(transcript, i)]


def _batch(s, gpu_ctx, curve, transcript, idx, **kw):
    rows = [s["rows"][i] for i in idx]
    return _pm(s, gpu_ctx, curve, transcript).prove_batch(s["pk"], [(r["xl"], r["wl"]) for r in rows], [r["r_a"] for r in rows], **kw)


# ---- 1. bytes equal the single prover and the oracle -----------------------------------------------------------------------------
@pytest.mark.parametrize("curve,shape_name,counts,transcripts", [
    ("bls12_381", "mimc16", (1, 2, 5, 33), ("merlin", "keccak256", "blake3")),
    ("bn254", "mimc16", (2, 5), ("merlin",)),
    ("bls12_381", "mimc322", (3,), ("merlin",)),
    ("bn254", "mimc322", (4,), ("merlin",)),
    ("bls12_381", "bench2p10", (5,), ("merlin",)),
    ("bls12_381", "bench2p13", (3,), ("merlin",)),
])
def test_bytes_equal_single_prover_and_oracle(gpu_ctx, oracle, curve, shape_name, counts, transcripts):
    s = _key(gpu_ctx, oracle, curve, shape_name, max(counts))
    for transcript in transcripts:
        for count in counts if transcript == "merlin" else (min(counts, key=lambda v: abs(v - 3)),):
            proofs, status = _batch(s, gpu_ctx, curve, transcript, range(count))
            assert status == [PM_OK] * count, (transcript, count, status)
            for i in range(count):
                assert len(proofs[i]) == PROOF_LEN[curve]
                assert proofs[i] == _single(s, gpu_ctx, curve, transcript, i), (transcript, count, i, "single prover")
                assert proofs[i] == _oracle_bytes(s, oracle, curve, transcript, i), (transcript, count, i, "oracle")


# ---- 2. golden fixtures -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["proofs.json", "proofs_bn254.json"])
def test_golden_fixtures(gpu_ctx, name):
    from polymath_amd import polymath as PM
    seen = set()
    for fx in load_golden(name):
        curve = fx["curve"]
        q = r1cs_from_json(fx["r1cs"])
        inst, wit, r_a = [I(v) for v in fx["instance"]], [I(v) for v in fx["witness"]], [I(v) for v in fx["r_a"]]
        pk = None
        for tname, ref in fx["proofs"].items():
            pm = PM.Polymath(curve, tname, ctx=gpu_ctx)
            if pk is None:
                pk = pm.setup((PM.R1CS(q.m0, q.mw, q.a, q.b, q.c), inst, wit), I(fx["x_trapdoor"]), I(fx["z_trapdoor"]))
            xl, wl = pm.field.fr_limbs(inst), pm.field.fr_limbs(wit)
            proofs, status = pm.prove_batch(pk, [(xl, wl)] * 3, [r_a] * 3)
            assert status == [0, 0, 0] and [p.hex() for p in proofs] == [ref["bytes"]] * 3, (fx["name"], tname, status)
        pk.free()
        seen.add(q.m0)
    assert seen >= ({1, 2, 3, 12} if name == "proofs.json" else {2})      # 2 m0 <= 16: the sparse sum; m0 = 12: the fifth transform


# ---- 3. per-proof status ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad_at", [2, 0, 4])
def test_per_proof_status(gpu_ctx, oracle, bad_at):
    from polymath_amd import polymath as PM
    curve = "bls12_381"
    s = _key(gpu_ctx, oracle, curve, "mimc16", 5)
    pm = _pm(s, gpu_ctx, curve, "merlin")
    rows = [dict(r) for r in s["rows"][:5]]
    wit = list(rows[bad_at]["wit"])
    wit[3] = (wit[3] + 1) % pm.field.r
    rows[bad_at]["wl"] = pm.field.fr_limbs(wit)
    with pytest.raises(PM.PolymathProverError) as e:
        pm.prove_native(s["pk"], rows[bad_at]["xl"], rows[bad_at]["wl"], rows[bad_at]["r_a"])
    xs, ws = np.stack([r["xl"] for r in rows]), np.stack([r["wl"] for r in rows])
    ra = np.stack([pm.field.fr_limbs(r["r_a"]) for r in rows])
    rc, data, status = s["pk"].host_prove_batch("merlin", xs, xs, ws, ra)
    assert rc == PM_OK
    assert status[bad_at] == e.value.status and e.value.status != 0
    assert data[bad_at * 176:(bad_at + 1) * 176] == bytes(176)
    for i in range(5):
        if i != bad_at:
            assert status[i] == 0 and data[i * 176:(i + 1) * 176] == _single(s, gpu_ctx, curve, "merlin", i), i
    proofs, st = pm.prove_batch(s["pk"], [(r["xl"], r["wl"]) for r in rows], [r["r_a"] for r in rows])
    assert proofs[bad_at] is None and st[bad_at] == e.value.status and all(p is not None for i, p in enumerate(proofs) if i != bad_at)


# ---- 4. group split and the per-proof fallback --------------------------------------------------------------------------------------
def test_group_split_and_fallback(gpu_ctx, oracle):
    curve = "bls12_381"
    s = _key(gpu_ctx, oracle, curve, "mimc16", 7)
    whole, st = _batch(s, gpu_ctx, curve, "merlin", range(7))
    assert st == [0] * 7 and whole == [_single(s, gpu_ctx, curve, "merlin", i) for i in range(7)]
    n = s["pk"].n
    assert 3 * (10 * n + 22) <= 1 << 12 < 4 * (10 * n + 22) and 10 * n + 22 > 1 << 10
    gpu_ctx.set_option("msm_max_piece_log", 12)          # groups of 3 + 3 + 1
    split, st = _batch(s, gpu_ctx, curve, "merlin", range(7))
    assert st == [0] * 7 and split == whole
    gpu_ctx.set_option("msm_max_piece_log", 10)          # one proof's [d]_1 row exceeds a piece: the per-proof path, its MSMs in pieces
    loop, st = _batch(s, gpu_ctx, curve, "merlin", range(7))
    assert st == [0] * 7 and loop == whole
    t = gpu_ctx.timings()
    assert t["msm_total"] > 0 and t["ntt"] > 0 and t["phase"] > 0


# ---- 5. device-resident assignment -------------------------------------------------------------------------------------------------
def test_device_resident_assignment(gpu_ctx, oracle):
    hip = ct.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [ct.POINTER(ct.c_void_p), ct.c_size_t]
    hip.hipMemcpy.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_size_t, ct.c_int]
    hip.hipFree.argtypes = [ct.c_void_p]
    curve = "bn254"
    s = _key(gpu_ctx, oracle, curve, "mimc322", 4)
    host, st = _batch(s, gpu_ctx, curve, "merlin", range(4))
    assert st == [0] * 4
    bufs = []
    for key in ("xl", "wl"):
        arr = np.ascontiguousarray(np.stack([s["rows"][i][key] for i in range(4)]))
        p = ct.c_void_p()
        assert hip.hipMalloc(ct.byref(p), arr.nbytes) == 0
        assert hip.hipMemcpy(p, arr.ctypes.data_as(ct.c_void_p), arr.nbytes, 1) == 0
        bufs.append(p)
    dev, st = _batch(s, gpu_ctx, curve, "merlin", range(4), device_ptrs=(bufs[0].value, bufs[1].value))
    for p in bufs:
        hip.hipFree(p)
    assert st == [0] * 4 and dev == host


# ---- 6. tables on and off -----------------------------------------------------------------------------------------------------------
def test_tables_on_and_off(gpu_ctx, oracle):
    curve = "bls12_381"
    a = _key(gpu_ctx, oracle, curve, "mimc322", 3, tables="auto")
    b = _key(gpu_ctx, oracle, curve, "mimc322", 3, tables="off")
    assert [r["r_a"] for r in a["rows"][:3]] == [r["r_a"] for r in b["rows"][:3]]       # the same seeded rows
    pa, sa = _batch(a, gpu_ctx, curve, "merlin", range(3))
    pb, sb = _batch(b, gpu_ctx, curve, "merlin", range(3))
    assert sa == sb == [0] * 3 and pa == pb


# ---- 7. round trip with the batch verifier ------------------------------------------------------------------------------------------
def test_round_trip_with_verify_batch(gpu_ctx, oracle):
    curve = "bls12_381"
    s = _key(gpu_ctx, oracle, curve, "mimc16", 8)
    pm = _pm(s, gpu_ctx, curve, "merlin")
    vk = pm.make_vk(s["pk"], s["x"], s["z"])
    proofs, st = _batch(s, gpu_ctx, curve, "merlin", range(8))
    assert st == [0] * 8
    v, ok, checks = pm.verify_batch(vk, [s["rows"][i]["inst"][1:] for i in range(8)], proofs)
    assert ok is True and v.tolist() == [1] * 8
    rows = [dict(r) for r in s["rows"][:8]]
    wit = list(rows[5]["wit"])
    wit[0] = (wit[0] + 1) % pm.field.r
    rows[5]["wl"] = pm.field.fr_limbs(wit)
    proofs, st = pm.prove_batch(s["pk"], [(r["xl"], r["wl"]) for r in rows], [r["r_a"] for r in rows])
    assert st[5] != 0 and proofs[5] is None
    keep = [i for i in range(8) if st[i] == 0]
    assert keep == [0, 1, 2, 3, 4, 6, 7]
    v, ok, checks = pm.verify_batch(vk, [rows[i]["inst"][1:] for i in keep], [proofs[i] for i in keep])
    assert ok is True and v.tolist() == [1] * 7


# ---- 8. hygiene -----------------------------------------------------------------------------------------------------------------------
def test_hygiene_and_flat_memory(gpu_ctx, oracle):
    from polymath_amd import polymath as PM
    curve = "bls12_381"
    s = _key(gpu_ctx, oracle, curve, "mimc16", 6)
    pm, pk = _pm(s, gpu_ctx, curve, "merlin"), s["pk"]
    rows = s["rows"][:6]
    xs, ws = np.stack([r["xl"] for r in rows]), np.stack([r["wl"] for r in rows])
    ra = np.stack([pm.field.fr_limbs(r["r_a"]) for r in rows])
    # count == 0
    proofs, st = pm.prove_batch(pk, [], [])
    assert proofs == [] and st == []
    # a sharded key, a wrong proof_len, an unknown transcript: PM_ERR_INVALID_ARG, status[] untouched
    q, row0 = s["q"], rows[0]
    half = pm.setup((PM.R1CS(q.m0, q.mw, q.a, q.b, q.c), row0["inst"], row0["wit"]), s["x"], s["z"], 0, 2)
    assert half.host_prove_batch("merlin", xs, xs, ws, ra)[0] == PM_ERR_INVALID_ARG
    half.free()
    L, buf, status = gpu_ctx.L, ct.create_string_buffer(6 * 176), (ct.c_int * 6)(*([-1] * 6))
    from polymath_amd import api
    args = lambda t, plen: (gpu_ctx.h, pk.h, t, 6, api._p(xs), xs.ctypes.data_as(ct.c_void_p), ws.ctypes.data_as(ct.c_void_p), 0, api._p(ra), buf, plen, status)
    assert L.pm_host_prove_batch(*args(0, 175)) == PM_ERR_INVALID_ARG
    assert L.pm_host_prove_batch(*args(7, 176)) == PM_ERR_INVALID_ARG
    assert list(status) == [-1] * 6 and buf.raw == bytes(6 * 176)
    # the context after a batch: the single prover's bytes, and summed stage times
    before = pm.prove_native(pk, rows[1]["xl"], rows[1]["wl"], rows[1]["r_a"])
    proofs, st = _batch(s, gpu_ctx, curve, "merlin", range(6))
    t = gpu_ctx.timings()
    assert st == [0] * 6 and proofs[1] == before
    assert t["msm_total"] > 0 and t["ntt"] > 0 and t["phase"] > 0 and t["poly"] > 0 and t["witness_map"] > 0, t
    assert pm.prove_native(pk, rows[1]["xl"], rows[1]["wl"], rows[1]["r_a"]) == before
    # a proof in flight between the phases is not disturbed by a batch on the same context
    f = pm.field
    rc = pk.phase1(rows[2]["xl"], rows[2]["wl"], f.fr_limbs(rows[2]["r_a"]))[0]
    one = f.fr_limbs([12345])[0]
    u_before = pk.phase2(one)[1].copy()
    _batch(s, gpu_ctx, curve, "merlin", range(6))
    assert rc == 0 and np.array_equal(pk.phase2(one)[1], u_before)
    # free device memory over 20 batches of one shape is flat (the soak test's method and tolerance)
    hip = ct.CDLL("libamdhip64.so")

    def free_hbm():
        fr, tot = ct.c_size_t(), ct.c_size_t()
        assert hip.hipMemGetInfo(ct.byref(fr), ct.byref(tot)) == 0
        return fr.value

    free0 = free_hbm()
    for _ in range(20):
        assert _batch(s, gpu_ctx, curve, "merlin", range(6))[1] == [0] * 6
    free1 = free_hbm()
    print("free device memory before / after 20 batches:", free0, free1)
    assert abs(free0 - free1) <= 8 << 20, (free0, free1)
