"""GPU: pm_host_prove_batch with PM_PROVE_GLUE_DEVICE (Polymath.prove_batch(glue="device")) -- the Fiat-Shamir glue between the phases
of a group of proofs in kernels with one lane per proof (csrc/prove_glue.hip), one copy to the host and one synchronisation per group.
The bar is equality of bytes and statuses with host mode of the same call; where stated also with the single prover (prove_native),
the CPU oracle and the committed fixtures.  Shapes are test_gpu_prove_batch.py's smallest (its keys and seeded rows are shared);
counts walk the lane, wave and workgroup edges of the one-lane-per-proof kernels (1, 63, 64, 65, 257), m0 walks FS_INV_CHUNK
(2 m0 = 14, 16, 18)."""
import ctypes as ct

import numpy as np
import pytest

import test_gpu_prove_batch as PB
import test_gpu_witness_solve as WS
from helpers import I, load_golden, r1cs_from_json
from oracle.pyref import circuits as CI
from oracle.pyref.fields import CURVES

pytestmark = pytest.mark.gpu

PM_OK, PM_ERR_INVALID_ARG, PM_ERR_REMAINDER_NONZERO = 0, 1, 4
PROOF_LEN = PB.PROOF_LEN


def _both(s, gpu_ctx, curve, transcript, idx, **kw):
    """the same batch in device mode and in host mode -> (device proofs, device statuses); the two are asserted equal"""
    dev = PB._batch(s, gpu_ctx, curve, transcript, idx, glue="device", **kw)
    host = PB._batch(s, gpu_ctx, curve, transcript, idx, **kw)
    assert dev[1] == host[1], (transcript, dev[1], host[1])
    assert dev[0] == host[0], (transcript, [i for i, (a, b) in enumerate(zip(dev[0], host[0])) if a != b])
    return dev


def _raw(s, pm, rows, inst=None, glue="device", **kw):
    xs, ws = np.stack([r["xl"] for r in rows]), np.stack([r["wl"] for r in rows])
    ra = np.stack([pm.field.fr_limbs(r["r_a"]) for r in rows])
    return s["pk"].host_prove_batch(pm.transcript_name, xs if inst is None else inst, xs, ws, ra, glue=glue, **kw)


# ---- 1. bytes equal host mode, the single prover and the oracle ---------------------------------------------------------------------
@pytest.mark.parametrize("curve,shape_name,counts,transcripts", [
    ("bls12_381", "mimc16", (1, 2, 5, 33), ("merlin", "keccak256", "blake3")),
    ("bn254", "mimc16", (1, 2, 5, 33), ("merlin",)),
    ("bls12_381", "mimc322", (3,), ("merlin",)),
    ("bls12_381", "bench2p10", (5,), ("merlin",)),
])
def test_bytes_equal_host_mode_single_prover_and_oracle(gpu_ctx, oracle, curve, shape_name, counts, transcripts):
    s = PB._key(gpu_ctx, oracle, curve, shape_name, max(counts))
    for transcript in transcripts:
        for count in counts:
            proofs, status = _both(s, gpu_ctx, curve, transcript, range(count))
            assert status == [PM_OK] * count, (transcript, count, status)
            for i in range(min(count, 5)):        # rows 0 .. 4 against the two other provers (their bytes are computed once per row)
                assert len(proofs[i]) == PROOF_LEN[curve]
                assert proofs[i] == PB._single(s, gpu_ctx, curve, transcript, i), (transcript, count, i, "single prover")
                assert proofs[i] == PB._oracle_bytes(s, oracle, curve, transcript, i), (transcript, count, i, "oracle")


# ---- 2. golden fixtures ---------------------------------------------------------------------------------------------------------------
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
            proofs, status = pm.prove_batch(pk, [(xl, wl)] * 3, [r_a] * 3, glue="device")
            assert status == [0, 0, 0] and [p.hex() for p in proofs] == [ref["bytes"]] * 3, (fx["name"], tname, status)
        pk.free()
        seen.add(q.m0)
    assert seen >= ({1, 2, 3, 12} if name == "proofs.json" else {2})


# ---- 3. lane, wave and workgroup edges ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [63, 64, 65, 257])
def test_lane_wave_and_workgroup_edges(gpu_ctx, oracle, count):
    curve = "bls12_381"
    s = PB._key(gpu_ctx, oracle, curve, "mimc16", count)
    proofs, status = _both(s, gpu_ctx, curve, "merlin", range(count))
    assert status == [PM_OK] * count
    assert proofs[count - 1] == PB._single(s, gpu_ctx, curve, "merlin", count - 1)      # the last lane's proof is a proof


# ---- 4. m0 = 7, 8, 9: 2 m0 around FS_INV_CHUNK -----------------------------------------------------------------------------------------
def _wide_instance(c, m0, g):
    """three gates over four witnesses and m0 instance columns: w0 w1 = w2, w2 w2 = w3, (w3 + x_1 + ... + x_{m0-2}) 1 = x_{m0-1}"""
    w0, w1 = g.fr(c.r), g.fr(c.r)
    w2 = w0 * w1 % c.r
    w3 = w2 * w2 % c.r
    xs = [g.fr(c.r) for _ in range(m0 - 2)]
    inst = [1] + xs + [(w3 + sum(xs)) % c.r]
    W = m0
    q = CI.R1CS(m0, 4, [[(1, W)], [(1, W + 2)], [(1, W + 3)] + [(1, j) for j in range(1, m0 - 1)]],
                [[(1, W + 1)], [(1, W + 2)], [(1, 0)]],
                [[(1, W + 2)], [(1, W + 3)], [(1, m0 - 1)]])
    return q, inst, [w0, w1, w2, w3]


@pytest.mark.parametrize("curve", ["bls12_381", "bn254"])
@pytest.mark.parametrize("m0", [7, 8, 9])
def test_instance_widths_around_the_inversion_chunk(gpu_ctx, oracle, curve, m0):
    from polymath_amd import polymath as PM
    c = CURVES[curve]
    g = CI.SplitMix64(9100 + m0)
    pm = PM.Polymath(curve, "keccak256", ctx=gpu_ctx)
    f = pm.field
    x, z = g.fr(c.r), g.fr(c.r)
    rows, q = [], None
    for _ in range(3):
        q, inst, wit = _wide_instance(c, m0, g)
        rows.append(dict(inst=inst, wit=wit, r_a=[g.fr(c.r), g.fr(c.r)], xl=f.fr_limbs(inst), wl=f.fr_limbs(wit)))
    pk = pm.setup((PM.R1CS(q.m0, q.mw, q.a, q.b, q.c), rows[0]["inst"], rows[0]["wit"]), x, z)
    assert pk.m0 == m0
    s = dict(pk=pk, q=q, x=x, z=z, rows=rows, pm={"keccak256": pm}, opk=None, single={}, oracle={})
    proofs, status = _both(s, gpu_ctx, curve, "keccak256", range(3))
    assert status == [PM_OK] * 3
    for i in range(3):
        assert proofs[i] == PB._oracle_bytes(s, oracle, curve, "keccak256", i), (m0, i)
    pk.free()


# ---- 5. a refused row -----------------------------------------------------------------------------------------------------------------
def test_unsatisfied_row_in_a_batch(gpu_ctx, oracle):
    curve = "bls12_381"
    s = PB._key(gpu_ctx, oracle, curve, "mimc16", 8)
    pm = PB._pm(s, gpu_ctx, curve, "merlin")
    rows = [dict(r) for r in s["rows"][:8]]
    wit = list(rows[5]["wit"])
    wit[3] = (wit[3] + 1) % pm.field.r
    rows[5]["wl"] = pm.field.fr_limbs(wit)
    rc_h, data_h, st_h = _raw(s, pm, rows, glue="host")
    rc_d, data_d, st_d = _raw(s, pm, rows)
    assert rc_h == rc_d == PM_OK
    assert st_d.tolist() == st_h.tolist() == [0] * 5 + [PM_ERR_REMAINDER_NONZERO] + [0] * 2
    assert data_d == data_h and data_d[5 * 176:6 * 176] == bytes(176)
    for i in (0, 4, 6, 7):
        assert data_d[i * 176:(i + 1) * 176] == PB._single(s, gpu_ctx, curve, "merlin", i), i
    tap = s["pk"].glue_challenges(8)
    assert not tap[5].any() and all(tap[i].any(axis=1).all() for i in range(8) if i != 5)


# ---- 6. several groups and the per-proof fallback ---------------------------------------------------------------------------------------
def test_group_split_and_fallback(gpu_ctx, oracle):
    curve = "bls12_381"
    s = PB._key(gpu_ctx, oracle, curve, "mimc16", 5)
    whole, st = _both(s, gpu_ctx, curve, "merlin", range(5))
    assert st == [0] * 5
    n = s["pk"].n
    assert 3 * (10 * n + 22) <= 1 << 12 < 4 * (10 * n + 22) and 10 * n + 22 > 1 << 10
    gpu_ctx.set_option("msm_max_piece_log", 12)          # groups of 3 + 2
    split, st = PB._batch(s, gpu_ctx, curve, "merlin", range(5), glue="device")
    assert st == [0] * 5 and split == whole
    tap = s["pk"].glue_challenges(5)                     # the tap covers all groups of the call
    assert all(tap[i].any(axis=1).all() for i in range(5))
    gpu_ctx.set_option("msm_max_piece_log", 10)          # one proof's [d]_1 row exceeds a piece: the per-proof loop, host glue
    loop, st = PB._batch(s, gpu_ctx, curve, "merlin", range(5), glue="device")
    assert st == [0] * 5 and loop == whole
    with pytest.raises(Exception):
        s["pk"].glue_challenges(5)                       # ... which leaves no tap 11


# ---- 7. PM_ASSIGNMENT_SOLVE ---------------------------------------------------------------------------------------------------------------
def test_solve_with_device_glue(gpu_ctx):
    curve = "bls12_381"
    s = WS._mimc_key(gpu_ctx, curve)
    pm, pk, c = s["pm"], s["pk"], s["c"]
    rows = WS._mimc_rows(c, 3, 9200)
    limbs = [pm.partial_limbs(*p) for _, _, p in rows]           # the public output is a marker in instance_host
    r_as = [[61 + i, 71 + i] for i in range(3)]
    dev = pm.prove_batch(pk, limbs, r_as, solve=True, glue="device")
    host = pm.prove_batch(pk, limbs, r_as, solve=True)
    assert dev[1] == host[1] == [0] * 3 and dev[0] == host[0] and dev[2] == host[2]
    assert dev[2] == [list(inst) for inst, _, _ in rows]
    one = pm.prove_batch(pk, limbs[:1], r_as[:1], solve=True, glue="device")      # count == 1 is the group path with one row
    assert one[1] == [0] and one[0] == host[0][:1]
    # one stuck row in a batch of four
    k = WS._kinds_key(gpu_ctx, curve)
    pm, pk, c = k["pm"], k["pk"], k["c"]
    vals = [(21, 22), (0, 5), (23, 24), (25, 26)]
    limbs = [pm.partial_limbs(*WS.kinds_partial(a, cc, a * a % c.r)) for a, cc in vals]
    r_as = [[31 + i, 41 + i] for i in range(4)]
    dev = pm.prove_batch(pk, limbs, r_as, solve=True, glue="device")
    host = pm.prove_batch(pk, limbs, r_as, solve=True)
    assert dev[1] == host[1] == [0, PM_ERR_INVALID_ARG, 0, 0]
    assert dev[0] == host[0] and dev[0][1] is None and dev[2] == host[2]
    xs, ws = np.stack([l[0] for l in limbs]), np.stack([l[1] for l in limbs])
    ra = np.stack([pm.field.fr_limbs(r) for r in r_as])
    rc, data, st = pk.host_prove_batch("merlin", xs, xs, ws, ra, solve=True, glue="device")
    assert rc == PM_OK and data[176:352] == bytes(176) and not pk.glue_challenges(4)[1].any()


# ---- 8. device pointers -----------------------------------------------------------------------------------------------------------------
def test_device_resident_assignment(gpu_ctx, oracle):
    hip = ct.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [ct.POINTER(ct.c_void_p), ct.c_size_t]
    hip.hipMemcpy.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_size_t, ct.c_int]
    hip.hipFree.argtypes = [ct.c_void_p]
    curve = "bn254"
    s = PB._key(gpu_ctx, oracle, curve, "mimc16", 4)
    host, st = PB._batch(s, gpu_ctx, curve, "merlin", range(4))
    assert st == [0] * 4
    bufs = []
    for key in ("xl", "wl"):
        arr = np.ascontiguousarray(np.stack([s["rows"][i][key] for i in range(4)]))
        p = ct.c_void_p()
        assert hip.hipMalloc(ct.byref(p), arr.nbytes) == 0
        assert hip.hipMemcpy(p, arr.ctypes.data_as(ct.c_void_p), arr.nbytes, 1) == 0
        bufs.append(p)
    dev, st = PB._batch(s, gpu_ctx, curve, "merlin", range(4), device_ptrs=(bufs[0].value, bufs[1].value), glue="device")
    for p in bufs:
        hip.hipFree(p)
    assert st == [0] * 4 and dev == host


# ---- 9. the hashed inputs are instance_host's ---------------------------------------------------------------------------------------------
def test_instance_host_differs_from_the_x_rows(gpu_ctx, oracle):
    curve = "bls12_381"
    s = PB._key(gpu_ctx, oracle, curve, "mimc16", 4)
    pm = PB._pm(s, gpu_ctx, curve, "blake3")
    rows = s["rows"][:4]
    # element 0 is hashed and enters nothing else (pi(x1) takes 2 for it): proofs of other bytes, equal in both modes
    other = np.stack([r["xl"] for r in rows]).copy()
    for i in range(4):
        other[i, 0] = pm.field.fr_limbs([12345 + i])[0]                  # not even a leading one
    rc_d, data_d, st_d = _raw(s, pm, rows, inst=other)
    rc_h, data_h, st_h = _raw(s, pm, rows, inst=other, glue="host")
    assert rc_d == rc_h == PM_OK and st_d.tolist() == st_h.tolist() == [0] * 4 and data_d == data_h
    same = _raw(s, pm, rows)[1]
    assert all(data_d[i * 176:(i + 1) * 176] != same[i * 176:(i + 1) * 176] for i in range(4))      # the instance is hashed
    # the neighbour's public inputs: pi(x1) is theirs, the quotient's remainder is not zero -- refused alike, not proved from the x rows
    other = np.stack([rows[(i + 1) % 4]["xl"] for i in range(4)]).copy()
    rc_d, data_d, st_d = _raw(s, pm, rows, inst=other)
    rc_h, data_h, st_h = _raw(s, pm, rows, inst=other, glue="host")
    assert rc_d == rc_h == PM_OK and st_d.tolist() == st_h.tolist() == [PM_ERR_REMAINDER_NONZERO] * 4 and data_d == data_h == bytes(4 * 176)


# ---- 10. tap 11 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve,transcript", [("bls12_381", "merlin"), ("bls12_381", "keccak256"), ("bn254", "blake3")])
def test_tap_11(gpu_ctx, oracle, curve, transcript):
    from polymath_amd import api
    s = PB._key(gpu_ctx, oracle, curve, "mimc16", 5)
    pm = PB._pm(s, gpu_ctx, curve, transcript)
    f = pm.field
    proofs, st = PB._batch(s, gpu_ctx, curve, transcript, range(5), glue="device")
    assert st == [0] * 5
    tap = s["pk"].glue_challenges(5).copy()
    vk = pm.make_vk(s["pk"], s["x"], s["z"])
    pub = np.stack([f.fr_limbs(s["rows"][i]["inst"][1:]) for i in range(5)])
    x1, x2, c_at, ok = api.verifier_challenges_batch(gpu_ctx, curve, transcript, vk, pub, proofs)
    assert ok.tolist() == [1] * 5
    assert np.array_equal(tap[:, 0], x1) and np.array_equal(tap[:, 1], x2) and np.array_equal(tap[:, 3], c_at)
    nb = (PROOF_LEN[curve] - 32) // 3
    for i in range(5):
        assert f.fr_int(tap[i, 2]) == int.from_bytes(proofs[i][2 * nb:2 * nb + 32], "little"), i


# ---- 11. hygiene --------------------------------------------------------------------------------------------------------------------------
def test_hygiene_and_flat_memory(gpu_ctx, oracle):
    from polymath_amd import api
    curve = "bls12_381"
    s = PB._key(gpu_ctx, oracle, curve, "mimc16", 6)
    pm, pk = PB._pm(s, gpu_ctx, curve, "merlin"), s["pk"]
    rows = s["rows"][:6]
    f = pm.field
    xs, ws = np.stack([r["xl"] for r in rows]), np.stack([r["wl"] for r in rows])
    ra = np.stack([f.fr_limbs(r["r_a"]) for r in rows])
    # bits outside 255 | 256, or no pm_transcript below them: PM_ERR_INVALID_ARG, outputs untouched; the single prover refuses the flag
    L, buf, status = gpu_ctx.L, ct.create_string_buffer(6 * 176), (ct.c_int * 6)(*([-1] * 6))
    args = lambda t: (gpu_ctx.h, pk.h, t, 6, api._p(xs), xs.ctypes.data_as(ct.c_void_p), ws.ctypes.data_as(ct.c_void_p), 0, api._p(ra), buf, 176, status)
    for t in (256 | 3, 256 | 7, 512, 256 | 1024):
        assert L.pm_host_prove_batch(*args(t)) == PM_ERR_INVALID_ARG, t
    assert list(status) == [-1] * 6 and buf.raw == bytes(6 * 176)
    n = ct.c_size_t(0)
    assert L.pm_host_prove(gpu_ctx.h, pk.h, 256, api._p(xs[0]), xs[0].ctypes.data_as(ct.c_void_p), ws[0].ctypes.data_as(ct.c_void_p), 0, api._p(ra[0]),
                           buf, 176, ct.byref(n)) == PM_ERR_INVALID_ARG
    # the context after a device-glue batch: host mode and the single prover give the old bytes; summed stage times
    before = pm.prove_native(pk, rows[1]["xl"], rows[1]["wl"], rows[1]["r_a"])
    host_before = PB._batch(s, gpu_ctx, curve, "merlin", range(6))
    proofs, st = PB._batch(s, gpu_ctx, curve, "merlin", range(6), glue="device")
    t = gpu_ctx.timings()
    assert st == [0] * 6 and proofs[1] == before
    assert t["msm_total"] > 0 and t["ntt"] > 0 and t["phase"] > 0 and t["poly"] > 0, t
    assert PB._batch(s, gpu_ctx, curve, "merlin", range(6)) == host_before
    assert pk.glue_challenges(6).any()                   # a host-mode call leaves the last device-glue call's tap alone
    assert pm.prove_native(pk, rows[1]["xl"], rows[1]["wl"], rows[1]["r_a"]) == before
    # a proof in flight between the phases is not disturbed by a device-glue batch on the same context
    rc = pk.phase1(rows[2]["xl"], rows[2]["wl"], f.fr_limbs(rows[2]["r_a"]))[0]
    one = f.fr_limbs([12345])[0]
    u_before = pk.phase2(one)[1].copy()
    PB._batch(s, gpu_ctx, curve, "merlin", range(6), glue="device")
    assert rc == 0 and np.array_equal(pk.phase2(one)[1], u_before)
    # free device memory over 20 batches of one shape is flat (the soak test's method and tolerance)
    hip = ct.CDLL("libamdhip64.so")

    def free_hbm():
        fr, tot = ct.c_size_t(), ct.c_size_t()
        assert hip.hipMemGetInfo(ct.byref(fr), ct.byref(tot)) == 0
        return fr.value

    free0 = free_hbm()
    for _ in range(20):
        assert PB._batch(s, gpu_ctx, curve, "merlin", range(6), glue="device")[1] == [0] * 6
    free1 = free_hbm()
    print("free device memory before / after 20 batches:", free0, free1)
    assert abs(free0 - free1) <= 8 << 20, (free0, free1)
