"""Proving keys as bytes, decoded on the device: pm_g1_decode, pm_pk_load_bytes, pm_pk_export_bases_compressed.

The specification is the host mirror's deser_g1 / ser_g1 (polymath_amd/host/wire.hpp): ark-serialize's compressed G1, zcash
flags on BLS12-381, short-Weierstrass flags on BN254, Validate::Yes = on the curve and in the prime-order subgroup.  Expected
verdicts here come from big-integer decoding (oracle.pyref) with [r]P for subgroup membership.
"""
import os
import re
import struct

import numpy as np
import pytest

from helpers import I, load_golden, r1cs_from_json
from oracle.pyref.fields import CURVES, _jac_add_affine, _jac_dbl, g1_add, g1_neg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pm_g1_decode", "pm_pk_load_bytes", "pm_pk_export_bases_compressed")
OK, BAD_FLAGS, GE_P, NOT_ON_CURVE, NOT_IN_G1, NONCANON_INF, INF_SIGN = range(7)
REASONS = {BAD_FLAGS: "G1: not a compressed point", GE_P: "G1: coordinate >= p", NOT_ON_CURVE: "G1: not on the curve",
           NOT_IN_G1: "G1: not in the prime-order subgroup", NONCANON_INF: "G1: non-canonical encoding of the point at infinity",
           INF_SIGN: "G1: sign bit on the point at infinity"}
NB = {"bls12_381": 48, "bn254": 32}
VK_LEN = {"bls12_381": 392, "bn254": 280}
WIRE_ORDER = (0, 1, 4, 2, 3, 5)
NAMES = {0: "x_powers_g1", 1: "x_powers_y_alpha_g1", 2: "x_powers_y_gamma_g1", 3: "x_powers_y_gamma_z_g1", 4: "x_powers_zh_by_y_alpha_g1",
         5: "uj_wj_lcs_by_y_alpha_g1"}


# ------------------------------------------------------------------------------------------------------------- big-int codec
def times(c, P, k):
    """[k] P without reducing k mod r (pyref's g1_mul does: [r] P would always come out as O)"""
    if P is None:
        return None
    X, Y, Z = 1, 1, 0
    for bit in bin(k)[2:]:
        X, Y, Z = _jac_dbl(c.p, X, Y, Z)
        if bit == "1":
            X, Y, Z = _jac_add_affine(c.p, X, Y, Z, P[0], P[1])
    if Z == 0:
        return None
    zi = pow(Z, -1, c.p)
    return (X * zi * zi % c.p, Y * zi * zi * zi % c.p)


def _sqrt(c, a):
    y = pow(a, (c.p + 1) // 4, c.p)
    return y if y * y % c.p == a % c.p else None


def ref_encode(c, P):
    if c.name == "bls12_381":
        if P is None:
            return bytes([0xC0]) + bytes(47)
        b = bytearray(P[0].to_bytes(48, "big"))
        b[0] |= 0x80 | (0x20 if P[1] > c.p - P[1] else 0)
        return bytes(b)
    if P is None:
        return bytes(31) + b"\x40"
    b = bytearray(P[0].to_bytes(32, "little"))
    b[31] |= 0x80 if P[1] > (c.p - P[1]) % c.p else 0
    return bytes(b)


def ref_decode(c, rec, validate):
    """deser_g1 of wire.hpp restated on integers -> (status, point or None)"""
    if c.name == "bls12_381":
        f = rec[0]
        if not f & 0x80:
            return BAD_FLAGS, None
        inf, larger = bool(f & 0x40), bool(f & 0x20)
        x = int.from_bytes(bytes([f & 0x1F]) + rec[1:], "big")
        if inf:
            return (INF_SIGN, None) if larger else ((NONCANON_INF, None) if x else (OK, None))
    else:
        f = rec[31]
        inf, larger = bool(f & 0x40), bool(f & 0x80)
        if inf and larger:
            return BAD_FLAGS, None
        x = int.from_bytes(rec[:31] + bytes([f & 0x3F]), "little")
        if inf:
            return (NONCANON_INF, None) if x else (OK, None)
    if x >= c.p:
        return GE_P, None
    y = _sqrt(c, (x * x * x + c.b) % c.p)
    if y is None:
        return NOT_ON_CURVE, None
    if (y > (c.p - y) % c.p) != larger:
        y = (c.p - y) % c.p
    if validate and c.name == "bls12_381" and times(c, (x, y), c.r) is not None:
        return NOT_IN_G1, None
    return OK, (x, y)


def _random_curve_point(c, rng):
    while True:
        x = int(rng.integers(0, 2 ** 62)) * (1 << 300) % c.p + int(rng.integers(1, 2 ** 62))
        y = _sqrt(c, (x ** 3 + c.b) % c.p)
        if y is not None:
            return (x, y)


def _crafted(c, rng, valid_recs):
    """>= 512 hand-made encodings of every class, with the points the BLS12-381 subgroup cases were made from"""
    out = []
    nb = NB[c.name]
    bls = c.name == "bls12_381"
    for k in range(48):
        rec = bytearray(valid_recs[k])
        if bls:
            rec[0] &= 0x7F                                             # compression bit clear
        else:
            rec[31] |= 0xC0                                            # both flags
        out.append(bytes(rec))
        inf = bytearray(ref_encode(c, None))
        inf[1 + k % (nb - 2)] ^= 1 << (k % 8)                          # infinity with a stray bit in x
        out.append(bytes(inf))
    if bls:
        out.append(bytes([0xE0]) + bytes(47))                          # sign bit on infinity
        out.append(bytes([0xC1]) + bytes(47))                          # stray bit in the flag byte's x part
    else:
        out.append(bytes(31) + b"\x41")
    top = (1 << (8 * nb - 3)) if bls else (1 << (8 * nb - 2))
    for x in [c.p, c.p + 1, top - 1] + [c.p + int(rng.integers(0, 2 ** 62)) * 977 % (top - c.p) for _ in range(45)]:
        if x >= top:
            continue
        if bls:
            b = bytearray(x.to_bytes(48, "big"))
            b[0] |= 0x80 | (0x20 if x & 1 else 0)
        else:
            b = bytearray(x.to_bytes(32, "little"))
            b[31] |= 0x80 if x & 1 else 0
        out.append(bytes(b))
    nsq = 0
    while nsq < 100:                                                   # x^3 + b a non-residue
        x = int(rng.integers(1, 2 ** 62)) ** 5 % c.p
        if _sqrt(c, (x ** 3 + c.b) % c.p) is None:
            out.append(ref_encode(c, (x, 0))[:])
            nsq += 1
    for _ in range(300):                                               # random byte strings
        out.append(bytes(rng.integers(0, 256, nb, dtype=np.uint8)))
    if bls:
        for _ in range(64):                                            # on the curve, not in G1
            out.append(ref_encode(c, _random_curve_point(c, rng)))
        for _ in range(8):                                             # torsion T = [r]Q != O and G + T
            T = times(c, _random_curve_point(c, rng), c.r)
            assert T is not None and times(c, T, c.r) is not None
            out.append(ref_encode(c, T))
            out.append(ref_encode(c, g1_add(c, c.g1, T)))
            out.append(ref_encode(c, g1_neg(c, T)))
    return out


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_header_python_and_sys_crate_declare_the_byte_key_entry_points():
    from polymath_amd import api
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "polymath_hip.h")).read(), flags=re.S)
    sys_rs = open(os.path.join(ROOT, "rust", "polymath-hip-sys", "src", "lib.rs")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, header) and s in api.EXPORTS and ("pub fn %s(" % s) in sys_rs, s
    assert re.search(r"PM_OPT_WIRE_CHUNK_LOG\s*=\s*8", header) and re.search(r"PM_NUM_OPTIONS\s*=\s*9", header)
    assert api.OPTIONS["wire_chunk_log"] == 8
    assert "pub const PM_OPT_WIRE_CHUNK_LOG: i32 = 8;" in sys_rs and "pub const PM_NUM_OPTIONS: i32 = 9;" in sys_rs
    for k, name in enumerate(("OK", "BAD_FLAGS", "COORD_GE_P", "NOT_ON_CURVE", "NOT_IN_SUBGROUP", "NONCANONICAL_INF", "INF_SIGN")):
        assert re.search(r"PM_G1_%s\s*=\s*%d\b" % (name, k), header), name
    wrapper = open(os.path.join(ROOT, "rust", "polymath-hip", "src", "lib.rs")).read()
    assert "pub fn load_bytes<E: Pairing>" in wrapper and "sys::pm_pk_load_bytes(" in wrapper


def test_null_context_is_invalid_arg():
    import ctypes as ct
    from polymath_amd import api
    L = api.load_library()
    buf = ct.create_string_buffer(64)
    out = ct.c_void_p()
    xy = np.zeros(16, dtype=np.uint64)
    assert L.pm_g1_decode(None, 0, buf, 1, 1, api._p(xy), buf) == 1
    assert L.pm_pk_load_bytes(None, 0, buf, 64, 1, 0, 1, 0, ct.byref(out)) == 1 and not out.value
    assert L.pm_pk_export_bases_compressed(None, None, 0, 0, 1, buf) == 1


def test_reference_codec_agrees_with_the_python_twin_on_fixture_points():
    """The test's own big-int codec (the expectation of the GPU tests) re-encodes the fixture keys' points byte for byte."""
    c = CURVES["bls12_381"]
    for key in load_golden("pk_wire.json")["keys"][:2]:
        data = bytes.fromhex(key["pk_bytes"])
        for which, (off, cnt) in _vec_offsets(data, "bls12_381").items():
            for i in range(cnt):
                rec = data[off + 48 * i: off + 48 * (i + 1)]
                st, P = ref_decode(c, rec, True)
                assert st == OK and ref_encode(c, P) == rec, (which, i)


def _vec_offsets(data, curve):
    """{pm_base_vec: (byte offset of point 0, count)} of a serialize_compressed key"""
    nb = NB[curve]
    o = VK_LEN[curve] + 24
    for _ in range(3):
        rows = struct.unpack_from("<Q", data, o)[0]
        o += 8
        for _ in range(rows):
            cnt = struct.unpack_from("<Q", data, o)[0]
            o += 8 + 40 * cnt
    out = {}
    for which in WIRE_ORDER:
        cnt = struct.unpack_from("<Q", data, o)[0]
        out[which] = (o + 8, cnt)
        o += 8 + nb * cnt
    assert o == len(data)
    return out


# ------------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("curve", ["bls12_381", "bn254"])
def test_decode_agrees_per_point(gpu_ctx, curve):
    from polymath_amd import api
    from polymath_amd.polymath import Field
    c, f = CURVES[curve], Field(curve)
    rng = np.random.default_rng(0xDEC0DE + len(curve))
    mult = api.Bases.multiples(gpu_ctx, curve, 2048)
    pts = [f.g1_affine(row, False) for row in mult.download()]
    mult.free()
    valid = [ref_encode(c, P) for P in pts] + [ref_encode(c, g1_neg(c, P)) for P in pts] + [ref_encode(c, None)]
    recs = valid + _crafted(c, rng, valid)
    assert len(valid) >= 4096 and len(recs) - len(valid) >= 512
    gpu_ctx.set_option("wire_chunk_log", 10)                           # several chunks
    for validate in (True, False):
        xy, st = api.g1_decode(gpu_ctx, curve, b"".join(recs), validate)
        for i, rec in enumerate(recs):
            if i < len(valid):                                         # generator multiples: in G1 by construction
                exp = (OK, pts[i] if i < 2048 else (g1_neg(c, pts[i - 2048]) if i < 4096 else None))
            else:
                exp = ref_decode(c, rec, validate)
            got = None if not xy[i].any() else f.g1_affine(xy[i], False)
            assert (int(st[i]), got) == exp, (curve, validate, i, rec.hex())
        if validate and curve == "bls12_381":
            assert (st == NOT_IN_G1).sum() >= 64
    # validate = 0: exactly the subgroup verdicts change, to the on-curve point
    xy1, st1 = api.g1_decode(gpu_ctx, curve, b"".join(recs), True)
    xy0, st0 = api.g1_decode(gpu_ctx, curve, b"".join(recs), False)
    moved = st1 != st0
    assert (st1[moved] == NOT_IN_G1).all() and (st0[moved] == OK).all() and (xy1[~moved] == xy0[~moved]).all()


def _fixture_setups(pm, key, e):
    from polymath_amd import polymath as PM
    q = r1cs_from_json(e["r1cs"])
    r1cs = PM.R1CS(q.m0, q.mw, q.a, q.b, q.c)
    inst, wit, r_a = [I(v) for v in e["instance"]], [I(v) for v in e["witness"]], [I(v) for v in e["r_a"]]
    return r1cs, inst, wit, r_a


@pytest.mark.gpu
def test_export_compressed_equals_fixture_bytes(gpu_ctx):
    from polymath_amd import polymath as PM
    proofs = {e["name"]: e for e in load_golden("proofs.json")}
    pm = PM.Polymath("bls12_381", "merlin", ctx=gpu_ctx)
    for key in load_golden("pk_wire.json")["keys"]:
        e = proofs[key["name"]]
        r1cs, inst, wit, _ = _fixture_setups(pm, key, e)
        pk = pm.setup((r1cs, inst, wit), I(e["x_trapdoor"]), I(e["z_trapdoor"]))
        data = bytes.fromhex(key["pk_bytes"])
        for which, (off, cnt) in _vec_offsets(data, "bls12_381").items():
            assert pk.export_bases_compressed(which) == data[off:off + 48 * cnt], (key["name"], which)
            if cnt > 2:
                assert pk.export_bases_compressed(which, 1, cnt - 2) == data[off + 48:off + 48 * (cnt - 1)]
        assert pm.pk_serialize(pk, r1cs, bytes.fromhex(key["vk"]["bytes"])) == data
        pk.free()


@pytest.mark.gpu
def test_fixture_keys_load_and_prove(gpu_ctx):
    from polymath_amd import polymath as PM
    proofs = {e["name"]: e for e in load_golden("proofs.json")}
    default_chunk = gpu_ctx.get_option("wire_chunk_log")
    for key in load_golden("pk_wire.json")["keys"]:
        e = proofs[key["name"]]
        data = bytes.fromhex(key["pk_bytes"])
        ref_pm = PM.Polymath("bls12_381", "merlin", ctx=gpu_ctx)
        ref_pk, _, _ = ref_pm.pk_from_bytes(data)
        ref_bases = [ref_pk.export_bases(v) for v in range(6)]
        ref_info = (ref_pk.n, ref_pk.m0, ref_pk.sigma, ref_pk.omega_limbs.tolist(), ref_pk.base_lens)
        ref_pk.free()
        _, inst, wit, r_a = _fixture_setups(ref_pm, key, e)
        for validate in (True, False):
            for chunk in (default_chunk, 4):
                gpu_ctx.set_option("wire_chunk_log", chunk)
                for tname, ref in e["proofs"].items():
                    pm = PM.Polymath("bls12_381", tname, ctx=gpu_ctx)
                    pk, vk_bytes = pm.pk_load_bytes(memoryview(data), validate)
                    assert vk_bytes.hex() == key["vk"]["bytes"]
                    assert (pk.n, pk.m0, pk.sigma, pk.omega_limbs.tolist(), pk.base_lens) == ref_info
                    if tname == "merlin":
                        for v in range(6):
                            assert (pk.export_bases(v) == ref_bases[v]).all(), (key["name"], v)
                    proof = pm.prove_limbs(pk, inst, pm.field.fr_limbs(inst), pm.field.fr_limbs(wit), r_a)
                    assert proof.to_bytes().hex() == ref["bytes"], (key["name"], tname, validate, chunk)
                    pk.free()


@pytest.mark.gpu
def test_bn254_round_trip_2p12(gpu_ctx):
    from polymath_amd import api, circuits as PC
    from polymath_amd import polymath as PM
    curve = "bn254"
    c = CURVES[curve]
    lc = PC.synthetic_r1cs_native(curve, (1 << 12) - 100)
    g = PC.SplitMix64(0xB254)
    x, z, r_a = g.fr(c.r), g.fr(c.r), [g.fr(c.r), g.fr(c.r)]
    pm = PM.Polymath(curve, "merlin", ctx=gpu_ctx)
    pk = pm.setup(lc, x, z)
    vk = pm.make_vk(pk, x, z)
    gpu_ctx.set_option("wire_chunk_log", 9)
    data = pm.pk_serialize(pk, lc, vk)
    f = pm.field
    for which, (off, cnt) in _vec_offsets(data, curve).items():
        xy = pk.export_bases(which)
        expect = b"".join(PM.ser_g1(f, f.g1_affine(row, not row.any())) for row in xy)
        assert data[off:off + 32 * cnt] == expect, which
    pk2, vk2 = pm.pk_load_bytes(data)
    assert vk2 == vk
    for v in range(6):
        assert (pk2.export_bases(v) == pk.export_bases(v)).all(), v
    p1 = pm.prove_native(pk, lc.inst_limbs, lc.wit_limbs, r_a)
    p2 = pm.prove_native(pk2, lc.inst_limbs, lc.wit_limbs, r_a)
    assert p1 == p2 and api.verify(curve, "merlin", vk2, lc.inst_limbs[1:], p2)
    pk.free()
    pk2.free()


@pytest.mark.gpu
def test_bls12_381_at_2p16_single_and_sharded(gpu_ctx):
    import threading
    from polymath_amd import api, circuits as PC
    from polymath_amd import polymath as PM
    curve = "bls12_381"
    c = CURVES[curve]
    lc = PC.synthetic_r1cs_native(curve, (1 << 16) - 100)
    g = PC.SplitMix64(0x1616)
    x, z, r_a = g.fr(c.r), g.fr(c.r), [g.fr(c.r), g.fr(c.r)]
    pm = PM.Polymath(curve, "merlin", ctx=gpu_ctx)
    pk = pm.setup(lc, x, z)
    ref = pm.prove_native(pk, lc.inst_limbs, lc.wit_limbs, r_a)
    data = pm.pk_serialize(pk, lc, pm.make_vk(pk, x, z))
    pk.free()
    pk2, _ = pm.pk_load_bytes(data, validate=True)
    assert pm.prove_native(pk2, lc.inst_limbs, lc.wit_limbs, r_a) == ref
    pk2.free()
    for layout in ("pairs", "vector"):
        comms = api.Comm.local_group(2)
        pms = [PM.Polymath(curve, "merlin", device=0) for _ in range(2)]
        for r in range(2):
            pms[r].ctx.set_comm(comms[r])
        keys = [pms[r].pk_load_bytes(data, True, r, 2, layout)[0] for r in range(2)]
        outs, errs = [None, None], []

        def body(r):
            try:
                outs[r] = pms[r].prove_native(keys[r], lc.inst_limbs, lc.wit_limbs, r_a,
                                              combine=_LocalCombine(comms[r], curve) if layout == "pairs" else None)
            except BaseException as ex:        # noqa: BLE001 -- re-raised below
                errs.append(ex)
                comms[r].abort("rank %d raised" % r)
        th = [threading.Thread(target=body, args=(r,), daemon=True) for r in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join(600)
        assert not errs and not any(t.is_alive() for t in th), errs
        assert outs == [ref, ref], layout
        for r in range(2):
            keys[r].free()
            pms[r].ctx.set_comm(None)
            pms[r].ctx.close()
        for cm in comms:
            cm.close()


class _LocalCombine:
    """PointCombiner over a local communicator: all-gather of the partial points + pm_g1_sum"""

    def __init__(self, comm, curve):
        self.comm, self.curve = comm, curve

    def many(self, pts):
        from polymath_amd import api
        xy = np.stack([np.asarray(p, dtype=np.uint64) for p, _ in pts])
        inf = np.array([i for _, i in pts], dtype=np.int64)
        all_xy, all_inf = self.comm.all_gather(xy), self.comm.all_gather(inf)
        return [api.g1_sum(self.curve, all_xy[:, j], all_inf[:, j].astype(np.int32)) for j in range(len(pts))]


@pytest.mark.gpu
def test_refusals_name_the_point_and_leave_the_context_usable(gpu_ctx):
    from polymath_amd import api
    from polymath_amd import polymath as PM
    c = CURVES["bls12_381"]
    rng = np.random.default_rng(0x5EF)
    key = [k for k in load_golden("pk_wire.json")["keys"] if k["name"] == "m0_12"][0]   # 33 x powers, 35 lcs points: 2+ chunks of 16
    e = {x["name"]: x for x in load_golden("proofs.json")}[key["name"]]
    data = bytes.fromhex(key["pk_bytes"])
    gpu_ctx.set_option("wire_chunk_log", 4)
    pm = PM.Polymath("bls12_381", "merlin", ctx=gpu_ctx)
    offs = _vec_offsets(data, "bls12_381")
    gen = ref_encode(c, c.g1)
    off_curve = gen
    while ref_decode(c, off_curve, False)[0] != NOT_ON_CURVE:
        off_curve = ref_encode(c, (int(rng.integers(1, 2 ** 62)), 0))
    outside = ref_encode(c, _random_curve_point(c, rng))
    assert ref_decode(c, outside, True)[0] == NOT_IN_G1
    bad = {BAD_FLAGS: bytes([gen[0] & 0x7F]) + gen[1:], GE_P: bytes([c.p.to_bytes(48, "big")[0] | 0x80]) + c.p.to_bytes(48, "big")[1:],
           NOT_ON_CURVE: off_curve, NOT_IN_G1: outside, NONCANON_INF: bytes([0xC0]) + bytes(46) + b"\x01", INF_SIGN: bytes([0xE0]) + bytes(47)}
    first, last = WIRE_ORDER[0], WIRE_ORDER[-1]
    spots = [(first, 0), (first, 15), (first, 16), (last, 31), (last, offs[last][1] - 1)]
    for which, idx in spots:
        assert idx < offs[which][1]
        for code, rec in bad.items():
            o = offs[which][0] + 48 * idx
            corrupt = data[:o] + rec + data[o + 48:]
            with pytest.raises(api.PolymathError) as ex:
                pm.pk_load_bytes(corrupt, True)
            assert ex.value.status == 1
            assert "%s[%d]: %s" % (NAMES[which], idx, REASONS[code]) in str(ex.value), str(ex.value)
        o = offs[which][0] + 48 * idx
        pk, _ = pm.pk_load_bytes(data[:o] + bad[NOT_IN_G1] + data[o + 48:], validate=False)   # unchecked: loads
        pk.free()
    # the byte string itself
    vk = VK_LEN["bls12_381"]
    n_at, m0_at, sigma_at, omega_at = vk - 56, vk - 48, vk - 40, vk - 32
    u64 = lambda at, v: data[:at] + struct.pack("<Q", v) + data[at + 8:]
    xo, xc = offs[WIRE_ORDER[0]]
    shorter = data[:xo - 8] + struct.pack("<Q", xc - 1) + data[xo:xo + 48 * (xc - 1)] + data[xo + 48 * xc:]
    omega = int.from_bytes(data[omega_at:omega_at + 32], "little")
    cases = {"truncated key": data[:-1], "trailing bytes after the key": data + b"\x00", "does not match the key's shape": shorter,
             "vk.m0 disagrees": u64(m0_at, struct.unpack_from("<Q", data, m0_at)[0] + 1),
             "vk.n / vk.sigma disagree": u64(n_at, struct.unpack_from("<Q", data, n_at)[0] * 2),
             "vk.omega is not the generator": data[:omega_at] + (omega * omega % c.r).to_bytes(32, "little") + data[omega_at + 32:]}
    for why, blob in cases.items():
        with pytest.raises(api.PolymathError) as ex:
            pm.pk_load_bytes(blob, True)
        assert ex.value.status == 1 and why in str(ex.value), (why, str(ex.value))
    # the same context still loads and proves
    pk, _ = pm.pk_load_bytes(data)
    inst, wit, r_a = [I(v) for v in e["instance"]], [I(v) for v in e["witness"]], [I(v) for v in e["r_a"]]
    proof = pm.prove_limbs(pk, inst, pm.field.fr_limbs(inst), pm.field.fr_limbs(wit), r_a)
    assert proof.to_bytes().hex() == e["proofs"]["merlin"]["bytes"]
    pk.free()
