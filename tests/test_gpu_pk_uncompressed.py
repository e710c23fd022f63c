"""GPU: proving keys in ark's uncompressed form -- PM_WIRE_UNCOMPRESSED in pm_g1_decode, pm_pk_load_bytes and
pm_pk_export_bases_compressed (csrc/g1_codec.hip: k_g1_decode_uncompressed, k_g1_encode_uncompressed).

The specification is the host mirror's deser_g1_uncompressed / ser_g1_uncompressed (polymath_amd/host/wire.hpp).  Expected verdicts
and Montgomery words come from Python integers computed here ([r]P unreduced for subgroup membership) and from the literal records
of the format's description, never from the code under test.  Counts 1, 255, 256, 257, 513 are the edges of the 256-lane workgroup;
wire_chunk_log 4 puts staging-chunk boundaries inside every one of them.
"""
import ctypes as ct
import struct

import numpy as np
import pytest

from helpers import I, load_golden, r1cs_from_json
from oracle.pyref.fields import CURVES, _jac_add_affine, _jac_dbl, g1_add, g1_neg

OK, BAD_FLAGS, GE_P, NOT_ON_CURVE, NOT_IN_G1, NONCANON_INF, INF_SIGN = range(7)
NB = {"bls12_381": 48, "bn254": 32}
VK_LEN = {"bls12_381": 392, "bn254": 280}
VK_LEN_U = {"bls12_381": 728, "bn254": 504}
WIRE_ORDER = (0, 1, 4, 2, 3, 5)
COUNTS = (1, 255, 256, 257, 513)
BLS_G = bytes.fromhex("17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb"
                      "08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1")
LITERALS = {"bls12_381": (BLS_G, b"\x40" + bytes(95)), "bn254": (b"\x01" + bytes(31) + b"\x02" + bytes(31), bytes(63) + b"\x40")}


# ------------------------------------------------------------------------------------------------------------- big-int codec
def times(c, P, k):
    """[k] P without reducing k mod r"""
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


def enc_c(c, P):
    """the compressed record (the format test_pk_bytes.py pins)"""
    if c.name == "bls12_381":
        if P is None:
            return bytes([0xC0]) + bytes(47)
        b = bytearray(P[0].to_bytes(48, "big"))
        b[0] |= 0x80 | (0x20 if P[1] > c.p - P[1] else 0)
        return bytes(b)
    if P is None:
        return bytes(31) + b"\x40"
    b = bytearray(P[0].to_bytes(32, "little"))
    b[31] |= 0x80 if P[1] > c.p - P[1] else 0
    return bytes(b)


def enc_u(c, P, sign=None):
    """the uncompressed record; sign: BN254's "y > -y" bit as the writer sets it (None), or forced set / clear"""
    if c.name == "bls12_381":
        return b"\x40" + bytes(95) if P is None else P[0].to_bytes(48, "big") + P[1].to_bytes(48, "big")
    if P is None:
        return bytes(63) + b"\x40"
    b = bytearray(P[0].to_bytes(32, "little") + P[1].to_bytes(32, "little"))
    if (P[1] > c.p - P[1]) if sign is None else sign:
        b[63] |= 0x80
    return bytes(b)


def dec_u(c, rec, validate, in_g1=False):
    """deser_g1_uncompressed restated on integers -> (status, point or None); in_g1: known to be a multiple of G"""
    if c.name == "bls12_381":
        f = rec[0]
        if f & 0x80:
            return BAD_FLAGS, None
        if f & 0x20:
            return (INF_SIGN if f & 0x40 else BAD_FLAGS), None
        inf = bool(f & 0x40)
        x, y = int.from_bytes(bytes([f & 0x1F]) + rec[1:48], "big"), int.from_bytes(rec[48:], "big")
    else:
        f = rec[63]
        if f & 0xC0 == 0xC0:
            return BAD_FLAGS, None
        inf = bool(f & 0x40)
        x, y = int.from_bytes(rec[:32], "little"), int.from_bytes(rec[32:63] + bytes([f & 0x3F]), "little")
    if inf:
        return (NONCANON_INF, None) if x or y else (OK, None)
    if x >= c.p or y >= c.p:
        return GE_P, None
    if (y * y - x * x * x - c.b) % c.p:
        return NOT_ON_CURVE, None
    if validate and c.name == "bls12_381" and not in_g1 and times(c, (x, y), c.r) is not None:
        return NOT_IN_G1, None
    return OK, (x, y)


def mont_rows(c, pts):
    """points (None: infinity / refused) -> the ABI's rows: x || y in Montgomery form, little-endian 64-bit limbs, all-zero for None"""
    nq = c.fq_limbs64
    R = 1 << (64 * nq)
    buf = b"".join(bytes(16 * nq) if P is None else (P[0] * R % c.p).to_bytes(8 * nq, "little") + (P[1] * R % c.p).to_bytes(8 * nq, "little")
                   for P in pts)
    return np.frombuffer(buf, dtype=np.uint64).reshape(len(pts), 2 * nq)


def _random_curve_point(c, rng):
    while True:
        x = int(rng.integers(0, 2 ** 62)) * (1 << 300) % c.p + int(rng.integers(1, 2 ** 62))
        y = _sqrt(c, (x ** 3 + c.b) % c.p)
        if y is not None:
            return (x, y)


_RECORDS = {}


def records(curve):
    """513 records, every class among the first 64 or so -> (records, in_g1 flags, {validate: (status array, Montgomery rows)})"""
    if curve in _RECORDS:
        return _RECORDS[curve]
    c = CURVES[curve]
    bls = curve == "bls12_381"
    nb = NB[curve]
    order = "big" if bls else "little"
    rng = np.random.default_rng(0x0C0DEC + nb)
    gen, inf = LITERALS[curve]
    assert enc_u(c, c.g1) == gen and enc_u(c, None) == inf
    mult, P = [], None
    for _ in range(230):
        P = g1_add(c, P, c.g1)
        mult.append(P)
    fq = lambda v: v.to_bytes(nb, order)
    xy = lambda x, y: fq(x) + fq(y)                     # raw coordinates, no flags
    top = 2 ** 381 if bls else 2 ** 256                  # x's width once the flag bits are masked; y: 2^384 / 2^254
    ytop = 2 ** 384 if bls else 2 ** 254
    G = c.g1
    crafted = [gen]                                      # record 0: count = 1 decodes the literal generator
    flag = (lambda rec, bits: bytes([rec[0] | bits]) + rec[1:]) if bls else (lambda rec, bits: rec[:63] + bytes([rec[63] | bits]))
    if bls:
        crafted += [flag(gen, 0x80), flag(enc_u(c, mult[4]), 0xA0), flag(gen, 0x20), flag(inf, 0x20), flag(inf, 0x80), flag(inf, 0xA0)]
    else:
        crafted += [flag(inf, 0x80), flag(gen, 0xC0), enc_u(c, mult[6], sign=True), enc_u(c, mult[6], sign=False),
                    enc_u(c, g1_neg(c, mult[6]), sign=True), enc_u(c, g1_neg(c, mult[6]), sign=False)]
    stray = bytearray(inf)
    stray[5] |= 0x01
    crafted.append(bytes(stray))                         # a stray bit in the x half of infinity
    stray = bytearray(inf)
    stray[nb + 7] |= 0x10
    crafted.append(bytes(stray))                         # ... in the y half
    stray = bytearray(inf)
    stray[0 if bls else 63] |= 0x01
    crafted.append(bytes(stray))                         # ... in the flag byte
    crafted += [inf, xy(c.p, G[1]), xy(G[0], c.p), xy(c.p + 1, G[1]), xy(G[0], c.p + 1), xy(top - 1, G[1]), xy(G[0], ytop - 1),
                xy(c.p, c.p), xy(G[0], (G[1] + 1) % c.p), xy((G[0] + 1) % c.p, G[1]), xy(0, 0), xy(G[0], 0)]
    for k in (1, 7, 100):                                # y + 1 on further points
        crafted.append(xy(mult[k][0], (mult[k][1] + 1) % c.p))
    outside = []
    if bls:                                              # on the curve, outside G1 (the cofactor is ~2^126)
        for _ in range(24):
            outside.append(_random_curve_point(c, rng))
        T = times(c, outside[0], c.r)                    # a point of the cofactor's torsion, and G + T
        assert T is not None
        outside += [T, g1_add(c, c.g1, T), g1_neg(c, T)]
        crafted += [enc_u(c, Q) for Q in outside]
    recs = list(crafted)
    in_g1 = [False] * len(recs)
    in_g1[0] = True
    k = 0
    while len(recs) < 513:                               # multiples of G, their negatives, and infinity now and then
        if k % 41 == 40:
            recs.append(inf)
            in_g1.append(False)
        else:
            Q = mult[k % len(mult)] if k % 2 == 0 else g1_neg(c, mult[k % len(mult)])
            recs.append(enc_u(c, Q))
            in_g1.append(True)
        k += 1
    # a crafted record sits in the LAST lane of the first workgroup, the first of the second, and the very last record
    recs[255], recs[256], recs[512] = xy(G[0], (G[1] + 1) % c.p), flag(inf, 0x80 if not bls else 0x20), xy(c.p, G[1])
    in_g1[255] = in_g1[256] = in_g1[512] = False
    expect = {}
    for validate in (True, False):
        verdicts = [dec_u(c, rec, validate, in_g1=g) for rec, g in zip(recs, in_g1)]
        expect[validate] = (np.array([v[0] for v in verdicts], dtype=np.uint8), mont_rows(c, [v[1] for v in verdicts]))
    st = expect[True][0]
    classes = {BAD_FLAGS, GE_P, NOT_ON_CURVE, NONCANON_INF} | ({NOT_IN_G1, INF_SIGN} if bls else set())
    assert classes <= set(st[:64].tolist()) and (st == OK).sum() > 400
    if bls:
        assert (st == NOT_IN_G1).sum() == 27 and (expect[False][0] == NOT_IN_G1).sum() == 0
    _RECORDS[curve] = (recs, in_g1, expect)
    return _RECORDS[curve]


# ------------------------------------------------------------------------------------------------------------------ decode
@pytest.mark.gpu
@pytest.mark.parametrize("curve", ["bls12_381", "bn254"])
def test_decode_against_integers(gpu_ctx, curve):
    from polymath_amd import api
    recs, _, expect = records(curve)
    default_chunk = gpu_ctx.get_option("wire_chunk_log")
    for chunk in (4, default_chunk):
        gpu_ctx.set_option("wire_chunk_log", chunk)
        for count in COUNTS:
            blob = b"".join(recs[:count])
            for validate in (True, False):
                xy, st = api.g1_decode(gpu_ctx, curve, blob, validate, form="uncompressed")
                want_st, want_xy = expect[validate]
                bad = np.nonzero(st != want_st[:count])[0]
                assert not len(bad), (curve, chunk, count, validate, bad[:8].tolist(), st[bad[:8]].tolist(), want_st[bad[:8]].tolist())
                rows = np.nonzero((xy != want_xy[:count]).any(axis=1))[0]
                assert not len(rows), (curve, chunk, count, validate, rows[:8].tolist())
    # validation off: exactly the subgroup verdicts change (to the point itself); the off-curve ones do not
    blob = b"".join(recs)
    xy1, st1 = api.g1_decode(gpu_ctx, curve, blob, True, form="uncompressed")
    xy0, st0 = api.g1_decode(gpu_ctx, curve, blob, False, form="uncompressed")
    moved = st1 != st0
    assert (st1[moved] == NOT_IN_G1).all() and (st0[moved] == OK).all() and (xy1[~moved] == xy0[~moved]).all()
    assert moved.sum() == (27 if curve == "bls12_381" else 0)
    assert (st0 == NOT_ON_CURVE).sum() == (st1 == NOT_ON_CURVE).sum() >= 6 and not xy0[st0 != OK].any()


@pytest.mark.gpu
@pytest.mark.parametrize("curve", ["bls12_381", "bn254"])
def test_sign_bit_is_written_and_not_read_on_bn254_and_literals_decode(gpu_ctx, curve):
    from polymath_amd import api
    c = CURVES[curve]
    gen, inf = LITERALS[curve]
    xy, st = api.g1_decode(gpu_ctx, curve, gen + inf, True, form="uncompressed")
    assert st.tolist() == [OK, OK] and (xy == mont_rows(c, [c.g1, None])).all()
    if curve == "bn254":
        P = times(c, c.g1, 12345)
        pair = enc_u(c, P, sign=True) + enc_u(c, P, sign=False)
        assert pair[:63] == pair[64:127] and pair[63] ^ pair[127] == 0x80
        xy, st = api.g1_decode(gpu_ctx, curve, pair, True, form="uncompressed")
        assert st.tolist() == [OK, OK] and (xy == mont_rows(c, [P, P])).all()


@pytest.mark.gpu
@pytest.mark.parametrize("curve", ["bls12_381", "bn254"])
def test_both_forms_decode_to_the_same_words(gpu_ctx, curve):
    from polymath_amd import api
    c = CURVES[curve]
    rng = np.random.default_rng(0xF0F0)
    pts, P = [None], None
    for k in range(300):
        P = g1_add(c, P, c.g1)
        pts += [P, g1_neg(c, P)] if k % 3 else [P]
    if curve == "bls12_381":
        pts += [_random_curve_point(c, rng) for _ in range(12)]
    pts = pts[:513]
    gpu_ctx.set_option("wire_chunk_log", 5)
    for validate in (True, False):
        xy_c, st_c = api.g1_decode(gpu_ctx, curve, b"".join(enc_c(c, Q) for Q in pts), validate)
        xy_u, st_u = api.g1_decode(gpu_ctx, curve, b"".join(enc_u(c, Q) for Q in pts), validate, form="uncompressed")
        assert (st_c == st_u).all() and (xy_c == xy_u).all(), (curve, validate)
        assert (st_u == NOT_IN_G1).sum() == (12 if validate and curve == "bls12_381" else 0)
        assert xy_u[1:len(pts) - 12].any(axis=1).all()


# -------------------------------------------------------------------------------------------------------------------- keys
def vec_offsets(data, curve, form):
    """{pm_base_vec: (byte offset of point 0, count)} of a serialised key in either form"""
    rec = NB[curve] * (2 if form == "uncompressed" else 1)
    o = (VK_LEN_U if form == "uncompressed" else VK_LEN)[curve] + 24
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
        o += 8 + rec * cnt
    assert o == len(data)
    return out


def dec_c(c, rec):
    """a valid compressed record -> point (integers)"""
    if c.name == "bls12_381":
        if rec[0] & 0x40:
            return None
        x, larger = int.from_bytes(bytes([rec[0] & 0x1F]) + rec[1:], "big"), bool(rec[0] & 0x20)
    else:
        if rec[31] & 0x40:
            return None
        x, larger = int.from_bytes(rec[:31] + bytes([rec[31] & 0x3F]), "little"), bool(rec[31] & 0x80)
    y = _sqrt(c, (x ** 3 + c.b) % c.p)
    return (x, c.p - y if (y > c.p - y) != larger else y)


def to_uncompressed(data, curve):
    """A serialize_compressed key -> the serialize_uncompressed one: the points on Python integers, the vk (G2) by the Python twin,
    which tests/test_pk_uncompressed_abi.py checks against the host mirror's bytes without a GPU."""
    from polymath_amd import polymath as PM
    c = CURVES[curve]
    offs = vec_offsets(data, curve, "compressed")
    nb = NB[curve]
    rd = PM._Reader(data[:VK_LEN[curve]])
    out = [PM.VerifyingKey.read(PM.Field(curve), rd).to_bytes("uncompressed"), data[VK_LEN[curve]:offs[WIRE_ORDER[0]][0] - 8]]
    assert len(out[0]) == VK_LEN_U[curve]
    for which in WIRE_ORDER:
        off, cnt = offs[which]
        out.append(struct.pack("<Q", cnt))
        out.extend(enc_u(c, dec_c(c, data[off + nb * i:off + nb * (i + 1)])) for i in range(cnt))
    wide = b"".join(out)
    assert len(wide) == len(data) + nb * sum(cnt for _, cnt in offs.values()) + VK_LEN_U[curve] - VK_LEN[curve]
    return wide


_KEYS = {}


def golden(name):
    """(entry of proofs.json, compressed bytes, uncompressed bytes) of a fixture key, transcoded once"""
    if name not in _KEYS:
        key = [k for k in load_golden("pk_wire.json")["keys"] if k["name"] == name][0]
        e = {x["name"]: x for x in load_golden("proofs.json")}[name]
        data = bytes.fromhex(key["pk_bytes"])
        _KEYS[name] = (e, data, to_uncompressed(data, "bls12_381"))
    return _KEYS[name]


def _assignment(e):
    return [I(v) for v in e["instance"]], [I(v) for v in e["witness"]], [I(v) for v in e["r_a"]]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["m0_12", "mimc2"])
def test_uncompressed_fixture_key_loads_and_proves(gpu_ctx, name):
    """On the parent commit bit 8 of `validate` read as plain "validate" and the parse refused these bytes."""
    from polymath_amd import polymath as PM
    e, data, wide = golden(name)
    inst, wit, r_a = _assignment(e)
    pm = PM.Polymath("bls12_381", "merlin", ctx=gpu_ctx)
    ref_pk, ref_vk = pm.pk_load_bytes(data)
    ref_bases = [ref_pk.export_bases(v) for v in range(6)]
    ref_info = (ref_pk.n, ref_pk.m0, ref_pk.sigma, ref_pk.omega_limbs.tolist(), ref_pk.base_lens)
    ref_pk.free()
    for validate in (True, False):
        for chunk in (4, 20):
            gpu_ctx.set_option("wire_chunk_log", chunk)
            pk, vk_u = pm.pk_load_bytes(memoryview(wide), validate, form="uncompressed")
            assert len(vk_u) == 728 and vk_u == wide[:728] and pm.vk_transcode(vk_u, "uncompressed", "compressed") == ref_vk
            assert (pk.n, pk.m0, pk.sigma, pk.omega_limbs.tolist(), pk.base_lens) == ref_info
            for v in range(6):
                assert (pk.export_bases(v) == ref_bases[v]).all(), (name, validate, chunk, v)
            proof = pm.prove_limbs(pk, inst, pm.field.fr_limbs(inst), pm.field.fr_limbs(wit), r_a)
            assert proof.to_bytes().hex() == e["proofs"]["merlin"]["bytes"], (name, validate, chunk)
            pk.free()


@pytest.mark.gpu
def test_export_uncompressed_and_round_trip(gpu_ctx):
    from polymath_amd import api
    from polymath_amd import polymath as PM
    e, data, wide = golden("m0_12")
    q = r1cs_from_json(e["r1cs"])
    r1cs = PM.R1CS(q.m0, q.mw, q.a, q.b, q.c)
    pm = PM.Polymath("bls12_381", "merlin", ctx=gpu_ctx)
    pk, _ = pm.pk_load_bytes(data)
    offs = vec_offsets(wide, "bls12_381", "uncompressed")
    default_chunk = gpu_ctx.get_option("wire_chunk_log")
    for chunk in (default_chunk, 4):
        gpu_ctx.set_option("wire_chunk_log", chunk)
        for which, (off, cnt) in offs.items():
            assert pk.export_bases_compressed(which, form="uncompressed") == wide[off:off + 96 * cnt], (chunk, which)
            for lo, n in ((1, cnt - 2), (15, 3), (16, 17), (cnt - 1, 1), (3, 0)):
                if lo + n <= cnt:
                    assert pk.export_bases_compressed(which, lo, n, form="uncompressed") == wide[off + 96 * lo:off + 96 * (lo + n)], (chunk, which, lo, n)
    # export -> load -> export is the identity
    assert pm.pk_serialize(pk, r1cs, wide[:728], form="uncompressed") == wide
    pk2, _ = pm.pk_load_bytes(wide, form="uncompressed")
    assert pm.pk_serialize(pk2, r1cs, wide[:728], form="uncompressed") == wide and pm.pk_serialize(pk2, r1cs, data[:392]) == data
    pk2.free()
    # a bad `which` under the flag, and any other high bit
    L, buf = gpu_ctx.L, ct.create_string_buffer(96 * 64)
    for which in (6 | 256, 255 | 256, 512, 512 | 256, 1024 | 1, 1 << 16, -1, -256):
        assert L.pm_pk_export_bases_compressed(gpu_ctx.h, pk.h, which, 0, 1, buf) == 1, which
    assert L.pm_pk_export_bases_compressed(gpu_ctx.h, pk.h, 0 | 256, 0, pk.base_lens[0] + 1, buf) == 1      # the ranges are unchanged
    assert L.pm_pk_export_bases_compressed(gpu_ctx.h, pk.h, 0 | 256, 0, 1, buf) == 0 and buf.raw[:96] == wide[offs[0][0]:offs[0][0] + 96]
    pk.free()


@pytest.mark.gpu
def test_bn254_round_trip_in_the_uncompressed_form(gpu_ctx):
    from polymath_amd import api, circuits as PC
    from polymath_amd import polymath as PM
    curve = "bn254"
    c = CURVES[curve]
    lc = PC.synthetic_r1cs_native(curve, (1 << 9) - 100)
    g = PC.SplitMix64(0xB254)
    x, z, r_a = g.fr(c.r), g.fr(c.r), [g.fr(c.r), g.fr(c.r)]
    pm = PM.Polymath(curve, "merlin", ctx=gpu_ctx)
    pk = pm.setup(lc, x, z)
    vk = pm.make_vk(pk, x, z)
    vk_u = pm.vk_transcode(vk, "compressed", "uncompressed")
    assert len(vk_u) == 504 and pm.vk_transcode(vk_u, "uncompressed", "compressed") == vk
    gpu_ctx.set_option("wire_chunk_log", 7)
    data, wide = pm.pk_serialize(pk, lc, vk), pm.pk_serialize(pk, lc, vk_u, form="uncompressed")
    offs_c, offs_u = vec_offsets(data, curve, "compressed"), vec_offsets(wide, curve, "uncompressed")
    for which, (off, cnt) in offs_u.items():             # the exported records against integers, through the compressed records
        oc = offs_c[which][0]
        expect = b"".join(enc_u(c, dec_c(c, data[oc + 32 * i:oc + 32 * (i + 1)])) for i in range(cnt))
        assert wide[off:off + 64 * cnt] == expect, which
    for validate in (True, False):
        pk2, vk2 = pm.pk_load_bytes(wide, validate, form="uncompressed")
        assert vk2 == vk_u
        for v in range(6):
            assert (pk2.export_bases(v) == pk.export_bases(v)).all(), v
        p2 = pm.prove_native(pk2, lc.inst_limbs, lc.wit_limbs, r_a)
        assert p2 == pm.prove_native(pk, lc.inst_limbs, lc.wit_limbs, r_a) and api.verify(curve, "merlin", vk, lc.inst_limbs[1:], p2)
        pk2.free()
    for blob, form in ((wide, "compressed"), (data, "uncompressed")):
        with pytest.raises(api.PolymathError) as ex:
            pm.pk_load_bytes(blob, form=form)
        assert ex.value.status == 1
    pk.free()


@pytest.mark.gpu
def test_refusals(gpu_ctx):
    from polymath_amd import api
    from polymath_amd import polymath as PM
    c = CURVES["bls12_381"]
    rng = np.random.default_rng(0x5EF)
    e, data, wide = golden("m0_12")                        # 33 x powers: records 17 sits in the second chunk of 16
    gpu_ctx.set_option("wire_chunk_log", 4)
    pm = PM.Polymath("bls12_381", "merlin", ctx=gpu_ctx)
    offs = vec_offsets(wide, "bls12_381", "uncompressed")

    def refused(blob, validate=True, form="uncompressed", why=None, **kw):
        with pytest.raises(api.PolymathError) as ex:
            pm.pk_load_bytes(blob, validate, form=form, **kw)
        assert ex.value.status == 1 and (why is None or why in str(ex.value)), str(ex.value)

    refused(wide[:-1], why="truncated key")
    refused(wide + b"\x00", why="trailing bytes after the key")
    refused(data, form="uncompressed")                     # compressed bytes with the flag
    refused(wide, form="compressed")                       # uncompressed bytes without it
    refused(data, validate=False, form="uncompressed")
    refused(wide, validate=False, form="compressed")
    at = offs[0][0] + 96 * 17
    G = c.g1
    off_curve = G[0].to_bytes(48, "big") + ((G[1] + 1) % c.p).to_bytes(48, "big")
    outside = _random_curve_point(c, rng)
    assert times(c, outside, c.r) is not None
    put = lambda rec, o=at: wide[:o] + rec + wide[o + 96:]
    for validate in (True, False):
        refused(put(off_curve), validate, why="x_powers_g1[17]: G1: not on the curve")
        refused(put(bytes([wide[at] | 0x80]) + wide[at + 1:at + 96]), validate, why="x_powers_g1[17]: G1: not an uncompressed point")
    refused(put(enc_u(c, outside)), True, why="x_powers_g1[17]: G1: not in the prime-order subgroup")
    pk, _ = pm.pk_load_bytes(put(enc_u(c, outside)), False, form="uncompressed")       # unchecked: loads
    assert (pk.export_bases(0, 17, 1) == mont_rows(c, [outside])).all()
    pk.free()
    # a shard reads and checks only its resident ranges: rank 1 of 2 (pairs layout) does not see a bad record it does not hold
    comms = api.Comm.local_group(2)
    pm1 = PM.Polymath("bls12_381", "merlin", device=0)
    pm1.ctx.set_comm(comms[1])
    pm1.ctx.set_option("wire_chunk_log", 4)
    pk1, _ = pm1.pk_load_bytes(wide, True, 1, 2, "pairs", form="uncompressed")
    held, absent = None, None
    for which in WIRE_ORDER:
        for i in range(offs[which][1]):
            try:
                pk1.export_bases(which, i, 1)
                held = held or (which, i)
            except api.PolymathError:
                absent = absent or (which, i)
    pk1.free()
    assert held and absent
    spot = lambda wi: offs[wi[0]][0] + 96 * wi[1]
    pk1, _ = pm1.pk_load_bytes(put(off_curve, spot(absent)), True, 1, 2, "pairs", form="uncompressed")
    pk1.free()
    with pytest.raises(api.PolymathError) as ex:
        pm1.pk_load_bytes(put(off_curve, spot(held)), True, 1, 2, "pairs", form="uncompressed")
    assert ex.value.status == 1 and "G1: not on the curve" in str(ex.value)
    refused(put(off_curve, spot(absent)), why="G1: not on the curve")          # the whole key sees it
    pm1.ctx.set_comm(None)
    pm1.ctx.close()
    for cm in comms:
        cm.close()
    # the same context still loads and proves
    pk, _ = pm.pk_load_bytes(wide, form="uncompressed")
    inst, wit, r_a = _assignment(e)
    proof = pm.prove_limbs(pk, inst, pm.field.fr_limbs(inst), pm.field.fr_limbs(wit), r_a)
    assert proof.to_bytes().hex() == e["proofs"]["merlin"]["bytes"]
    pk.free()
