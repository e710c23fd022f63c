"""CPU: PM_WIRE_UNCOMPRESSED at every layer of the boundary -- a flag of the `validate` argument of pm_g1_decode / pm_pk_load_bytes
and of the `which` argument of pm_pk_export_bases_compressed, and nothing else new there.  The header's enum, api.py and the -sys
crate carry 0 and 256; the Rust wrapper has a WireForm and a loader and exporter that take it; the pinned counts (70 entry points,
PM_NUM_OPTIONS = 9) hold; api hands the library validate | 256 and which | 256 (seen by a stand-in library); the Python twin
(polymath.ser_g1 / deser_g1 / ser_g2 / deser_g2 / VerifyingKey with a form) against the literal records of the format and against
Python integers; a golden key transcoded by the twin has the length the formula gives and transcodes back to its bytes.  No GPU."""
import os
import re
import struct

import pytest

from helpers import load_golden
from oracle.pyref.fields import CURVES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLS_G = bytes.fromhex("17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb"
                      "08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1")
BLS_O = b"\x40" + bytes(95)
BN_G = b"\x01" + bytes(31) + b"\x02" + bytes(31)
BN_O = bytes(63) + b"\x40"
LITERALS = {"bls12_381": (BLS_G, BLS_O), "bn254": (BN_G, BN_O)}
VK_LEN = {"bls12_381": (392, 728), "bn254": (280, 504)}
WIRE_ORDER = (0, 1, 4, 2, 3, 5)


def _code():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "polymath_hip.h")).read(), flags=re.S)


def test_the_enum_in_the_header_python_and_the_sys_crate():
    from polymath_amd import api
    code = _code()
    assert re.search(r"typedef\s+enum\s+pm_wire_form\s*\{\s*PM_WIRE_COMPRESSED\s*=\s*0\s*,\s*PM_WIRE_UNCOMPRESSED\s*=\s*256\s*\}\s*pm_wire_form\s*;", code)
    assert code.index("} pm_g1_status;") < code.index("pm_wire_form") < code.index("int pm_g1_decode(")
    sys_rs = open(os.path.join(ROOT, "rust", "polymath-hip-sys", "src", "lib.rs")).read()
    assert "pub const PM_WIRE_COMPRESSED: i32 = 0;" in sys_rs and "pub const PM_WIRE_UNCOMPRESSED: i32 = 256;" in sys_rs
    assert (api.PM_WIRE_COMPRESSED, api.PM_WIRE_UNCOMPRESSED) == (0, 256)
    assert api.WIRE_FORMS == {"compressed": 0, "uncompressed": 256}
    # pm_g1_status got no new value
    assert sorted(int(v) for v in re.findall(r"\bPM_G1_[A-Z_]+\s*=\s*(\d+)", code)) == list(range(7))
    wrapper = open(os.path.join(ROOT, "rust", "polymath-hip", "src", "lib.rs")).read()
    assert "pub enum WireForm" in wrapper and "Uncompressed = sys::PM_WIRE_UNCOMPRESSED" in wrapper
    assert "pub fn load_bytes_form<E: Pairing>" in wrapper and "validate as i32 | form as i32" in wrapper
    assert "pub fn export_bases_bytes<E: Pairing>" in wrapper and "which as i32 | form as i32" in wrapper


def test_the_header_states_the_contract():
    text = " ".join(open(os.path.join(ROOT, "include", "polymath_hip.h")).read().replace("*", " ").split())
    for phrase in ("validation is on iff (validate & ~256) != 0", "used to read as plain \"validate\"", "G1: not an uncompressed point",
                   "728 bytes on BLS12-381 and 504 on BN254", "the form is never guessed", "checked ALWAYS",
                   "keep taking and producing COMPRESSED vk and proof bytes", "(which & 255) >= PM_NUM_BASE_VECS"):
        assert phrase in text, phrase


def test_the_pinned_counts_still_hold():
    code = _code()
    assert len(set(re.findall(r"\b(pm_[a-z0-9_]+)\s*\(", code))) == 70
    assert re.search(r"\bPM_NUM_OPTIONS\s*=\s*9\b", code)
    from polymath_amd import api
    assert len(api.EXPORTS) == 70 and len(api.OPTIONS) == 9


class _StandIn:
    """records what the wrappers hand pm_g1_decode / pm_pk_load_bytes / pm_pk_export_bases_compressed"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


class _Ctx:
    h = None

    def __init__(self):
        self.L = _StandIn()

    def check(self, status):
        assert status == 0


def test_api_hands_the_library_the_flag():
    from polymath_amd import api
    ctx = _Ctx()
    for curve, cid in (("bls12_381", 0), ("bn254", 1)):
        nb = api.G1_BYTES[cid]
        assert (api.g1_record_bytes(cid), api.g1_record_bytes(cid, "uncompressed")) == (nb, 2 * nb)
        for form, flag, rec in (("compressed", 0, nb), ("uncompressed", 256, 2 * nb)):
            for validate in (True, False):
                ctx.L.calls.clear()
                xy, st = api.g1_decode(ctx, curve, bytes(3 * rec), validate, form=form)
                (name, args), = ctx.L.calls
                assert name == "pm_g1_decode" and args[3] == 3 and args[4] == int(validate) | flag and xy.shape[0] == 3 and len(st) == 3
            with pytest.raises(ValueError):
                api.g1_decode(ctx, curve, bytes(3 * rec + 16), True, form=form)
    with pytest.raises(KeyError):
        api.g1_decode(ctx, "bn254", bytes(64), True, form="long")
    pk = api.ProvingKey.__new__(api.ProvingKey)
    pk.ctx, pk.h, pk.cid, pk.base_lens = ctx, None, 0, [5] * 6
    for form, flag, rec in (("compressed", 0, 48), ("uncompressed", 256, 96)):
        ctx.L.calls.clear()
        out = pk.export_bases_compressed(4, 1, form=form)
        (name, args), = ctx.L.calls
        assert name == "pm_pk_export_bases_compressed" and args[2:5] == (4 | flag, 1, 4) and len(out) == 4 * rec


def _mult(c, k):
    from oracle.pyref.fields import g1_mul
    return g1_mul(c, c.g1, k)


@pytest.mark.parametrize("curve", ["bls12_381", "bn254"])
def test_python_twin_against_the_literals_and_integers(curve):
    from polymath_amd import polymath as PM
    c, f = CURVES[curve], PM.Field(curve)
    gen, inf = LITERALS[curve]
    nb = len(gen) // 2
    assert (c.g1[1] ** 2 - c.g1[0] ** 3 - c.b) % c.p == 0
    assert PM.ser_g1(f, c.g1, "uncompressed") == gen and PM.ser_g1(f, None, "uncompressed") == inf
    assert PM.deser_g1(f, gen, "uncompressed") == c.g1 and PM.deser_g1(f, inf, "uncompressed") is None
    assert PM.g1_bytes(f) == nb and PM.g1_bytes(f, "uncompressed") == 2 * nb and PM.g2_bytes(f, "uncompressed") == 4 * nb
    order = "big" if curve == "bls12_381" else "little"
    for k in (2, 3, 5, 0x1234567, c.r - 1):
        for P in (_mult(c, k), (_mult(c, k)[0], c.p - _mult(c, k)[1])):
            rec = PM.ser_g1(f, P, "uncompressed")
            body = bytearray(rec)
            if curve == "bn254":
                assert bool(body[63] & 0x80) == (P[1] > c.p - P[1]) and not body[63] & 0x40
                body[63] &= 0x3F
            assert (int.from_bytes(body[:nb], order), int.from_bytes(body[nb:], order)) == P
            assert PM.deser_g1(f, rec, "uncompressed") == P == PM.deser_g1(f, PM.ser_g1(f, P))
            if curve == "bn254":                      # the sign bit is not read
                flipped = rec[:63] + bytes([rec[63] ^ 0x80])
                assert PM.deser_g1(f, flipped, "uncompressed") == P
    bad = {}
    if curve == "bls12_381":
        bad["G1: not an uncompressed point"] = [bytes([gen[0] | 0x80]) + gen[1:], bytes([gen[0] | 0x20]) + gen[1:]]
        bad["G1: sign bit on the point at infinity"] = [b"\x60" + bytes(95)]
        top = lambda v: v.to_bytes(48, "big")
        bad["G1: coordinate >= p"] = [top(c.p) + gen[48:], gen[:48] + top(c.p), gen[:48] + top(c.p + 1), gen[:48] + b"\xff" * 48]
    else:
        bad["G1: both flag bits set"] = [bytes(63) + b"\xc0"]
        lo = lambda v: v.to_bytes(32, "little")
        bad["G1: coordinate >= p"] = [lo(c.p) + gen[32:], gen[:32] + lo(c.p), gen[:32] + lo(c.p + 1), b"\xff" * 32 + gen[32:]]
    bad["G1: non-canonical encoding of the point at infinity"] = [inf[:5] + b"\x01" + inf[6:], inf[:nb + 3] + b"\x01" + inf[nb + 4:]]
    y1 = (c.g1[1] + 1).to_bytes(nb, order)
    bad["G1: not on the curve"] = [gen[:nb] + y1]
    for why, recs in bad.items():
        for rec in recs:
            with pytest.raises(ValueError) as ex:
                PM.deser_g1(f, rec, "uncompressed")
            assert str(ex.value) == why, (why, rec.hex())
    with pytest.raises(ValueError):
        PM.ser_g1(f, c.g1, "long")


@pytest.mark.parametrize("curve", ["bls12_381", "bn254"])
def test_python_twin_g2_and_vk_in_both_forms(curve):
    """G2 on Python integers: the compressed bytes of api.make_vk (host C++: ser_vk_c) read by the twin, written uncompressed (728 /
    504 bytes), read again and written compressed give the same bytes; every uncompressed G2 is on the twist by its own equation."""
    from polymath_amd import api, polymath as PM
    c, f = CURVES[curve], PM.Field(curve)
    short, long = VK_LEN[curve]
    x, z = 0x1234567 % c.r, 0x7654321 % c.r
    vk_c = api.make_vk(curve, 8, 2, 11, f.fr_limbs([5])[0], f.fr_limbs([x])[0], f.fr_limbs([z])[0])
    assert len(vk_c) == short
    rd = PM._Reader(vk_c)
    vk = PM.VerifyingKey.read(f, rd)
    assert rd.o == short and vk.to_bytes() == vk_c
    vk_u = vk.to_bytes("uncompressed")
    assert len(vk_u) == long
    rd = PM._Reader(vk_u)
    vk2 = PM.VerifyingKey.read(f, rd, "uncompressed")
    assert rd.o == long and vk2.to_bytes() == vk_c and vk2.to_bytes("uncompressed") == vk_u
    assert (vk2.one_g1, vk2.one_g2, vk2.x_g2, vk2.z_g2) == (vk.one_g1, vk.one_g2, vk.x_g2, vk.z_g2)
    tb, p = PM._twist_b(f), c.p
    for (x0, x1), (y0, y1) in (vk.one_g2, vk.x_g2, vk.z_g2):
        xx = ((x0 * x0 - x1 * x1) % p, 2 * x0 * x1 % p)
        x3 = ((xx[0] * x0 - xx[1] * x1 + tb[0]) % p, (xx[0] * x1 + xx[1] * x0 + tb[1]) % p)
        assert ((y0 * y0 - y1 * y1) % p, 2 * y0 * y1 % p) == x3
    # the layout: the first G2 of the uncompressed vk holds the same x as the compressed one, then y
    g1n = 96 if curve == "bls12_381" else 64
    (x0, x1), (y0, y1) = vk.one_g2
    if curve == "bls12_381":
        assert vk_u[g1n:g1n + 192] == b"".join(v.to_bytes(48, "big") for v in (x1, x0, y1, y0))
    else:
        body = bytearray(vk_u[g1n:g1n + 128])
        body[-1] &= 0x3F
        assert bytes(body) == b"".join(v.to_bytes(32, "little") for v in (x0, x1, y0, y1))
    for wrong_bytes, form in ((vk_u, "compressed"), (vk_c, "uncompressed")):
        with pytest.raises(ValueError):
            rd = PM._Reader(wrong_bytes)
            PM.VerifyingKey.read(f, rd, form)
            if rd.o != len(wrong_bytes):
                raise ValueError("trailing bytes")
    G2_O = {"bls12_381": b"\x40" + bytes(191), "bn254": bytes(127) + b"\x40"}[curve]
    assert PM.ser_g2(f, None, "uncompressed") == G2_O and PM.deser_g2(f, G2_O, "uncompressed") is None


def transcode_key(data, field, form_from, form_to):
    """A BLS12-381 key string from one form into the other on Python integers (the twin's codecs) -> (bytes, points)"""
    from polymath_amd import polymath as PM
    rd = PM._Reader(data)
    out = [PM.VerifyingKey.read(field, rd, form_from).to_bytes(form_to)]
    start = rd.o
    rd.take(24)
    for _ in range(3):
        for _ in range(rd.u64()):
            rd.take(40 * rd.u64())
    out.append(rd.b[start:rd.o])
    n_in, points = PM.g1_bytes(field, form_from), 0
    for _ in WIRE_ORDER:
        cnt = rd.u64()
        points += cnt
        out.append(struct.pack("<Q", cnt))
        out.extend(PM.ser_g1(field, PM.deser_g1(field, rd.take(n_in), form_from), form_to) for _ in range(cnt))
    assert rd.o == len(rd.b)
    return b"".join(out), points


def test_transcoded_golden_key_has_the_length_of_the_formula():
    from polymath_amd import polymath as PM
    f = PM.Field("bls12_381")
    for key in load_golden("pk_wire.json")["keys"]:
        data = bytes.fromhex(key["pk_bytes"])
        wide, points = transcode_key(data, f, "compressed", "uncompressed")
        assert len(wide) == len(data) + 48 * points + (728 - 392), key["name"]
        assert wide[728:728 + 24] == data[392:392 + 24]
        back, points2 = transcode_key(wide, f, "uncompressed", "compressed")
        assert back == data and points2 == points, key["name"]
