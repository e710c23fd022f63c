"""GPU: PM_KEY_CHECK_RELATIONS in pm_pk_load_bytes (csrc/key_check.hip) -- is a key that passes point validation a proving key at all?

The specification is the host mirror (polymath_amd/host/key_check.hpp), which tests/native/key_check_selftest.cpp pins against a
literal restatement of the generator and tests/test_key_check_abi.py runs over the reference's own key bytes.  Here: valid keys at the
smallest shapes where the indexing can go wrong load with the flag and prove; every tamper is built from valid subgroup points on
Python integers, loads WITHOUT the flag (on the commit before the flag, 512 read as plain validation, so that load is what failed
there), and is refused with it, naming the relation, with device memory back where it was.
"""
import ctypes as ct

import pytest

from helpers import I, load_golden
from oracle.pyref.fields import CURVES, g1_mul
from test_gpu_pk_uncompressed import NB, VK_LEN, dec_c, enc_c, to_uncompressed, vec_offsets

CURVE_LIST = ["bls12_381", "bn254"]
SHAPES = {8: (1, 3), 16: (2, 5), 64: (12, 17)}            # domain -> (m0, rows): 2 (m0 + rows) <= domain
NAMES = ["x_powers_g1", "x_powers_y_alpha_g1", "x_powers_y_gamma_g1", "x_powers_y_gamma_z_g1", "x_powers_zh_by_y_alpha_g1",
         "uj_wj_lcs_by_y_alpha_g1"]
RATIO, ANCHOR, FIRST = ": consecutive entries are not in ratio x", ": is not anchored to vk.one_g1 and vk.z_g2", ": the first entry is not vk.one_g1"
LCS = NAMES[5] + ": does not match the SAP matrices"


def circuit(r, m0, nr, seed):
    """A satisfied R1CS of nr rows: row i multiplies two sums of earlier columns into its own witness column; two free witness
    columns in front, and a last witness column in no row (its uj_wj_lcs entry is the point at infinity)."""
    from polymath_amd import circuits as PC
    from polymath_amd import polymath as PM
    g = PC.SplitMix64(seed)
    mw = 2 + nr + 1
    z = [1] + [g.fr(r) for _ in range(m0 - 1 + 2)] + [0] * (nr + 1)
    a, b, c = [], [], []
    for i in range(nr):
        own = m0 + 2 + i
        ja, jb = g.fr(r) % own, 1 + g.fr(r) % (own - 1)   # own >= 3; no column twice in a row
        ra = [(g.fr(r), ja), (g.fr(r), (ja + 1) % own)]
        rb = [(g.fr(r), jb), (3, 0)]
        dot = lambda row: sum(v * z[j] for v, j in row) % r
        z[own] = dot(ra) * dot(rb) % r
        a.append(ra), b.append(rb), c.append([(1, own)])
    return PM.R1CS(m0, mw, a, b, c), z[:m0], z[m0:]


_MADE = {}


def made(gpu_ctx, curve, n, seed=1, trapdoors=0):
    """(pm, r1cs, instance, witness, x, z, vk bytes, key bytes) of a key made by Polymath.setup and pk_serialize, once a session"""
    from polymath_amd import circuits as PC
    from polymath_amd import polymath as PM
    key = (curve, n, seed, trapdoors)
    if key not in _MADE:
        c = CURVES[curve]
        m0, nr = SHAPES[n]
        r1cs, inst, wit = circuit(c.r, m0, nr, 100 * n + seed)
        g = PC.SplitMix64(0xC0FFEE + n + 1000 * trapdoors)
        x, z = g.fr(c.r), g.fr(c.r)
        pm = PM.Polymath(curve, "merlin", ctx=gpu_ctx)
        pk = pm.setup((r1cs, inst, wit), x, z)
        assert pk.n == n
        vk = pm.make_vk(pk, x, z)
        _MADE[key] = (r1cs, inst, wit, x, z, vk, pm.pk_serialize(pk, r1cs, vk))
        pk.free()
    return _MADE[key]


def free_bytes():
    """free device memory as the runtime reports it (hipMemGetInfo, the soak test's method)"""
    fr, tot = ct.c_size_t(), ct.c_size_t()
    assert ct.CDLL("libamdhip64.so").hipMemGetInfo(ct.byref(fr), ct.byref(tot)) == 0
    return fr.value


def load_prove_verify(pm, data, form, circ, relations=True):
    r1cs, inst, wit = circ
    pk, vk = pm.pk_load_bytes(data, True, form=form, relations=relations)
    proof = pm.prove(pk, (r1cs, inst, wit), [5, 7])
    vk_c = pm.vk_transcode(vk, form, "compressed") if form == "uncompressed" else vk
    assert pm.verify(vk_c, inst[1:], proof), "the proof of a key loaded with the relation check does not verify"
    pk.free()


# --------------------------------------------------------------------------------------------------------------- valid keys
@pytest.mark.gpu
@pytest.mark.parametrize("n", sorted(SHAPES))
@pytest.mark.parametrize("curve", CURVE_LIST)
def test_valid_keys_load_with_the_flag_and_prove(gpu_ctx, curve, n):
    from polymath_amd import polymath as PM
    r1cs, inst, wit, x, z, vk, data = made(gpu_ctx, curve, n)
    pm = PM.Polymath(curve, "merlin", ctx=gpu_ctx)
    offs = vec_offsets(data, curve, "compressed")
    off, cnt = offs[5]
    unused = off + NB[curve] * (r1cs.m0 + r1cs.mw - 1)
    assert dec_c(CURVES[curve], data[unused:unused + NB[curve]]) is None, "the unused witness column's entry is not the point at infinity"
    wide = to_uncompressed(data, curve)
    for form, blob in (("compressed", data), ("uncompressed", wide)):
        for tables in ("off", "auto", "wide"):
            gpu_ctx.set_option("tables", tables)
            load_prove_verify(pm, blob, form, (r1cs, inst, wit))
        gpu_ctx.set_option("tables", "auto")
        gpu_ctx.set_option("wire_chunk_log", 4)              # every vector but the two short ones spans several staging chunks
        load_prove_verify(pm, blob, form, (r1cs, inst, wit))
        gpu_ctx.set_option("wire_chunk_log", 20)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [k["name"] for k in load_golden("pk_wire.json")["keys"]])
def test_fixture_keys_pass_the_relations(gpu_ctx, name):
    from polymath_amd import polymath as PM
    key = [k for k in load_golden("pk_wire.json")["keys"] if k["name"] == name][0]
    data = bytes.fromhex(key["pk_bytes"])
    pm = PM.Polymath("bls12_381", "merlin", ctx=gpu_ctx)
    for form, blob in (("compressed", data), ("uncompressed", to_uncompressed(data, "bls12_381"))):
        pk, _ = pm.pk_load_bytes(blob, True, form=form, relations=True)
        if name in {x["name"] for x in load_golden("proofs.json")}:
            e = {x["name"]: x for x in load_golden("proofs.json")}[name]
            inst, wit, r_a = [I(v) for v in e["instance"]], [I(v) for v in e["witness"]], [I(v) for v in e["r_a"]]
            proof = pm.prove_limbs(pk, inst, pm.field.fr_limbs(inst), pm.field.fr_limbs(wit), r_a)
            assert proof.to_bytes().hex() == e["proofs"]["merlin"]["bytes"]
        pk.free()


# ------------------------------------------------------------------------------------------------------------------ tampers
def tampers(gpu_ctx, curve, n):
    """[(name, bytes, expected text)]: every tampered key is valid points throughout"""
    from polymath_amd import polymath as PM
    c = CURVES[curve]
    nb, vkl = NB[curve], VK_LEN[curve]
    r1cs, inst, wit, x, z, vk, data = made(gpu_ctx, curve, n)
    pm = PM.Polymath(curve, "merlin", ctx=gpu_ctx)
    offs = vec_offsets(data, curve, "compressed")

    def get(blob, v, i):
        o = offs[v][0] + nb * i
        return dec_c(c, blob[o:o + nb])

    def put(blob, v, i, P):
        o = offs[v][0] + nb * i
        return blob[:o] + enc_c(c, P) + blob[o + nb:]

    out = []
    mid = offs[0][1] // 2
    out.append(("x_powers_g1: adjacent entries swapped", put(put(data, 0, mid, get(data, 0, mid + 1)), 0, mid + 1, get(data, 0, mid)), NAMES[0] + RATIO))
    first = [NAMES[0] + FIRST] + [NAMES[v] + RATIO for v in range(1, 5)] + [LCS]
    last = [NAMES[v] + RATIO for v in range(5)] + [LCS]
    whole = [NAMES[0] + FIRST, NAMES[1] + ANCHOR, NAMES[2] + ANCHOR, NAMES[3] + ANCHOR, NAMES[4] + ANCHOR, LCS]
    for v in range(6):
        cnt = offs[v][1]
        out.append((NAMES[v] + ": first entry doubled", put(data, v, 0, g1_mul(c, get(data, v, 0), 2)), first[v]))
        out.append((NAMES[v] + ": last entry doubled", put(data, v, cnt - 1, g1_mul(c, get(data, v, cnt - 1), 2)), last[v]))
        blob = data
        for i in range(cnt):
            blob = put(blob, v, i, g1_mul(c, get(data, v, i), 2))
        out.append((NAMES[v] + ": every entry doubled", blob, whole[v]))
    m, Lz = r1cs.m0 + r1cs.mw, offs[5][1]
    for label, j in (("first R1CS column", 0), ("last R1CS column", m - 1), ("first y column", m), ("last y column", Lz - 1)):
        out.append(("uj_wj_lcs entry replaced: " + label, put(data, 5, j, g1_mul(c, c.g1, 7 + j)), LCS))
    g2 = 2 * nb                                              # a compressed G2 record; the vk is one_g1 | one_g2 | x_g2 | z_g2 | ...
    xs, zs = data[nb + g2:nb + 2 * g2], data[nb + 2 * g2:nb + 3 * g2]
    out.append(("x_g2 and z_g2 swapped", data[:nb + g2] + zs + xs + data[nb + 3 * g2:], NAMES[0] + RATIO))
    other = made(gpu_ctx, curve, n, trapdoors=1)             # the same circuit under other trapdoors
    pk = pm.setup((r1cs, inst, wit), x, z)
    out.append(("vk of another x", pm.make_vk(pk, other[3], z) + data[vkl:], NAMES[0] + RATIO))
    out.append(("vk of another z", pm.make_vk(pk, x, other[4]) + data[vkl:], NAMES[3] + ANCHOR))
    pk.free()
    twin = made(gpu_ctx, curve, n, seed=2)                   # another circuit of the same shape
    assert (twin[0].m0, twin[0].mw, twin[0].nr) == (r1cs.m0, r1cs.mw, r1cs.nr) and twin[0].a != r1cs.a
    head = offs[0][0] - 8
    out.append(("the matrices of one circuit with the bases of another", data[:head] + twin[6][head:], LCS))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("curve", CURVE_LIST)
def test_tampered_keys_load_without_the_flag_and_are_refused_with_it(gpu_ctx, curve):
    from polymath_amd import api
    from polymath_amd import polymath as PM
    n = 16
    pm = PM.Polymath(curve, "merlin", ctx=gpu_ctx)
    cases = tampers(gpu_ctx, curve, n)
    assert len(cases) == 1 + 18 + 4 + 3 + 1
    valid = made(gpu_ctx, curve, n)[6]
    pm.pk_load_bytes(valid, True, relations=True)[0].free()  # the context's workspaces have seen this shape
    failures = []
    for name, blob, text in cases:
        assert len(blob) == len(valid) and blob != valid, name
        pk, _ = pm.pk_load_bytes(blob, True)                 # every point is a valid subgroup point: plain validation accepts
        pk.free()
        before = free_bytes()
        try:
            pk, _ = pm.pk_load_bytes(blob, True, relations=True)
            pk.free()
            failures.append((name, "loaded"))
            continue
        except api.PolymathError as ex:
            if ex.status != 1 or not str(ex).endswith("pm_pk_load_bytes: " + text):
                failures.append((name, ex.status, str(ex)))
        after = free_bytes()
        if after < before:
            failures.append((name, "device memory", before, after))
    assert not failures, failures
    pm.pk_load_bytes(valid, True, relations=True)[0].free()  # and the context still accepts the valid key


@pytest.mark.gpu
def test_tampered_key_in_the_uncompressed_form(gpu_ctx):
    from polymath_amd import api
    from polymath_amd import polymath as PM
    curve = "bls12_381"
    pm = PM.Polymath(curve, "merlin", ctx=gpu_ctx)
    name, blob, text = [t for t in tampers(gpu_ctx, curve, 16) if t[0] == "uj_wj_lcs entry replaced: last y column"][0]
    wide = to_uncompressed(blob, curve)
    pm.pk_load_bytes(wide, True, form="uncompressed")[0].free()
    with pytest.raises(api.PolymathError) as ex:
        pm.pk_load_bytes(wide, True, form="uncompressed", relations=True)
    assert ex.value.status == 1 and str(ex.value).endswith("pm_pk_load_bytes: " + text), str(ex.value)


# ---------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.gpu
def test_the_flag_is_refused_on_shards_and_ignored_by_the_decoder(gpu_ctx):
    import numpy as np
    from polymath_amd import api
    from polymath_amd import polymath as PM
    curve = "bls12_381"
    data = made(gpu_ctx, curve, 16)[6]
    pm = PM.Polymath(curve, "merlin", ctx=gpu_ctx)
    for args in ((0, 2, "pairs"), (1, 2, "pairs"), (0, 1, "vector")):
        with pytest.raises(api.PolymathError) as ex:
            pm.pk_load_bytes(data, True, *args, relations=True)
        assert ex.value.status == 1 and "PM_KEY_CHECK_RELATIONS" in str(ex.value), str(ex.value)
    pm.pk_load_bytes(data, True, 0, 2, "pairs")[0].free()    # without the flag the shard loads as before
    # 512 alone is the flag with validation on (validation is on iff (validate & ~256) != 0)
    h = ct.c_void_p()
    keep, addr, nbytes = api._byte_view(data)
    assert gpu_ctx.L.pm_pk_load_bytes(gpu_ctx.h, 0, ct.c_void_p(addr), nbytes, 512, 0, 1, 0, ct.byref(h)) == 0 and h.value
    gpu_ctx.L.pm_pk_free(h)
    # pm_g1_decode reads 512 as it always did: plain "validate"
    off, cnt = vec_offsets(data, curve, "compressed")[0]
    recs = data[off:off + 48 * cnt]
    out_a, st_a = api.g1_decode(gpu_ctx, curve, recs, True)
    out = np.zeros((cnt, 12), dtype=np.uint64)
    st = np.zeros(cnt, dtype=np.uint8)
    keep, addr, nbytes = api._byte_view(recs)
    assert gpu_ctx.L.pm_g1_decode(gpu_ctx.h, 0, ct.c_void_p(addr), cnt, 512 | 1, api._p(out), st.ctypes.data_as(ct.c_void_p)) == 0
    assert (out == out_a).all() and (st == st_a).all() and not st.any()
